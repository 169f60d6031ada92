"""The value net's last layer at MANY pixels per image (csrc/fs_edgetrain.hip: fs_head_forward_pixels / fs_head_backward_pixels;
trainops.HeadPixelsFunction), SpatialValueNet.forward_pixels, train.optimize_maps(hip_step=True) and train.fit_maps on the GPU.

The float64 reference is F.conv2d on the host and its autograd, gathered at the listed pixels.  The bound is the project's own
(vn_reference.tolerance): max(4 e32, 2e-6 max(1, max |f64|)), e32 the larger error of the two stock fp32 paths -- host and GPU --
on the same tensors; test_edgetrain_gpu.compare prints every figure before anything is asserted.
Where the kernels split their work: the forward takes 4 list entries per workgroup; the data gradient's workgroups own 8-row
strips (rows 7 | 8, ..., 55 | 56) and scatter an image's list 256 entries per trip; a thread owns 4 neighbouring columns
(3 | 4, ..., 59 | 60); the weight gradient adds the list in chunks of 64 entries and the chunk sums in 16 slices (one
chunk more than 16 at 1025 entries).  No malformed table goes to a kernel here: the host checks are tested without a GPU."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_edgetrain_gpu as eg
import vn_reference as ref
from test_edgetrain_gpu import compare

pytestmark = pytest.mark.gpu

D = 64
DEV = "cuda:0"


def _nets():
    from flingbot_amd import nets
    return nets


def table(lists):
    """(offsets int64 [B + 1], flat pixels int32 [L]) of per-image lists of (y, x)."""
    offsets = np.concatenate([[0], np.cumsum([len(rows) for rows in lists])]).astype(np.int64)
    return offsets, np.array([y * D + x for rows in lists for y, x in rows], np.int32)


def pixels(h, w, lists, gpred=None):
    """(pred, dh, dw) of the kernels for host tensors."""
    fn = _nets().HeadPixelsFunction
    offsets, pix = table(lists)
    hd, wd = h.to(DEV).contiguous(), w.to(DEV).contiguous()
    od, pd = torch.from_numpy(offsets.astype(np.int32)).to(DEV), torch.from_numpy(pix).to(DEV)
    pred = fn._forward(hd, wd, od, pd)
    if gpred is None:
        return pred, None, None
    dh, dw = fn._backward(hd, wd, od, pd, gpred.to(DEV).contiguous())
    return pred, dh, dw


def stock(h, w, lists, gpred, dtype, device):
    """dense F.conv2d -> gather at [b(l), pix[l]] -> autograd, as float64 host tensors."""
    offsets, pix = table(lists)
    image = torch.from_numpy(np.repeat(np.arange(len(lists)), np.diff(offsets))).to(device)
    h = h.to(device=device, dtype=dtype).requires_grad_(True)
    w = w.to(device=device, dtype=dtype).requires_grad_(True)
    pred = F.conv2d(h, w, padding=1).reshape(len(lists), -1)[image, torch.from_numpy(pix).long().to(device)]
    dh, dw = torch.autograd.grad(pred, (h, w), gpred.to(device=device, dtype=dtype))
    return tuple(t.detach().double().cpu() for t in (pred, dh, dw))


def drawn(rng, count):
    """`count` distinct pixels, in drawn (unsorted) order."""
    return [divmod(int(p), D) for p in rng.permutation(D * D)[:count]]


def lattice(first, last, stride):
    return [(y, x) for y in range(first, last + 1, stride) for x in range(first, last + 1, stride)]


def _cases():
    rng = np.random.default_rng(2)
    cases = {"B=1, one pixel": [[(20, 40)]]}
    for counts in ([0, 1, 7], [5, 0, 0], [2, 0, 3]):
        cases[f"counts {counts}"] = [drawn(rng, c) for c in counts]
    cases["corners and edges"] = [[(0, 0), (0, 63), (63, 0), (63, 63), (0, 31), (31, 0), (63, 31), (31, 63)],
                                  [(63, 63), (0, 0), (7, 5), (8, 5), (55, 60), (56, 59)]]
    cases["blocks and a row"] = [[(3, 3), (3, 4), (4, 3), (4, 4)], [(y, x) for y in (58, 59, 60) for x in (58, 59, 60)],
                                 [(17, x) for x in range(D)]]
    cases["stride-4 lattice 12 x 12"] = [lattice(8, 55, 4), [(9, 9)]]
    cases["stride-1 lattice 48 x 48"] = [[(9, 9)], lattice(8, 55, 1)]
    cases["all 4096 pixels, shuffled"] = [drawn(rng, 4096), drawn(rng, 3)]
    # either side of the weight gradient's 64-entry chunks, of its 16 slices of chunk sums, of the scatter's 256-entry trips
    for counts in ([30, 33], [64, 0], [1, 64], [256, 257], [1000, 24], [1, 1024]):
        cases[f"{sum(counts)} entries {counts}"] = [drawn(rng, c) for c in counts]
    return cases


CASES = _cases()


def test_the_cases_are_what_the_docstring_says():
    assert [len(rows) for rows in CASES["stride-4 lattice 12 x 12"]] == [144, 1] and CASES["stride-4 lattice 12 x 12"][0][-1] == (52, 52)
    assert [len(rows) for rows in CASES["stride-1 lattice 48 x 48"]] == [1, 2304]
    assert sorted(CASES["all 4096 pixels, shuffled"][0]) == [divmod(p, D) for p in range(4096)]
    assert CASES["all 4096 pixels, shuffled"][0] != sorted(CASES["all 4096 pixels, shuffled"][0])
    assert sorted(sum(len(r) for r in rows) for name, rows in CASES.items() if "entries" in name) == [63, 64, 65, 513, 1024, 1025]
    for rows in CASES.values():
        for image in rows:
            assert len(set(image)) == len(image)


@pytest.mark.parametrize("name", list(CASES))
def test_against_float64(gpu_required, name):
    lists = CASES[name]
    gen = torch.Generator().manual_seed(len(name))
    n = sum(len(rows) for rows in lists)
    h = torch.randn(len(lists), 16, D, D, generator=gen)
    w = torch.randn(1, 16, 3, 3, generator=gen) * 0.3
    gpred = torch.randn(n, generator=gen)
    got = pixels(h, w, lists, gpred)
    want = stock(h, w, lists, gpred, torch.float64, "cpu")
    host = stock(h, w, lists, gpred, torch.float32, "cpu")
    gpu = stock(h, w, lists, gpred, torch.float32, DEV)
    failed = []
    for k, what in enumerate(("pred", "dh", "dw")):
        compare(f"{name}: {what}", got[k], want[k], host[k], gpu[k], failed)
    assert not failed, failed
    # +0 bit for bit wherever no listed pixel's patch reaches, every plane of an image without entries included
    outside = torch.ones(len(lists), 16, D, D, dtype=torch.bool)
    for b, rows in enumerate(lists):
        for y, x in rows:
            outside[b, :, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = False
    bits = got[1].cpu().view(torch.int32)
    assert bool((bits[outside] == 0).all()) and bool((want[1][outside] == 0).all())
    if name != "all 4096 pixels, shuffled":
        assert int(outside.sum()) > 0
    else:      # the dense convolution and its whole backward
        dense = F.conv2d(h[:1].double(), w.double(), padding=1).reshape(-1)
        order = torch.tensor([y * D + x for y, x in lists[0]])
        assert torch.allclose(want[0][:4096], dense[order], rtol=0.0, atol=1e-12)


@pytest.mark.parametrize("name", ["corners and edges", "blocks and a row", "stride-1 lattice 48 x 48", "all 4096 pixels, shuffled",
                                  "counts [0, 1, 7]", "1025 entries [1, 1024]"])
def test_ones_count_every_term(gpu_required, name):
    """h = 1, W = 1, g = 1: pred is 16 x the number of in-image taps, dh the number of listed pixels whose patch covers the point,
    dw the number of list entries whose tap lies in the image -- small integers, so the comparison is for equality."""
    lists = CASES[name]
    n = sum(len(rows) for rows in lists)
    pred, dh, dw = pixels(torch.ones(len(lists), 16, D, D), torch.ones(1, 16, 3, 3), lists, torch.ones(n))
    taps = torch.zeros(n)
    cover = torch.zeros(len(lists), D, D)
    count = torch.zeros(3, 3)
    flat = [(b, y, x) for b, rows in enumerate(lists) for y, x in rows]
    for l, (b, y, x) in enumerate(flat):
        for ky in range(3):
            for kx in range(3):
                yy, xx = y + ky - 1, x + kx - 1
                if 0 <= yy < D and 0 <= xx < D:
                    taps[l] += 1
                    cover[b, yy, xx] += 1
                    count[ky, kx] += 1
    assert torch.equal(pred.cpu(), 16 * taps)
    assert torch.equal(dh.cpu(), cover[:, None].expand(len(lists), 16, D, D))
    assert torch.equal(dw.cpu(), count.expand(1, 16, 3, 3))


@pytest.mark.parametrize("batch", [1, 7, 128])
def test_one_pixel_per_image_is_the_one_pixel_head(gpu_required, batch):
    """pred and dh equal HeadPixelFunction's (torch.equal); dw, whose sum runs in another order, is within the bound."""
    gen = torch.Generator().manual_seed(batch)
    rng = np.random.default_rng(batch)
    pix = [(0, 0), (63, 63), (0, 40), (31, 63)][:batch] + [divmod(int(p), D) for p in rng.integers(0, D * D, max(batch - 4, 0))]
    h = torch.randn(batch, 16, D, D, generator=gen)
    w = torch.randn(1, 16, 3, 3, generator=gen) * 0.3
    gpred = torch.randn(batch, generator=gen)
    lists = [[p] for p in pix]
    got = pixels(h, w, lists, gpred)
    one = eg.head(h, w, pix, gpred)
    assert torch.equal(got[0], one[0]) and torch.equal(got[1], one[1])
    want, host, gpu = (stock(h, w, lists, gpred, dt, dv) for dt, dv in ((torch.float64, "cpu"), (torch.float32, "cpu"), (torch.float32, DEV)))
    failed = []
    compare(f"one pixel per image, B={batch}: dw", got[2], want[2], host[2], gpu[2], failed)
    compare(f"one pixel per image, B={batch}: dw of the one-pixel head", one[2], want[2], host[2], gpu[2], failed)
    assert not failed, failed


def test_three_calls_give_identical_bits(gpu_required):
    lists = CASES["1025 entries [1, 1024]"] + CASES["stride-4 lattice 12 x 12"]
    gen = torch.Generator().manual_seed(5)
    h = torch.randn(len(lists), 16, D, D, generator=gen)
    w = torch.randn(1, 16, 3, 3, generator=gen)
    gpred = torch.randn(sum(len(r) for r in lists), generator=gen)
    first = pixels(h, w, lists, gpred)
    for _ in range(2):
        for a, b in zip(first, pixels(h, w, lists, gpred)):
            assert torch.equal(a, b)


def test_an_image_does_not_depend_on_its_batch(gpu_required):
    """pred and dh of an image, bit for bit, alone and with other images (listing many, few and no pixels) before and after it."""
    rng = np.random.default_rng(8)
    gen = torch.Generator().manual_seed(8)
    mine = drawn(rng, 300)
    others = [drawn(rng, 77), [], drawn(rng, 1000), drawn(rng, 2)]
    h = torch.randn(5, 16, D, D, generator=gen)
    w = torch.randn(1, 16, 3, 3, generator=gen)
    g_mine, g_others = torch.randn(300, generator=gen), [torch.randn(len(o), generator=gen) for o in others]
    alone = pixels(h[:1], w, [mine], g_mine)
    for place in (0, 2, 4):
        lists = others[:place] + [mine] + others[place:]
        order = list(range(1, place + 1)) + [0] + list(range(place + 1, 5))
        gpred = torch.cat(g_others[:place] + [g_mine] + g_others[place:])
        pred, dh, _ = pixels(h[order], w, lists, gpred)
        first = sum(len(o) for o in others[:place])
        assert torch.equal(pred[first:first + 300], alone[0]), place
        assert torch.equal(dh[place], alone[1][0]), place


def test_function_and_what_it_refuses(gpu_required):
    fn = _nets().HeadPixelsFunction
    lists = CASES["counts [0, 1, 7]"]
    offsets, pix = table(lists)
    gen = torch.Generator().manual_seed(35)
    h, w, gpred = torch.randn(3, 16, D, D, generator=gen), torch.randn(1, 16, 3, 3, generator=gen), torch.randn(8, generator=gen)
    hd, wd = h.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    pd = torch.from_numpy(pix).to(DEV).long()                       # int64 is taken too
    pd.host = pix
    before = (fn.n_forward, fn.n_backward)
    pred = fn.apply(hd, wd, offsets, pd)
    pred.backward(gpred.to(DEV))
    assert (fn.n_forward, fn.n_backward) == (before[0] + 1, before[1] + 1)
    want = pixels(h, w, lists, gpred)
    assert torch.equal(pred.detach(), want[0]) and torch.equal(hd.grad, want[1]) and torch.equal(wd.grad, want[2])
    assert torch.equal(fn.apply(hd, wd, torch.from_numpy(offsets), pd).detach(), want[0])          # a host tensor of offsets
    bad_pixels = torch.from_numpy(pix).to(DEV)
    bad_pixels.host = np.concatenate([pix[:7], pix[6:7]])           # the host copy names a pixel twice in image 2
    for args in ((hd[:, :8], wd, offsets, pd), (hd, wd[:, :8], offsets, pd), (hd, wd, offsets, pd.float()), (hd, wd, offsets, pd[:0]),
                 (hd, wd, offsets, pd[:4]), (hd, wd, offsets[:3], pd), (hd, wd, offsets + 1, pd), (hd, wd, offsets[::-1].copy(), pd),
                 (hd, wd, torch.from_numpy(offsets).to(DEV), pd), (hd, wd, offsets, bad_pixels), (hd.double(), wd, offsets, pd),
                 (hd, wd, offsets, pd.cpu())):
        with pytest.raises(ValueError):
            fn.apply(*args)
    assert (fn.n_forward, fn.n_backward) == (before[0] + 2, before[1] + 1)


# ---- a real network -------------------------------------------------------------------------------------------------------------
def _lists_4x3():
    return [[(0, 0), (0, 1), (1, 0)], [(63, 63), (20, 40), (33, 3)], [(8, 8), (7, 60), (40, 4)], [(31, 31), (32, 32), (56, 0)]]


@pytest.mark.parametrize("mode", ["rgb", "depth", "rgbd"])
def test_forward_pixels_agrees_with_the_dense_forward(gpu_required, mode):
    """forward_pixels with the edge switch on against the gather of the switch-off dense forward, same net and batch: both within
    the bound of the float64 train-mode forward, e32 from the host and the all-stock GPU forward -- the comparison of
    test_edgetrain_gpu.test_forward_selected_agrees_with_the_dense_forward, at 4 images x 3 pixels."""
    nets = _nets()
    flags = dict(rgb_only=mode == "rgb", depth_only=mode == "depth")
    net = eg._net(47, **flags)
    obs = ref.make_obs(4, 47)
    offsets, pix = table(_lists_4x3())
    image = torch.from_numpy(np.repeat(np.arange(4), 3))
    sel = lambda out: out.reshape(4, -1)[image.to(out.device), torch.from_numpy(pix).long().to(out.device)]   # noqa: E731
    pd = torch.from_numpy(pix).to(DEV)
    with torch.no_grad():
        want = sel(copy.deepcopy(net).cpu().double().train()(obs.double()))
        host = sel(copy.deepcopy(net).cpu().train()(obs)).double()
        saved = (nets._TRAIN_CONV_HIP, nets._TRAIN_BN_HIP)
        try:
            nets._TRAIN_CONV_HIP, nets._TRAIN_BN_HIP = False, False
            gpu = sel(copy.deepcopy(net).train()(obs.to(DEV))).double().cpu()
        finally:
            nets._TRAIN_CONV_HIP, nets._TRAIN_BN_HIP = saved
        dense = sel(copy.deepcopy(net).train()(obs.to(DEV)))
        calls = (nets.ConvInFunction.n_forward, nets.HeadPixelsFunction.n_forward)
        with nets.train_edge_hip():
            got = copy.deepcopy(net).train().forward_pixels(obs.to(DEV), offsets, pd)
        assert (nets.ConvInFunction.n_forward, nets.HeadPixelsFunction.n_forward) == (calls[0] + 1, calls[1] + 1)
        # outside the context, and in eval mode inside it: the dense forward gathered, bit for bit, and no Function
        assert torch.equal(copy.deepcopy(net).train().forward_pixels(obs.to(DEV), offsets, pd), dense)
        eval_net = copy.deepcopy(net).eval()
        with nets.train_edge_hip():
            assert torch.equal(eval_net.forward_pixels(obs.to(DEV), offsets, pd), sel(eval_net(obs.to(DEV))))
        assert nets.HeadPixelsFunction.n_forward == calls[1] + 1
    failed = []
    compare(f"{mode}: forward_pixels, switch on", got, want, host, gpu, failed)
    compare(f"{mode}: dense forward, switch off", dense, want, host, gpu, failed)
    assert not failed, failed


def test_parameter_gradients_against_float64(gpu_required):
    """One forward_pixels + mse_loss backward on 4 images x 3 pixels inside train_edge_hip(): every parameter gradient against the
    float64 host gradient, e32 from the two stock fp32 paths (host, and the GPU with every switch off)."""
    nets = _nets()
    net = eg._net(53)
    obs = ref.make_obs(4, 53, channels=3)
    offsets, pix = table(_lists_4x3())
    label = torch.from_numpy(np.random.default_rng(53).uniform(-0.1, 0.2, 12).astype(np.float32))

    def gradients(model, device, dtype, edge):
        model = model.train()
        with nets.train_edge_hip(edge):
            pred = model.forward_pixels(obs.to(device=device, dtype=dtype), offsets, torch.from_numpy(pix).to(device))
        F.mse_loss(pred, label.to(device=device, dtype=dtype)).backward()
        return {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None}

    f64 = copy.deepcopy(net).cpu().double()
    f64.mean, f64.std = f64.mean.double(), f64.std.double()
    want = gradients(f64, "cpu", torch.float64, False)
    host = gradients(copy.deepcopy(net).cpu(), "cpu", torch.float32, False)
    saved = (nets._TRAIN_CONV_HIP, nets._TRAIN_BN_HIP)
    try:
        nets._TRAIN_CONV_HIP, nets._TRAIN_BN_HIP = False, False
        gpu = gradients(copy.deepcopy(net), DEV, torch.float32, False)
    finally:
        nets._TRAIN_CONV_HIP, nets._TRAIN_BN_HIP = saved
    fns = (nets.ConvInFunction, nets.HeadPixelsFunction, nets.Conv16Function, nets.BatchNormAct16Function)
    calls = [(f.n_forward, f.n_backward) for f in fns]
    mine = copy.deepcopy(net).train()
    with nets.train_edge_hip():
        pred = mine.forward_pixels(obs.to(DEV), offsets, torch.from_numpy(pix).to(DEV))
    F.mse_loss(pred, label.to(DEV)).backward()
    assert [(f.n_forward - c[0], f.n_backward - c[1]) for f, c in zip(fns, calls)] == [(1, 1), (1, 1), (16, 16), (17, 17)]
    assert set(want) == set(host) == set(gpu) and len(want) == 2 + 16 + 2 * 17
    failed = []
    for name, p in mine.named_parameters():
        if name in want:
            compare(f"gradient of {name}", p.grad, want[name], host[name], gpu[name], failed)
        else:
            assert p.grad is None, name
    assert not failed, failed


# ---- the update -----------------------------------------------------------------------------------------------------------------
def map_set(n_images=8, n_pixels=6, seed=0):
    """A fixed set of images in the style of test_vntrain_gpu.learning_set with `n_pixels` labelled pixels each, labels in
    [-0.1, 0.2], no colour jitter: the set is to be memorised."""
    import test_vntrain_gpu as vt
    from flingbot_amd import replay

    rng = np.random.default_rng(seed)
    obs = vt.learning_set(seed, n_images).observations
    lists = [drawn(rng, n_pixels) for _ in range(n_images)]
    offsets, pix = table(lists)
    labels = rng.uniform(-0.1, 0.2, len(pix)).astype(np.float32)
    return replay.MapSet.from_arrays(obs, offsets, pix, labels, obs_color_jitter=False)


def test_wiring_of_a_dense_hip_step(gpu_required, monkeypatch):
    """With F.conv2d and F.batch_norm made to raise, one optimize_maps(hip_step=True) update with a HipAdam completes: one
    HeadPixelsFunction call forward and one backward (and none of the one-pixel head), one first-layer call, one fs_adam_step,
    value_net.steps + 1 -- what test_edgetrain_gpu.test_wiring_of_a_hip_step checks of optimize."""
    from flingbot_amd import nets, train

    net = eg._net(43).train()
    data = map_set().to_device(DEV)
    opt = train.HipAdam(net.parameters(), lr=1e-3, weight_decay=1e-6)
    before_state = {k: v.clone() for k, v in net.state_dict().items()}

    def refuse(*args, **kwargs):
        raise AssertionError("a library operator was called inside a hip_step update")

    deterministic = torch.backends.cudnn.deterministic
    monkeypatch.setattr(F, "conv2d", refuse)
    monkeypatch.setattr(F, "batch_norm", refuse)
    fns = (nets.ConvInFunction, nets.HeadPixelsFunction, nets.HeadPixelFunction, nets.Conv16Function, nets.BatchNormAct16Function)
    calls = [(f.n_forward, f.n_backward) for f in fns]
    launches, steps = train.HipAdam.n_launches, int(net.steps)
    rows = []
    losses = train.optimize_maps("fling", net, opt, data, 1, 8, np.random.default_rng(0), hip_step=True, stats=rows)
    monkeypatch.undo()
    assert len(losses) == 1 and np.isfinite(losses[0]) and rows == [dict(loss=losses[0], images=8, labels=48)]
    assert [(f.n_forward - c[0], f.n_backward - c[1]) for f, c in zip(fns, calls)] == [(1, 1), (1, 1), (0, 0), (16, 16), (17, 17)]
    assert train.HipAdam.n_launches == launches + 1 and int(net.steps) == steps + 1
    assert torch.backends.cudnn.deterministic == deterministic and nets._TRAIN_EDGE_HIP is False
    after = net.state_dict()
    changed = [k for k in after if not torch.equal(after[k], before_state[k])]
    assert len(changed) == len(after), sorted(set(after) - set(changed))     # every weight, buffer and counter moved
    # the ranked form: one segment per image, one fs_group_loss launch
    from flingbot_amd.trainops import GroupLossFunction
    group = GroupLossFunction.n_forward
    rows = []
    train.optimize_maps("fling", net, opt, data, 1, 8, np.random.default_rng(1), pixels_per_image=4, hip_step=True, rank_weight=0.5, stats=rows)
    assert GroupLossFunction.n_forward == group + 1 and rows[0]["labels"] == 32 and 0 < rows[0]["pairs"] <= 8 * 6
    assert nets.HeadPixelsFunction.n_forward - calls[1][0] == 2


def _updates(n_updates, seed=0):
    from flingbot_amd import nets, train

    torch.manual_seed(seed)
    net = nets.SpatialValueNet(rgb_only=True, device=DEV).to(DEV)
    opt = train.HipAdam(net.parameters(), lr=1e-3, weight_decay=1e-6)
    data = map_set().to_device(DEV)
    net.train()
    losses = train.optimize_maps("fling", net, opt, data, n_updates, 8, np.random.default_rng(seed), hip_step=True)
    net.eval()
    return losses, net, opt


def test_dense_updates_learn_and_two_runs_end_with_the_same_bits(gpu_required):
    """30 updates on a fixed set of 8 images x 6 pixels, twice from one seed: the loss falls (mean of updates 1-5 against 26-30)
    and every entry of the state_dict and of the optimizer's state is the same, bit for bit."""
    losses, net, opt = _updates(30)
    losses_again, net_again, opt_again = _updates(30)
    first, last = float(np.mean(losses[:5])), float(np.mean(losses[25:]))
    print(f"mean loss of updates 1-5 {first:.4e}, of updates 26-30 {last:.4e}")
    assert len(losses) == 30 and all(np.isfinite(losses)) and last < first and int(net.steps) == 30
    assert losses == losses_again
    a, b = net.state_dict(), net_again.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    sa, sb = opt.state_dict()["state"], opt_again.state_dict()["state"]
    assert list(sa) == list(sb) and len(sa) == 2 + 16 + 2 * 17
    for k in sa:
        for name in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(sa[k][name], sb[k][name]), (k, name)


def test_sample_maps_on_the_device_is_the_host_path(gpu_required):
    """The images through fs_replay_sample, the lists in one upload: the same numbers as the host path, jitter included."""
    from flingbot_amd import replay

    host = map_set(5, 9)
    host.obs_color_jitter = True
    dev = replay.MapSet.from_arrays(host.images, host.offsets, host.pixels, host.labels, obs_color_jitter=True).to_device(DEV)
    assert dev.resident_bytes() == 5 * (4 * D * D * 4 + D * D + 4) and host.resident_bytes() == 0
    for ppi in (None, 4):
        want = host.sample_maps(7, np.random.default_rng(3), ppi)
        got = dev.sample_maps(7, np.random.default_rng(3), ppi)
        assert got[0].is_cuda and got[2].is_cuda and got[3].is_cuda and tuple(got[0].shape) == (7, 3, D, D)
        assert torch.equal(got[0].cpu(), want[0]) and np.array_equal(got[1], want[1])
        assert torch.equal(got[2].cpu(), want[2]) and np.array_equal(got[2].host, want[2].host) and got[2].dtype == torch.int32
        assert torch.equal(got[3].cpu(), want[3]) and got[3].dtype == torch.float32


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def test_probe_run_to_map_set_to_fit_maps(gpu_required, tmp_path):
    """The smallest probe run of tests/test_probe_gpu.py (2 tasks, stride 16, step 0, 18 free slots) with record_experience,
    saved through lookahead.save_replay: the MapSet has one image per non-empty map with n_executed labels each, and fit_maps
    with 2 updates, twice from scratch, leaves identical checkpoints."""
    import random

    import test_probe_gpu as tp
    from flingbot_amd import lookahead, nets, replay, sim as fsim, tasks as ftasks, train

    random.seed(tp.SEED); np.random.seed(tp.SEED)
    gen = fsim.FlingSim(n_envs=2, solver=0)
    tasks = ftasks.generate_tasks(gen, [ftasks.draw_task_parameters(min_cloth_size=24, strict_min_edge_length=24, max_cloth_size=32)
                                        for _ in range(2)])
    gen.close()
    assert all(t is not None for t in tasks)
    probed = tp._probe(tasks, 20)
    path = str(tmp_path / "probes.npz")
    n = lookahead.save_replay(path, probed, tasks)
    maps = [m for m in probed["probe"]["maps"] if m["n_executed"] > 0]
    assert n == sum(m["n_executed"] for m in maps) >= 4 and len(maps) >= 1
    data = replay.MapSet([path], action_primitive="fling")
    entries = replay.ExperienceSet([path], action_primitive="fling")
    assert len(data) == len(maps) and np.diff(data.offsets).tolist() == [m["n_executed"] for m in maps]
    assert data.n_duplicate == 0 and data.n_invalid == 0 and len(entries) == n
    assert sorted(data.entry_keys) == sorted(entries.keys)
    label_of = dict(zip(entries.keys, entries.labels))
    assert np.array_equal(data.labels.view(np.int32), np.array([label_of[k] for k in data.entry_keys], np.float32).view(np.int32))
    for i, m in enumerate(maps):     # the listed pixels are the executed cells of the map's lattice
        cells = {(m["origin"][0] + int(a) * tp.STRIDE) * D + m["origin"][1] + int(b) * tp.STRIDE for a, b in np.argwhere(~np.isnan(m["measured"]))}
        assert set(data.pixels[data.offsets[i]:data.offsets[i + 1]].tolist()) == cells

    logs = [str(tmp_path / "a"), str(tmp_path / "b")]
    for log in logs:
        torch.manual_seed(7)
        policy = nets.MaximumValuePolicy(action_primitives=["fling"], num_rotations=tp.E_ROTATIONS, scale_factors=list(tp.E_SCALES),
                                         obs_dim=64, pix_grasp_dist=8, pix_drag_dist=8, pix_place_dist=5, rgb_only=True,
                                         depth_only=False, action_expl_prob=0.0, action_expl_decay=1.0, value_expl_prob=0.0,
                                         value_expl_decay=1.0, device=DEV)
        out = train.fit_maps(policy, train.make_optimizer(policy, hip=True), [path], log, 2, images_per_batch=len(maps), seed=3, hip_step=True)
        assert out["steps"] == 2 and out["primitives"]["fling"]["updates"] == 2 and out["primitives"]["fling"]["labels"] == n
        assert sorted(os.listdir(log)) == ["ckpt_000002.pth", "latest_ckpt.pth", "train_log.jsonl"]
    ckpts = [torch.load(os.path.join(d, train.LATEST), map_location="cpu") for d in logs]
    for k, v in ckpts[0]["net"].items():
        assert torch.equal(v, ckpts[1]["net"][k]), k
    sa, sb = ckpts[0]["optimizer"]["state"], ckpts[1]["optimizer"]["state"]
    assert list(sa) == list(sb) and len(sa) > 0
    for k in sa:
        for name in sa[k]:
            assert torch.equal(sa[k][name], sb[k][name]), (k, name)
    with open(os.path.join(logs[0], train.TRAIN_LOG)) as fa, open(os.path.join(logs[1], train.TRAIN_LOG)) as fb:
        assert fa.read() == fb.read()
