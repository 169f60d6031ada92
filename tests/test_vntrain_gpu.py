"""The training kernels (csrc/fs_vntrain.hip) through nets.Conv16Function, one operation at a time against float64, and
the training loop (flingbot_amd/train.py) on the GPU.

The float64 reference is torch.nn.functional.conv2d with autograd on the host.  The bound is the project's own
(vn_reference.tolerance): max(4 e32, 2e-6 max(1, max |f64|)), where e32 is the larger error of the two stock fp32 paths on
the same tensors -- host F.conv2d and GPU F.conv2d."""
import copy
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vn_reference as ref

pytestmark = pytest.mark.gpu

D = 64
SEAM_ROWS = [r for s in range(8, 64, 8) for r in (s - 1, s)]          # both rows on either side of every strip seam
PIXELS = [(0, 0), (0, 63), (63, 0), (63, 63)] + [(r, (15, 16, 31, 48)[k % 4]) for k, r in enumerate(SEAM_ROWS)]
DEV = "cuda:0"


def _fn():
    from flingbot_amd import nets
    return nets.Conv16Function


def conv(x, w, transposed=0):
    return _fn()._conv(x.contiguous(), w.contiguous(), transposed)


def wgrad(x, g):
    return _fn()._wgrad(x.contiguous(), g.contiguous())


def _in(y, x):
    return 0 <= y < D and 0 <= x < D


# ---- 1. exact cases ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 9])
def test_ones_count_every_term(gpu_required, batch):
    ones = torch.ones(batch, 16, D, D, device=DEV)
    w = torch.ones(16, 16, 3, 3, device=DEV)
    want = torch.full((D, D), 144.0)
    want[0, :] = want[-1, :] = want[:, 0] = want[:, -1] = 96.0
    want[0, 0] = want[0, -1] = want[-1, 0] = want[-1, -1] = 64.0
    for transposed in (0, 1):
        y = conv(ones, w, transposed).cpu()
        assert torch.equal(y, want.expand(batch, 16, D, D)), transposed
    dw = wgrad(ones, ones).cpu()
    taps = torch.tensor([[3969.0, 4032.0, 3969.0], [4032.0, 4096.0, 4032.0], [3969.0, 4032.0, 3969.0]]) * batch
    assert torch.equal(dw, taps.expand(16, 16, 3, 3))


@pytest.mark.parametrize("batch", [1, 9])
def test_impulses_at_corners_and_strip_seams(gpu_required, batch):
    g_cpu = torch.Generator().manual_seed(5)
    w = torch.randint(-3, 4, (16, 16, 3, 3), generator=g_cpu).float()
    w_dev = w.to(DEV)
    ones = torch.ones(batch, 16, D, D, device=DEV)
    for k, (py, px) in enumerate(PIXELS):
        b0, ch = k % batch, (5 * k + 3) % 16
        imp = torch.zeros(batch, 16, D, D)
        imp[b0, ch, py, px] = 1.0
        imp_dev = imp.to(DEV)
        # weight gradient of x = 1 with g = the impulse: the 0 / 1 in-bounds pattern in row `ch`, nothing elsewhere
        want_dw = torch.zeros(16, 16, 3, 3)
        for ky in range(3):
            for kx in range(3):
                want_dw[ch, :, ky, kx] = float(_in(py + ky - 1, px + kx - 1))
        assert torch.equal(wgrad(ones, imp_dev).cpu(), want_dw), (py, px)
        # ... and with the roles swapped (x the impulse, g = 1): column `ch`, taps mirrored
        want_dw = torch.zeros(16, 16, 3, 3)
        for ky in range(3):
            for kx in range(3):
                want_dw[:, ch, ky, kx] = float(_in(py - ky + 1, px - kx + 1))
        assert torch.equal(wgrad(imp_dev, ones).cpu(), want_dw), (py, px)
        # forward of the impulse: the flipped filter around the pixel; data gradient: the filter itself; clipped at the border
        want_y, want_dx = torch.zeros(batch, 16, D, D), torch.zeros(batch, 16, D, D)
        for ky in range(3):
            for kx in range(3):
                if _in(py - ky + 1, px - kx + 1):
                    want_y[b0, :, py - ky + 1, px - kx + 1] = w[:, ch, ky, kx]
                if _in(py + ky - 1, px + kx - 1):
                    want_dx[b0, :, py + ky - 1, px + kx - 1] = w[ch, :, ky, kx]
        assert torch.equal(conv(imp_dev, w_dev, 0).cpu(), want_y), (py, px)
        assert torch.equal(conv(imp_dev, w_dev, 1).cpu(), want_dx), (py, px)


# ---- 2. random cases --------------------------------------------------------------------------------------------------
def _three_passes_f(x, w, g, dtype, device):
    """(y, dx, dW) of the stock operator in `dtype` on `device`, as float64 host tensors."""
    x = x.to(device=device, dtype=dtype).requires_grad_(True)
    w = w.to(device=device, dtype=dtype).requires_grad_(True)
    y = F.conv2d(x, w, padding=1)
    dx, dw = torch.autograd.grad(y, (x, w), g.to(device=device, dtype=dtype))
    return [t.detach().double().cpu() for t in (y, dx, dw)]


def check_three_passes(x, w, g, what):
    """The three kernels on (x, w, g) [host fp32 tensors] against float64 under the bound of the module docstring.
    Returns the kernel-error / e32 ratios (y, dx, dW)."""
    want = _three_passes_f(x, w, g, torch.float64, "cpu")
    host = _three_passes_f(x, w, g, torch.float32, "cpu")
    stock = _three_passes_f(x, w, g, torch.float32, DEV)   # (F.conv2d itself: the routing flag does not reach it)
    xd, wd, gd = x.to(DEV), w.to(DEV), g.to(DEV)
    got = [conv(xd, wd, 0), conv(gd, wd, 1), wgrad(xd, gd)]
    ratios = []
    for name, out, f64, a, b in zip(("y", "dx", "dW"), got, want, host, stock):
        e32 = max(float((a - f64).abs().max()), float((b - f64).abs().max()))
        err = float((out.double().cpu() - f64).abs().max())
        bound = ref.tolerance(e32, f64)
        ratios.append(err / e32 if e32 > 0 else 0.0)
        print(f"{what} {name}: err {err:.3e}  e32 {e32:.3e}  ratio {ratios[-1]:.2f}  bound {bound:.3e}  max|f64| {float(f64.abs().max()):.3e}")
        assert torch.isfinite(out).all() and err <= bound, (what, name, err, e32, bound)
    return ratios


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("batch", [1, 3, 9])
def test_random_against_float64(gpu_required, batch, seed):
    """x = relu(randn), W = randn / 12, g = randn.  Measured kernel-to-e32 ratios on an MI355X over these twelve cases
    (the bound is 4): forward 1.00 in every case, data gradient 0.89 - 1.43, weight gradient 0.20 - 0.38.  Every run of
    this test prints them."""
    gen = torch.Generator().manual_seed(1000 * batch + seed)
    x = torch.relu(torch.randn(batch, 16, D, D, generator=gen))
    w = torch.randn(16, 16, 3, 3, generator=gen) / 12
    g = torch.randn(batch, 16, D, D, generator=gen)
    check_three_passes(x, w, g, f"B={batch} seed={seed}")


# ---- 3. determinism and batch invariance ------------------------------------------------------------------------------
def test_batch_invariance_and_repeatability(gpu_required):
    gen = torch.Generator().manual_seed(77)
    x9 = torch.randn(9, 16, D, D, generator=gen).to(DEV)
    g9 = torch.randn(9, 16, D, D, generator=gen).to(DEV)
    w = (torch.randn(16, 16, 3, 3, generator=gen) / 12).to(DEV)
    for transposed in (0, 1):
        full = conv(x9, w, transposed)
        for k in (0, 4, 8):
            alone = conv(x9[k:k + 1], w, transposed)
            three = conv(x9[[(k + 1) % 9, (k + 5) % 9, k]], w, transposed)
            assert torch.equal(alone[0], full[k]) and torch.equal(three[2], full[k]), (transposed, k)
    first = wgrad(x9, g9)
    for _ in range(2):
        assert torch.equal(wgrad(x9, g9), first)
    assert torch.equal(wgrad(x9[:3].clone(), g9[:3].clone()), wgrad(x9[:3], g9[:3]))


def test_function_takes_strided_and_offset_inputs(gpu_required):
    """Channels-last, a strided view and a view 4 bytes off a 16-byte boundary give the bits of the contiguous tensor."""
    fn = _fn()
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(2, 16, D, D, generator=gen).to(DEV)
    w = (torch.randn(16, 16, 3, 3, generator=gen) / 12).to(DEV)
    g = torch.randn(2, 16, D, D, generator=gen).to(DEV)

    def run(xi, gi):
        xi = xi.detach().requires_grad_(True)
        wi = w.detach().clone().requires_grad_(True)
        y = fn.apply(xi, wi)
        y.backward(gi)
        return y.detach(), xi.grad, wi.grad

    want = run(x, g)
    off = torch.empty(x.numel() + 1, device=DEV)[1:].view_as(x).copy_(x)
    assert off.data_ptr() % 16 == 4
    wide = torch.zeros(2, 16, D, 2 * D, device=DEV)
    wide[..., ::2] = x
    for xi, gi in ((x.contiguous(memory_format=torch.channels_last), g.contiguous(memory_format=torch.channels_last)),
                   (off, g), (wide[..., ::2], g)):
        for a, b in zip(run(xi, gi), want):
            assert torch.equal(a, b)
    # only what needs_input_grad asks for is computed
    before = (fn.n_forward, fn.n_backward)
    xi = x.detach().requires_grad_(True)
    fn.apply(xi, w).backward(g)
    assert torch.equal(xi.grad, want[1]) and (fn.n_forward, fn.n_backward) == (before[0] + 1, before[1] + 1)
    with pytest.raises(ValueError):
        fn.apply(x[:, :, :32, :32], w)


# ---- 4 / 5. a real network --------------------------------------------------------------------------------------------
def _net(seed):
    from flingbot_amd import nets

    torch.manual_seed(seed)
    net = nets.SpatialValueNet(rgb_only=True, device=DEV).to(DEV)
    return ref.randomise_bn(net, seed)


def _loss(net, obs, mask, label):
    return F.mse_loss(torch.masked_select(net(obs).squeeze(1), mask), label)


def _batch(batch, seed):
    rng = np.random.default_rng(seed)
    obs = ref.make_obs(batch, seed, channels=3)
    mask = torch.zeros(batch, D, D, dtype=torch.bool)
    for k in range(batch):
        mask[k, int(rng.integers(8, 56)), int(rng.integers(8, 56))] = True
    label = torch.from_numpy(rng.uniform(-0.1, 0.2, batch).astype(np.float32))
    return obs, mask, label


def test_per_layer_replay_on_a_real_network(gpu_required):
    """Inputs and output gradients of the 16 routed convolutions, recorded from a stock train-mode step, through the three
    kernels: every layer meets the bound of the random cases."""
    from flingbot_amd import nets

    net = _net(11).train()
    obs, mask, label = (t.to(DEV) for t in _batch(9, 11))
    convs = [c for blk in list(net.net)[1:-1] for c in (blk.conv1, blk.conv2)]
    assert len(convs) == 16
    seen = {}
    hooks = []
    for k, c in enumerate(convs):
        def record(module, inputs, output, k=k):
            seen[("x", k)] = inputs[0].detach().clone()
            output.register_hook(lambda grad, k=k: seen.__setitem__(("g", k), grad.detach().clone()))
        hooks.append(c.register_forward_hook(record))
    nets._TRAIN_CONV_HIP = False
    try:
        _loss(net, obs, mask, label).backward()
    finally:
        nets._TRAIN_CONV_HIP = True
        for h in hooks:
            h.remove()
    assert len(seen) == 32
    for k, c in enumerate(convs):
        x, g = seen[("x", k)].cpu(), seen[("g", k)].cpu()
        assert tuple(x.shape) == tuple(g.shape) == (9, 16, D, D) and float(g.abs().max()) > 0
        check_three_passes(x, c.weight.detach().cpu(), g, f"layer {k:2d}")


def test_whole_network_forward_and_wiring(gpu_required):
    from flingbot_amd import nets

    net = _net(21)
    obs, mask, label = _batch(9, 21)
    f64 = copy.deepcopy(net).cpu().double().train()
    with torch.no_grad():
        want = f64(obs.double())
    host = copy.deepcopy(net).cpu().train()
    with torch.no_grad():
        e_host = float((host(obs).double() - want).abs().max())
    stock = copy.deepcopy(net).train()
    nets._TRAIN_CONV_HIP = False
    try:
        out_stock = stock(obs.to(DEV))
        F.mse_loss(torch.masked_select(out_stock.squeeze(1), mask.to(DEV)), label.to(DEV)).backward()
    finally:
        nets._TRAIN_CONV_HIP = True
    e32 = max(e_host, float((out_stock.detach().double().cpu() - want).abs().max()))

    fn = nets.Conv16Function
    before = (fn.n_forward, fn.n_backward)
    running = {k: v.clone() for k, v in net.state_dict().items() if "running_" in k}
    net.train()
    out = net(obs.to(DEV))
    assert (fn.n_forward - before[0], fn.n_backward - before[1]) == (16, 0)
    err = float((out.detach().double().cpu() - want).abs().max())
    bound = ref.tolerance(e32, want)
    print(f"whole network: err {err:.3e}  e32 {e32:.3e}  ratio {err / e32:.2f}  bound {bound:.3e}")
    assert err <= bound
    F.mse_loss(torch.masked_select(out.squeeze(1), mask.to(DEV)), label.to(DEV)).backward()
    assert (fn.n_forward - before[0], fn.n_backward - before[1]) == (16, 16)
    with_grad = 0
    for (name, p), (_, q) in zip(net.named_parameters(), stock.named_parameters()):
        if q.grad is None:
            assert p.grad is None, name
            continue
        with_grad += 1
        assert p.grad is not None and p.grad.shape == q.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), name
    assert with_grad == 2 + 16 + 2 * 17          # 18 convolutions, 17 BatchNorms (weight and bias)
    moved = [k for k, v in running.items() if not torch.equal(v, net.state_dict()[k])]
    assert len(moved) == len(running) == 34


# ---- 6. learning ------------------------------------------------------------------------------------------------------
LEARN_UPDATES = 350   # chosen on the CPU with the stock operators: there update 350 ends at 0.007 x the first loss (last ten: <= 0.07 x)


def learning_set(seed=0, n=16):
    """16 synthetic samples: images in the style of test_replay_gpu._observations, one mask pixel each, labels in
    [-0.1, 0.2].  No colour jitter: the set is to be memorised."""
    from flingbot_amd import replay

    rng = np.random.default_rng(seed)
    obs = rng.random((n, 4, D, D), dtype=np.float32)
    obs[:, :3] = obs[:, :3] * np.float32(1.1) - np.float32(0.05)
    obs[:, 3] = np.float32(1.9) + np.float32(0.1) * obs[:, 3]
    obs[0, :3] = np.float32(0.18)
    obs[1, :3] = np.float32(0.4) + (rng.random((3, D, D), dtype=np.float32) - np.float32(0.5)) * np.float32(0.01)
    obs[2, :3, :8] = 0.0
    obs[2, :3, 8:16] = 1.0
    masks = np.zeros((n, D, D), bool)
    for k in range(n):
        masks[k, int(rng.integers(8, 56)), int(rng.integers(8, 56))] = True
    labels = rng.uniform(-0.1, 0.2, n).astype(np.float32)
    return replay.ExperienceSet.from_arrays(obs, masks, labels, obs_color_jitter=False)


def test_optimize_learns_a_fixed_set(gpu_required):
    from flingbot_amd import nets, train

    torch.manual_seed(0)
    net = nets.SpatialValueNet(rgb_only=True, device=DEV).to(DEV)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, weight_decay=1e-6)
    data = learning_set().to_device(DEV)
    before = nets.Conv16Function.n_backward
    net.train()
    losses = train.optimize("fling", net, opt, data, LEARN_UPDATES, 8, np.random.default_rng(0))
    net.eval()
    print(f"loss {losses[0]:.4e} -> {losses[-1]:.4e} in {len(losses)} updates")
    assert len(losses) == LEARN_UPDATES and all(np.isfinite(losses)) and int(net.steps) == LEARN_UPDATES
    assert losses[-1] < 0.5 * losses[0]
    assert nets.Conv16Function.n_backward - before == 16 * LEARN_UPDATES


# ---- 7. the eval path ---------------------------------------------------------------------------------------------------
def test_eval_path_after_training_is_the_folded_state_dict(gpu_required):
    from flingbot_amd import nets, train

    torch.manual_seed(2)
    net = nets.SpatialValueNet(rgb_only=True, device=DEV).to(DEV)
    net.fold_batchnorm()
    obs = ref.make_obs(5, 9).to(DEV)
    first = net(obs).clone()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    net.train()
    assert len(train.optimize("fling", net, opt, learning_set().to_device(DEV), 3, 8, np.random.default_rng(1))) == 3
    net.eval()
    with torch.no_grad():
        out = net(obs)
    assert net._hip is not None and not torch.equal(out, first)
    fresh = nets.SpatialValueNet(rgb_only=True, device=DEV).to(DEV)
    fresh.load_state_dict(net.state_dict())
    fresh.fold_batchnorm()
    with torch.no_grad():
        assert torch.equal(fresh(obs), out)


# ---- 8. end to end --------------------------------------------------------------------------------------------------------
def test_train_run_end_to_end(gpu_required, tmp_path):
    """Three generated tasks, two actions each: two rounds leave two replay files, a checkpoint that loads, updates and
    decayed probabilities; a second call resumes at round 2; a second run from scratch collects identical files."""
    import random

    from flingbot_amd import nets, sim as fsim, tasks as ftasks, train
    from flingbot_amd.env import BatchedFlingEnv

    random.seed(1); np.random.seed(1); torch.manual_seed(1)
    n = 3
    gen = fsim.FlingSim(n_envs=n, solver=0)
    tasks = ftasks.generate_tasks(gen, [ftasks.draw_task_parameters(min_cloth_size=24, strict_min_edge_length=24, max_cloth_size=32) for _ in range(n)])
    gen.close()

    def fresh(env):
        torch.manual_seed(7)
        policy = nets.MaximumValuePolicy(action_primitives=["fling"], num_rotations=12, scale_factors=list(env.scale_factors),
                                         obs_dim=64, pix_grasp_dist=8, pix_drag_dist=8, pix_place_dist=5, rgb_only=True,
                                         depth_only=False, action_expl_prob=0.5, action_expl_decay=0.9, value_expl_prob=0.5,
                                         value_expl_decay=0.9, device=DEV)
        return policy, train.make_optimizer(policy)

    def files(log_dir):
        out = []
        for path in train.replay_files(log_dir):
            z = np.load(path, allow_pickle=False)
            out.append({k: z[k] for k in z.files})
        return out

    logs = [str(tmp_path / "a"), str(tmp_path / "b")]
    ctx = fsim.FlingSim(n_envs=n, solver=0)
    try:
        env = BatchedFlingEnv(ctx, image_dim=128, episode_length=2, record_experience=True)
        policy, opt = fresh(env)
        out = train.run(policy, opt, env, tasks, logs[0], rounds=2, tasks_per_round=n, seed=3, batch_size=2, warmup=0)
        assert out["first_round"] == 0 and [r["round"] for r in out["rounds"]] == [0, 1]
        assert [os.path.basename(p) for p in train.replay_files(logs[0])] == ["replay_00000.npz", "replay_00001.npz"]
        assert int(policy.steps()) > 0 and out["rounds"][-1]["updates"] > 0 and not policy.training
        assert float(policy.action_expl_prob) < 0.5 and float(policy.value_expl_prob) < 0.5
        assert os.path.exists(os.path.join(logs[0], "train_log.jsonl"))
        again, again_opt = fresh(env)
        train.load_checkpoint(os.path.join(logs[0], "latest_ckpt.pth"), again, again_opt)
        for (k, a), (_, b) in zip(policy.state_dict().items(), again.state_dict().items()):
            assert torch.equal(a, b), k
        two = files(logs[0])

        resumed, resumed_opt = fresh(env)          # a new process would start like this: the checkpoint comes from log_dir
        out = train.run(resumed, resumed_opt, env, tasks, logs[0], rounds=1, tasks_per_round=n, seed=3, batch_size=2, warmup=0)
        assert out["first_round"] == 2 and len(train.replay_files(logs[0])) == 3
        assert int(resumed.steps()) > int(policy.steps()) and float(resumed.action_expl_prob) < float(policy.action_expl_prob)

        policy, opt = fresh(env)
        train.run(policy, opt, env, tasks, logs[1], rounds=2, tasks_per_round=n, seed=3, batch_size=2, warmup=0)
        other = files(logs[1])
    finally:
        ctx.close()
    assert len(two) == len(other) == 2
    for a, b in zip(two, other):
        assert set(a) == set(b) and any(k.endswith("/observations") for k in a)
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


# ---- sim.stream_call / sim.work_buffer: what every stateless entry point is called through ----------------------------------
def _b1():
    x = torch.zeros(1, 16, D, D, device=DEV)
    return x, torch.zeros(16, 16, 3, 3, device=DEV), torch.empty_like(x)


def test_stream_call_raises_the_librarys_refusal(gpu_required):
    """dim = 32 is refused before any launch: RuntimeError("<entry point>: " + exactly what fs_last_error then holds)."""
    from flingbot_amd import sim
    x, w, y = _b1()
    with pytest.raises(RuntimeError) as err:
        sim.stream_call("fs_conv16_forward", DEV, x, w, 0, 1, 32, y)
    last = sim.load_library().fs_last_error().decode()
    assert last.startswith("fs_conv16_forward: ") and str(err.value) == "fs_conv16_forward: " + last


def test_stream_call_passes_none_as_a_null_pointer(gpu_required):
    """Every other argument is servable, so the null pointer is what the library refuses (before any launch)."""
    from flingbot_amd import sim
    x, w, y = _b1()
    for args in ((None, w, 0, 1, D, y), (x, None, 0, 1, D, y), (x, w, 0, 1, D, None)):
        with pytest.raises(RuntimeError) as err:
            sim.stream_call("fs_conv16_forward", DEV, *args)
        last = sim.load_library().fs_last_error().decode()
        assert last.startswith("fs_conv16_forward: bad arguments") and str(err.value) == "fs_conv16_forward: " + last


def test_work_buffer_is_the_entry_points_scratch(gpu_required):
    from flingbot_amd import sim
    work = sim.work_buffer("fs_conv16_work_bytes", DEV, 1, 64)
    want = int(sim.load_library().fs_conv16_work_bytes(1, 64))
    assert want > 0 and work.dtype == torch.uint8 and work.is_cuda and work.device == torch.device(DEV)
    assert tuple(work.shape) == (want,) and work.data_ptr() % 16 == 0
    assert sim.work_buffer("fs_conv16_work_bytes", DEV, 1, 64).data_ptr() != work.data_ptr()   # fresh per call


@pytest.mark.parametrize("device", [DEV, "cuda", 0])
def test_stream_call_refuses_a_tensor_on_another_device(gpu_required, device):
    """A host tensor never reaches the entry point: ValueError, and fs_last_error still holds what another entry point left.
    (dim = 32, so that even a call that did get through would be refused before a launch.)"""
    from flingbot_amd import sim
    x, w, y = _b1()
    with pytest.raises(RuntimeError):
        sim.stream_call("fs_conv16_wgrad", device, x, x, 1, 32, w, y)
    before = sim.load_library().fs_last_error().decode()
    assert before.startswith("fs_conv16_wgrad: ")
    for args in ((x.cpu(), w, 0, 1, 32, y), (x, w, 0, 1, 32, y.cpu())):
        with pytest.raises(ValueError, match="fs_conv16_forward"):
            sim.stream_call("fs_conv16_forward", device, *args)
        assert sim.load_library().fs_last_error().decode() == before
