"""fs_map_list_loss (csrc/fs_maplist.hip) on the GPU against the float64 restatement of maplist_reference.py in both
normalisations, its exact properties, trainops.MapListFunction's backward, a descent on the predictions themselves, and
optimize_maps(map_loss=True, list_weight=0.5) end to end.

The bounds are maplist_reference's: the float32 outputs (d_dpred, d_table) within bound32(n, A) = (n + 16) 2^-24 A, the double
statistics within bound64(n, A) = (n + 16) 2^-53 A, with the restatement's n addends of absolute sum A (and the subnormal floor
its docstring explains); G_l, L_l, H and the arg-max indices exactly.  Every case prints its largest |got - ref| / bound; the
largest observed on an MI355X over all cases of this file: 0.044 (a dpred component of the mixed batch with T_y != T_p under the
image mean); the statistics and table entries stay below 0.03."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import maplist_reference as lref
from test_maploss_cpu import big_maps
from test_maplist_cpu import CASES, LIST_KEYS, MAP_KEYS, MIXED, T, W, compare, reference, values

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = (False, True)
_ratios = {}


def _device(pred, label, offsets):
    return (torch.from_numpy(np.ascontiguousarray(pred, np.float32)).to(DEV), torch.from_numpy(np.ascontiguousarray(label, np.float32)).to(DEV),
            torch.from_numpy(np.ascontiguousarray(offsets, np.int32)).to(DEV))


def _launch(pred, label, offsets, per_image, w=W, tp=T, ty=None, scale=1.0):
    from flingbot_amd import trainops

    p, y, off = _device(pred, label, offsets)
    dpred, stats, table = trainops.MapListFunction._launch(p, y, off, w, tp, tp if ty is None else ty, per_image, scale)
    torch.cuda.synchronize()
    return dpred.cpu().numpy(), stats.cpu().numpy(), table.cpu().numpy()


def _bits(*arrays):
    return [np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64).tolist() for a in arrays]


def _compare(name, got, ref):
    dpred, stats, table = got
    assert dpred.dtype == np.float32 and stats.dtype == np.float64 and table.dtype == np.float32
    return compare(name, ref, dpred, stats, table, lref.bound64, lref.bound32, lref.bound32)


@pytest.mark.parametrize("per_image", MODES, ids=["label_mean", "image_mean"])
@pytest.mark.parametrize("name", list(CASES))
def test_kernels_against_the_float64_restatement(gpu_required, name, per_image):
    lengths, kind, ty = CASES[name]
    pred, label, offsets = values(lengths, kind)
    ref = reference(name, per_image)
    got = _launch(pred, label, offsets, per_image, ty=ty)
    assert all(np.isfinite(a).all() for a in got), name                            # the spread of 10^4 T included
    _ratios[(name, per_image)] = _compare(f"{name} per_image={per_image}", got, ref)
    assert ref["listed"] == sum(k >= 2 for k in lengths) > 0 and ref["list"][0] > 0.0   # no case passes vacuously
    for b, k in enumerate(lengths):
        if k < 2:                                                                 # not listed: +0.0 gradients, the fixed row
            assert not got[0][int(offsets[b]):int(offsets[b + 1])].view(np.uint32).any() and got[2][b].tolist() == [0.0, 0.0, -1.0, -1.0]
    again = _launch(pred, label, offsets, per_image, ty=ty)                        # equal inputs: equal bits
    assert _bits(*got) == _bits(*again)
    print(f"largest err / bound so far over {len(_ratios)} cases: {max(_ratios.values()):.3f}")


@pytest.mark.parametrize("per_image", MODES, ids=["label_mean", "image_mean"])
def test_an_image_does_not_depend_on_its_place_or_on_the_others(gpu_required, per_image):
    """Permuting the images permutes the table rows bit for bit and, G_l and L_l being what they were, every image's dpred bits
    -- coef_b times its g_i; other values in another image at fixed counts change no bit outside it; one NaN makes its own image
    and the totals non-finite and changes no bit outside it either."""
    pred, label, offsets = values(MIXED, "replay")
    dpred, stats, table = _launch(pred, label, offsets, per_image)
    order = [10, 3, 0, 7, 9, 1, 4, 2, 8, 6, 5]
    lengths = np.diff(offsets)
    gather = np.concatenate([np.arange(offsets[b], offsets[b + 1]) for b in order])
    dpred2, stats2, table2 = _launch(pred[gather], label[gather], lref.offsets_of(lengths[order]), per_image)
    assert _bits(table2) == _bits(table[order]) and _bits(dpred2) == _bits(dpred[gather])
    assert stats2[2:5].tolist() == stats[2:5].tolist()
    _compare("moved", (dpred2[np.argsort(gather)], stats2, table2[np.argsort(order)]), reference("mixed", per_image))
    # other values in image 8 (256 labels), then a NaN label in it, then a NaN prediction
    lo, hi = int(offsets[8]), int(offsets[9])
    outside = np.ones(len(pred), bool)
    outside[lo:hi] = False
    rows = np.arange(len(MIXED)) != 8
    other_pred, other_label = pred.copy(), label.copy()
    other_pred[lo:hi], other_label[lo:hi] = pred[lo:hi][::-1] * np.float32(1.5), label[lo:hi][::-1]
    dpred3, stats3, table3 = _launch(other_pred, other_label, offsets, per_image)
    assert _bits(dpred3[outside]) == _bits(dpred[outside]) and _bits(table3[rows]) == _bits(table[rows])
    assert _bits(dpred3[lo:hi]) != _bits(dpred[lo:hi]) and np.isfinite(stats3).all()
    for which in ("label", "pred"):
        bad_pred, bad_label = pred.copy(), label.copy()
        (bad_label if which == "label" else bad_pred)[lo + 100] = np.nan
        dpred4, stats4, table4 = _launch(bad_pred, bad_label, offsets, per_image)
        assert _bits(dpred4[outside]) == _bits(dpred[outside]) and _bits(table4[rows]) == _bits(table[rows]), which
        assert not np.isfinite(dpred4[lo:hi]).any() and not np.isfinite(table4[8, 0]), which
        assert not np.isfinite(stats4[[0, 1]]).any() and stats4[2:4].tolist() == stats[2:4].tolist(), which
        assert 0 <= table4[8, 2] < 256 and 0 <= table4[8, 3] < 256 and table4[8, 2 if which == "pred" else 3] != 100   # NaN never wins
    assert torch.zeros(1, device=DEV).item() == 0.0


@pytest.mark.parametrize("per_image", MODES, ids=["label_mean", "image_mean"])
def test_degenerate_cases(gpu_required, per_image):
    lengths, kind, ty = CASES["ties"]
    pred, label, offsets = values(lengths, kind)
    one, stats, table = _launch(pred, label, offsets, per_image)
    assert one.any() and stats[1] > 0.0
    for k in (2, -3):                                                              # grad_scale 2^k scales dpred exactly
        scaled, stats_k, table_k = _launch(pred, label, offsets, per_image, scale=2.0 ** k)
        assert np.array_equal(scaled, np.float32(2.0 ** k) * one) and _bits(stats_k, table_k) == _bits(stats, table)
    zero, stats_0, table_0 = _launch(pred, label, offsets, per_image, w=0.0)       # weight 0: no gradient, the statistics stay
    assert not zero.view(np.uint32).any() and stats_0[0] == 0.0 and _bits(stats_0[1:], table_0) == _bits(stats[1:], table)
    # ties at the maximum go to the lowest index, in the kernel as in the restatement
    ref = reference("ties", per_image)
    assert [int(v) for v in table[:, 2]] == [row["chosen"] for row in ref["table"]]
    assert [int(v) for v in table[:, 3]] == [row["best"] for row in ref["table"]]
    # no image is listed: the term is +0.0, every gradient +0.0, every row the fixed one
    lone = lref.offsets_of([1, 0, 1, 1])
    p, y = np.float32([0.3, -0.2, 7.0]), np.float32([0.1, 0.2, 0.0])
    dpred, stats, table = _launch(p, y, lone, per_image)
    assert not dpred.view(np.uint32).any() and not stats.view(np.uint64).any() and table.tolist() == [[0.0, 0.0, -1.0, -1.0]] * 4


def test_a_malformed_table_is_clamped_and_bad_arguments_launch_nothing(gpu_required):
    """Through the C entry directly.  Offsets that are negative, fall, pass the labels and span more than 4096 labels: FS_OK, the
    clamped restatement's numbers (begin = clamp(off[b], 0, L), end = clamp(off[b + 1], begin, L), end = min(end, begin + 4096)),
    and the entries no clamped image owns untouched.  Bad arguments: FS_ERR_ARG, and not one output byte written."""
    from flingbot_amd import sim as fsim, trainops

    L = 6000
    pred, label, _ = values([L], "replay", seed=9)
    bad = np.int32([-7, 1000, 1000, 7000, 6500])
    assert lref.clamp_offsets(bad, L) == [(0, 1000), (1000, 0), (1000, 4096), (6000, 0)]
    with pytest.raises(ValueError):
        trainops.MapListFunction.apply(torch.from_numpy(pred).to(DEV), torch.from_numpy(label).to(DEV), bad.astype(np.int64), W, T, None, False)
    p, y, off = _device(pred, label, bad)
    lib = fsim.load_library()

    def outputs():
        return (torch.full((L,), 7.0, dtype=torch.float32, device=DEV), torch.full((8,), 7.0, dtype=torch.float64, device=DEV),
                torch.full((4, 4), 7.0, dtype=torch.float32, device=DEV))

    for per_image in MODES:
        dpred, stats, table = outputs()
        work = fsim.work_buffer("fs_map_list_work_bytes", torch.device(DEV), 4, L)
        fsim.stream_call("fs_map_list_loss", torch.device(DEV), p, y, off, 4, L, W, T, T, int(per_image), 1.0, dpred, stats, table, work)   # raises unless FS_OK
        torch.cuda.synchronize()
        ref = lref.map_list_f64(pred, label, bad, W, T, None, per_image)
        assert ref["listed"] == 2 and ref["labels"] == 5096
        dpred = dpred.cpu().numpy()
        _compare(f"clamped per_image={per_image}", (dpred, stats.cpu().numpy(), table.cpu().numpy()), ref)
        assert (dpred[5096:] == 7.0).all() and np.isnan(ref["dpred"][0][5096:]).all()
    # bad arguments: the device pointers are good, so a launch would have written
    dpred, stats, table = outputs()
    work = fsim.work_buffer("fs_map_list_work_bytes", torch.device(DEV), 4, L)
    torch.cuda.synchronize()
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    ok = dict(images=4, labels=L, w=W, tp=T, ty=T, per_image=0, s=1.0)
    nan, inf = float("nan"), float("inf")
    for kw in (dict(images=0), dict(labels=0), dict(per_image=2), dict(w=-1.0), dict(w=nan), dict(tp=0.0), dict(tp=inf), dict(ty=-0.1),
               dict(ty=5e-324), dict(s=inf)):
        a = {**ok, **kw}
        assert lib.fs_map_list_loss(ptr(p), ptr(y), ptr(off), a["images"], a["labels"], a["w"], a["tp"], a["ty"], a["per_image"], a["s"],
                                    ptr(dpred), ptr(stats), ptr(table), ptr(work), None) == -1, kw        # FS_ERR_ARG
        assert b"fs_map_list_loss" in lib.fs_last_error(), kw
    torch.cuda.synchronize()
    assert (dpred == 7.0).all().item() and (stats == 7.0).all().item() and (table == 7.0).all().item()


@pytest.mark.parametrize("per_image", MODES, ids=["label_mean", "image_mean"])
def test_autograd(gpu_required, per_image):
    """term is float32(stats[0]); backward with a non-unit grad_output is grad_output * dpred; stats and table carry no grad; the
    torch statement on the same device gives the same numbers to float32."""
    from flingbot_amd import trainops

    pred, label, offsets = values([40, 1, 17, 0, 64], seed=2)
    dpred, stats, table = _launch(pred, label, offsets, per_image, ty=0.07)
    p = torch.from_numpy(pred).to(DEV).requires_grad_(True)
    before = trainops.MapListFunction.n_forward
    term, got_stats, got_table = trainops.MapListFunction.apply(p, torch.from_numpy(label).to(DEV), offsets, W, T, 0.07, per_image)
    assert trainops.MapListFunction.n_forward == before + 1
    assert term.requires_grad and not got_stats.requires_grad and not got_table.requires_grad
    assert term.dtype == torch.float32 and got_stats.dtype == torch.float64 and got_table.dtype == torch.float32
    assert term.item() == float(np.float32(stats[0])) and _bits(got_stats.cpu().numpy(), got_table.cpu().numpy()) == _bits(stats, table)
    (term * 3.5).backward()
    assert np.array_equal(p.grad.cpu().numpy(), np.float32(3.5) * dpred)
    r = torch.from_numpy(pred).to(DEV).requires_grad_(True)
    t_term, t_stats, t_table = trainops.map_list_torch(r, torch.from_numpy(label).to(DEV), offsets, W, T, 0.07, per_image)
    t_term.backward()
    t_stats = t_stats.cpu().numpy()
    assert t_stats[2:5].tolist() == stats[2:5].tolist() and np.array_equal(t_table.cpu().numpy()[:, 2:], table[:, 2:])
    assert np.allclose(t_stats[[0, 1, 5, 6]], stats[[0, 1, 5, 6]], rtol=1e-5, atol=0)
    assert np.allclose(r.grad.cpu().numpy(), dpred, rtol=1e-4, atol=1e-7) and np.allclose(t_table.cpu().numpy()[:, :2], table[:, :2], rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize("per_image", MODES, ids=["label_mean", "image_mean"])
def test_descent_on_the_predictions(gpu_required, per_image):
    """weight * list is convex in the predictions, and its gradient is Lipschitz with a constant of at most weight / (2 T_p^2): the
    Hessian of D_b is (diag(s) - s s^T) / T_p^2, of norm at most 1 / (2 T_p^2), and coef_b <= 1.  A step of T_p^2 / weight along
    the kernel's dpred therefore cannot raise the term.  What is allowed on top: the bound of `list` itself (it is read from the
    kernel before and after, so twice), and what rounding the stepped predictions to float32 can add, sum_i |dlist / dp_i| 2^-24
    |p_i|.  30 steps on 8 images of 2 .. 300 labels: no rise beyond that, and a lower end."""
    lengths = [2, 3, 17, 64, 65, 129, 256, 300]
    pred, label, offsets = values(lengths, "replay", seed=12)
    step = T * T / W
    seen = []
    for _ in range(31):
        dpred, stats, _ = _launch(pred, label, offsets, per_image)
        ref = lref.map_list_f64(pred, label, offsets, W, T, None, per_image)
        tol = float(lref.bound64(ref["list"][1], ref["list"][2]))
        assert abs(stats[1] - ref["list"][0]) <= tol
        seen.append((float(stats[1]), tol))
        stepped = (pred.astype(np.float64) - step * dpred.astype(np.float64)).astype(np.float32)
        rounding = float((np.abs(dpred.astype(np.float64)) / W * 2.0 ** -24 * np.abs(stepped)).sum())
        pred = stepped
        seen[-1] += (rounding,)
    for (before, tol_a, rounding), (after, tol_b, _) in zip(seen, seen[1:]):
        assert after - before <= tol_a + tol_b + rounding, (before, after)
    print("list:", " ".join(f"{v[0]:.6g}" for v in seen))
    assert seen[-1][0] < seen[0][0]


# ---- end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hip_step", [True, False])
def test_optimize_maps_end_to_end(gpu_required, hip_step):
    """The 5 images with 5200 labels of test_maploss_gpu's end-to-end test; two updates with map_loss, rank_weight 0.5 and
    list_weight 0.5: the rows carry the list fields, one list launch per update, the term reached the weights; with list_weight = 0
    passed explicitly the state after the updates has the bits of a call that does not pass it, and no list launch happens."""
    from flingbot_amd import nets, train, trainops

    data = big_maps().to_device(DEV)
    torch.manual_seed(21)
    first = nets.SpatialValueNet(rgb_only=True, device=DEV).to(DEV)
    runs = {}
    for name, extra in (("absent", dict()), ("zero", dict(list_weight=0.0, list_temperature=0.3, label_temperature=0.7)),
                        ("listed", dict(list_weight=0.5)), ("again", dict(list_weight=0.5))):
        net = copy.deepcopy(first)
        opt = train.HipAdam(net.parameters(), lr=1e-3, weight_decay=1e-6) if hip_step else torch.optim.Adam(net.parameters(), lr=1e-3, weight_decay=1e-6)
        rows, launches, map_launches = [], trainops.MapListFunction.n_forward, trainops.MapLossFunction.n_forward
        net.train()
        with train.deterministic_library_convs(not hip_step):
            losses = train.optimize_maps("fling", net, opt, data, 2, 5, np.random.default_rng(3), hip_step=hip_step, rank_weight=0.5,
                                         map_loss=True, stats=rows, **extra)
        net.eval()
        assert trainops.MapListFunction.n_forward == launches + (2 if extra.get("list_weight") else 0), name
        assert trainops.MapLossFunction.n_forward == map_launches + 2 and int(net.steps) == 2
        runs[name] = (losses, rows, net.state_dict())
    for a, b in (("absent", "zero"), ("listed", "again")):
        assert runs[a][0] == runs[b][0] and runs[a][1] == runs[b][1], (a, b)
        for k, v in runs[a][2].items():
            assert torch.equal(v, runs[b][2][k]), (a, b, k)
    assert all(set(row) == MAP_KEYS for row in runs["absent"][1]) and all(set(row) == MAP_KEYS | LIST_KEYS for row in runs["listed"][1])
    assert any(not torch.equal(v, runs["absent"][2][k]) for k, v in runs["listed"][2].items() if k.endswith("weight"))
    losses, rows, _ = runs["listed"]
    plain = runs["absent"][1]
    assert rows[0]["mse"] == plain[0]["mse"] and rows[0]["rank"] == plain[0]["rank"] and rows[0]["pairs"] == plain[0]["pairs"]   # the same first batch
    for loss, row in zip(losses, rows):
        assert np.isfinite(loss) and row["loss"] == loss and row["listed_images"] == 5 and 0 <= row["top1_hits"] <= 5
        own = float(np.float32(row["mse"] + 0.5 * row["rank"]))
        assert loss == float(np.float32(own) + np.float32(0.5 * row["list"])) and row["list"] > 0.0
        assert 0.0 < row["chosen_mass"] <= row["best_mass"] <= 1.0
