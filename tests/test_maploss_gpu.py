"""fs_map_loss (csrc/fs_maploss.hip) on the GPU against the float64 restatement of maploss_reference.py in both normalisations,
its exact properties, trainops.MapLossFunction's backward, and optimize_maps(map_loss=True) end to end.

The bound for every output is grouploss_reference.bound: |got - ref| <= (n + 16) 2^-24 A with the restatement's n addends of
absolute sum A.  Largest |got - ref| / bound observed on an MI355X over all cases of this file: 0.174 (a dpred component of the
image mean in the layout of 300 small images and one of 300 labels); the statistics and table entries stay below 0.125."""
import copy

import numpy as np
import pytest
import torch

import grouploss_reference as gref
import maploss_reference as mref
from test_maploss_cpu import big_maps

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, TAU = 0.5, 0.1

MANY = [int(k) for k in np.random.default_rng(300).integers(1, 6, 300)] + [300]   # more images than a workgroup has threads
LAYOUTS = {**{str(k): [k] for k in (1, 2, 5, 64, 65, 255, 256, 257, 1024, 4096)},  # the wave, chunk and cap boundaries
           "40x144": [144] * 40,                                                   # 5760 labels: more than fs_group_loss takes
           "empties": [0, 3, 0, 0, 7, 0],
           "many": MANY,
           "mixed": [4096, 1, 257, 0, 64],
           "2x4096": [4096, 4096]}
MODES = (False, True)
_terms, _ratios = {}, {}


def _inputs(name):
    offsets = mref.offsets_of(LAYOUTS[name])
    pred, label = gref.batch(int(offsets[-1]), seed=len(name) + int(offsets[-1]))
    return pred, label, offsets


def _reference(name, per_image, weight=W, scale=1.0):
    """The restatement of a layout; its pair pass is computed once and shared."""
    if name not in _terms:
        _terms[name] = mref.image_terms(*_inputs(name), TAU, 0.0)
    return mref.normalise(_terms[name], weight, per_image, scale)


def _launch(pred, label, offsets, per_image, w=W, tau=TAU, gap=0.0, scale=1.0):
    from flingbot_amd import trainops

    p, y = torch.from_numpy(np.ascontiguousarray(pred, np.float32)).to(DEV), torch.from_numpy(np.ascontiguousarray(label, np.float32)).to(DEV)
    off = torch.from_numpy(np.ascontiguousarray(offsets, np.int32)).to(DEV)
    dpred, stats, table = trainops.MapLossFunction._launch(p, y, off, w, tau, gap, per_image, scale)
    torch.cuda.synchronize()
    return dpred.cpu().numpy(), stats.cpu().numpy(), table.cpu().numpy()


def _bits(*arrays):
    return [a.view(np.uint32 if a.dtype == np.float32 else np.uint64).tolist() for a in arrays]


def _compare(name, got, ref, factor=1.0):
    """Every output against the restatement within factor * bound; the counts exactly.  Returns the largest |got - ref| / bound."""
    dpred, stats, table = got
    assert stats.dtype == np.float64 and table.dtype == np.float32
    assert stats[3:].tolist() == [ref["pairs"], ref["concordant"], ref["filled"], ref["ranked"], 0.0], name
    worst = 0.0
    for k, out in enumerate(("loss", "mse", "rank")):
        value, n, A = ref[out]
        err, tol = abs(float(stats[k]) - value), float(gref.bound(n, A))
        print(f"{name}: {out} {stats[k]:.12g} ref {value:.12g} err {err:.3e} bound {tol:.3e}")
        assert err <= factor * tol, (name, out, err, tol)
        worst = max(worst, err / tol if tol else 0.0)
    for b, row in enumerate(ref["table"]):
        assert table[b, 2] == row["pairs"] and table[b, 3] == row["concordant"], (name, b)
        for k, out in enumerate(("mse", "rank")):
            value, n, A = row[out]
            err, tol = abs(float(table[b, k]) - value), float(gref.bound(n, A))
            assert err <= factor * tol, (name, b, out, err, tol)
            worst = max(worst, err / tol if tol else 0.0)
        if not row["pairs"]:
            assert table[b, 1:2].view(np.uint32)[0] == 0, (name, b)                  # +0.0
        if not row["mse"][1]:
            assert not table[b].view(np.uint32).any(), (name, b)                     # an empty image: a row of +0.0
    value, n, A = ref["dpred"]
    err, tol = np.abs(dpred.astype(np.float64) - value), gref.bound(n, A)
    ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), 0.0)
    print(f"{name}: dpred largest err / bound {ratio.max():.3f} at {int(ratio.argmax())}; table and stats {worst:.3f}")
    assert (err <= factor * tol).all(), (name, "dpred", int(np.argmax(err - tol)), float(err.max()))
    return max(worst, float(ratio.max()))


@pytest.mark.parametrize("per_image", MODES, ids=["label_mean", "image_mean"])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_kernels_against_the_float64_restatement(gpu_required, name, per_image):
    pred, label, offsets = _inputs(name)
    ref = _reference(name, per_image)
    got = _launch(pred, label, offsets, per_image)
    _ratios[(name, per_image)] = _compare(f"{name} per_image={per_image}", got, ref)
    if max(LAYOUTS[name]) > 4:
        assert ref["pairs"] > 0                                                     # no case passes vacuously
    again = _launch(pred, label, offsets, per_image)                                # equal inputs: equal bits
    assert _bits(*got) == _bits(*again)
    print(f"largest err / bound so far over {len(_ratios)} cases: {max(_ratios.values()):.3f}")


@pytest.mark.parametrize("per_image", MODES, ids=["label_mean", "image_mean"])
def test_an_image_does_not_depend_on_its_place(gpu_required, per_image):
    """Permuting the images permutes the table rows bit for bit and leaves every image's P_b, C_b -- and, with the scalars L, P,
    G', G'' unchanged by a permutation, its dpred bits; the totals are sums in another order and hold within the bound."""
    pred, label, offsets = _inputs("mixed")
    dpred, stats, table = _launch(pred, label, offsets, per_image)
    order = [3, 2, 0, 4, 1]
    lengths = np.diff(offsets)
    gather = np.concatenate([np.arange(offsets[b], offsets[b + 1]) for b in order])
    moved = mref.offsets_of(lengths[order])
    dpred2, stats2, table2 = _launch(pred[gather], label[gather], moved, per_image)
    assert _bits(table2) == _bits(np.ascontiguousarray(table[order]))
    assert _bits(dpred2) == _bits(np.ascontiguousarray(dpred[gather]))
    assert stats2[3:].tolist() == stats[3:].tolist()
    _compare("moved", (dpred2, stats2, table2), _reference_moved(order, gather, per_image))


def _reference_moved(order, gather, per_image):
    """The restatement of 'mixed' with its images in another order: the same terms, re-indexed."""
    _reference("mixed", per_image)
    t = _terms["mixed"]
    lengths = [t["images"][b][1] for b in order]
    begins = mref.offsets_of(lengths)[:-1]
    moved = dict(t, p=t["p"][gather], y=t["y"][gather], up=t["up"][gather], down=t["down"][gather], count=t["count"][gather],
                 images=[(int(begins[k]), int(lengths[k])) for k in range(len(order))],
                 S=t["S"][order], R=t["R"][order], P=t["P"][order], C=t["C"][order])
    return mref.normalise(moved, W, per_image)


@pytest.mark.parametrize("name", ["257", "empties", "28x144"])
def test_against_fs_group_loss_where_both_serve(gpu_required, name):
    """The label mean at L <= 4096: P and C are equal, every value lies within the sum of the two kernels' bounds of the other's,
    and with weight = 0 dpred has fs_group_loss' bits."""
    from flingbot_amd import trainops

    lengths = [144] * 28 if name == "28x144" else LAYOUTS[name]
    offsets = mref.offsets_of(lengths)
    pred, label = gref.batch(int(offsets[-1]), seed=5)
    ref = mref.map_loss_f64(pred, label, offsets, W, TAU, 0.0, False)
    assert ref["pairs"] > 0
    bounds = torch.from_numpy(mref.expanded_bounds(offsets)).to(DEV)
    p, y = torch.from_numpy(pred).to(DEV), torch.from_numpy(label).to(DEV)
    for w in (W, 0.0):
        dpred, stats, _ = _launch(pred, label, offsets, False, w=w)
        old_dpred, old_stats = trainops.GroupLossFunction._launch(p, y, bounds, w, TAU, 0.0)
        old_dpred, old_stats = old_dpred.cpu().numpy(), old_stats.cpu().numpy()
        assert stats[3] == old_stats[3] == ref["pairs"] and stats[4] == old_stats[4] == ref["concordant"]
        for k, out in enumerate(("loss", "mse", "rank")):
            assert abs(stats[k] - float(old_stats[k])) <= 2 * gref.bound(ref[out][1], ref[out][2]), (out, w)
        if w:
            assert (np.abs(dpred.astype(np.float64) - old_dpred) <= 2 * gref.bound(ref["dpred"][1], ref["dpred"][2])).all()
        else:
            assert _bits(dpred) == _bits(old_dpred)


@pytest.mark.parametrize("per_image", MODES, ids=["label_mean", "image_mean"])
@pytest.mark.parametrize("kind", ["singletons", "equal"])
def test_without_pairs_the_ranking_term_is_absent(gpu_required, kind, per_image):
    """P = 0 (images of one label, or equal labels): rank has the bits of +0.0 and dpred those of a launch with weight = 0."""
    lengths = [1] * 7 if kind == "singletons" else [64, 5]
    offsets = mref.offsets_of(lengths)
    pred, label = gref.batch(int(offsets[-1]), seed=8)
    if kind == "equal":
        label[:] = 0.25
    dpred, stats, table = _launch(pred, label, offsets, per_image, w=W)
    plain, plain_stats, plain_table = _launch(pred, label, offsets, per_image, w=0.0)
    assert stats[3] == 0 and stats[6] == 0 and stats[2:3].view(np.uint64)[0] == 0 and stats[0] == stats[1] == plain_stats[1]
    assert _bits(dpred) == _bits(plain) and _bits(table) == _bits(plain_table) and not table[:, 1:].view(np.uint32).any()
    if not per_image:
        assert np.array_equal(dpred, (np.float32(2.0) * (pred - label) / np.float32(len(pred))).astype(np.float32))


@pytest.mark.parametrize("per_image", MODES, ids=["label_mean", "image_mean"])
def test_gradient_scale_is_exact(gpu_required, per_image):
    pred, label, offsets = _inputs("empties")
    one, stats, table = _launch(pred, label, offsets, per_image, scale=1.0)
    half, stats_half, table_half = _launch(pred, label, offsets, per_image, scale=0.5)
    assert stats[3] > 0 and one.any() and np.array_equal(half, np.float32(0.5) * one)
    assert _bits(stats, table) == _bits(stats_half, table_half)


@pytest.mark.parametrize("per_image", MODES, ids=["label_mean", "image_mean"])
def test_edge_values(gpu_required, per_image):
    # one NaN label in image 1: NaN loss, mse and table[1][0]; every other row finite; the NaN in no pair; a clean return
    lengths = [40, 65, 17]
    offsets = mref.offsets_of(lengths)
    pred, label = gref.batch(int(offsets[-1]), seed=11)
    label[40 + 7] = np.nan
    dpred, stats, table = _launch(pred, label, offsets, per_image)
    keep = np.arange(len(pred)) != 47
    assert np.isnan(stats[0]) and np.isnan(stats[1]) and np.isfinite(stats[2]) and np.isnan(table[1, 0])
    assert np.isfinite(table[[0, 2]]).all() and np.isfinite(table[1, 1:]).all()
    without = mref.map_loss_f64(pred[keep], label[keep], mref.offsets_of([40, 64, 17]), W, TAU, 0.0, per_image)
    assert stats[3] == without["pairs"] > 0 and stats[4] == without["concordant"] and table[1, 2] == without["table"][1]["pairs"]
    assert np.isnan(dpred[47]) and np.isfinite(dpred[keep]).all()
    assert torch.zeros(1, device=DEV).item() == 0.0
    # |dp| / tau = 1e4, both signs: finite, within the bound
    for sign in (1.0, -1.0):
        y2, p2 = np.float32([1.0, 0.0, 0.3]), np.float32([sign * 500.0, -sign * 500.0, 0.1])
        ref = mref.map_loss_f64(p2, y2, [0, 2, 3], W, TAU, 0.0, per_image)
        got = _launch(p2, y2, [0, 2, 3], per_image)
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
        _compare(f"saturated {sign:+.0f}", got, ref)
        assert got[1][2] == (0.0 if sign > 0 else 1e4)
    # min_gap drops the close pairs, as on the host
    pred, label, offsets = _inputs("empties")
    _compare("gap", _launch(pred, label, offsets, per_image, gap=0.05), mref.map_loss_f64(pred, label, offsets, W, TAU, 0.05, per_image))


def test_a_malformed_table_is_refused_and_clamped(gpu_required):
    """The Python side refuses each defect (ValueError); the kernels, given them all at once, clamp and return: the clamp of
    fs_ml_image is begin = clamp(off[b], 0, L), end = clamp(off[b + 1], begin, L), end = min(end, begin + 4096), and every index
    of both kernels is formed from (begin, end - begin).  One launch."""
    from flingbot_amd import trainops

    L = 6000
    pred, label = gref.batch(L, seed=2)
    p, y = torch.from_numpy(pred).to(DEV), torch.from_numpy(label).to(DEV)
    for bad in ([0, 3000, 2000, L], [0, -5, L], [0, 3000, L + 100], [0, 5000, L]):   # falling, negative, past labels, an image of 5000
        with pytest.raises(ValueError):
            trainops.MapLossFunction.apply(p, y, np.array(bad), W, TAU, 0.0, False)
    bad = np.int32([-3, 5000, 40, 100000, 60])
    assert mref.clamp_offsets(bad, L) == [(0, 4096), (5000, 0), (40, 4096), (6000, 0)]
    ref = mref.map_loss_f64(pred, label, bad, W, TAU, 0.0, False)
    dpred, stats, table = _launch(pred, label, bad, False)
    assert stats[3] == ref["pairs"] > 0 and stats[4] == ref["concordant"] and stats[5] == 2
    assert [int(v) for v in table[:, 2]] == [row["pairs"] for row in ref["table"]]
    assert torch.zeros(1, device=DEV).item() == 0.0


@pytest.mark.parametrize("per_image", MODES, ids=["label_mean", "image_mean"])
def test_autograd(gpu_required, per_image):
    """loss is float32(stats[0]); backward with a non-unit grad_output is grad_output * dpred; stats and table carry no grad."""
    from flingbot_amd import trainops

    pred, label, offsets = _inputs("empties")
    dpred, stats, table = _launch(pred, label, offsets, per_image)
    p = torch.from_numpy(pred).to(DEV).requires_grad_(True)
    before = trainops.MapLossFunction.n_forward
    loss, got_stats, got_table = trainops.MapLossFunction.apply(p, torch.from_numpy(label).to(DEV), offsets, W, TAU, 0.0, per_image)
    assert trainops.MapLossFunction.n_forward == before + 1
    assert loss.requires_grad and not got_stats.requires_grad and not got_table.requires_grad
    assert loss.dtype == torch.float32 and got_stats.dtype == torch.float64 and got_table.dtype == torch.float32
    assert loss.item() == float(np.float32(stats[0])) and _bits(got_stats.cpu().numpy(), got_table.cpu().numpy()) == _bits(stats, table)
    (loss * 3.5).backward()
    assert np.array_equal(p.grad.cpu().numpy(), np.float32(3.5) * dpred)
    # the torch statement runs on the GPU too (what the kernels are timed against): the same pairs, the same numbers to float32
    r = torch.from_numpy(pred).to(DEV).requires_grad_(True)
    t_loss, t_stats, t_table = trainops.map_loss_torch(r, torch.from_numpy(label).to(DEV), offsets, W, TAU, 0.0, per_image)
    t_loss.backward()
    t_stats = t_stats.cpu().numpy()
    assert t_stats[3:].tolist() == stats[3:].tolist() and np.array_equal(t_table.cpu().numpy()[:, 2:], table[:, 2:])
    assert np.allclose(t_stats[:3], stats[:3], rtol=1e-5, atol=0) and np.allclose(r.grad.cpu().numpy(), dpred, rtol=1e-4, atol=1e-7)


# ---- end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hip_step", [True, False])
def test_optimize_maps_end_to_end(gpu_required, hip_step):
    """5 images with 5200 labels, which fs_group_loss cannot take; two updates of 5 images with map_loss and rank_weight 0.5,
    twice from identical initial weights: identical parameter bits, losses and rows; the parameters moved; two kernel calls."""
    from flingbot_amd import nets, train, trainops

    data = big_maps().to_device(DEV)
    torch.manual_seed(21)
    first = nets.SpatialValueNet(rgb_only=True, device=DEV).to(DEV)
    runs = []
    for _ in range(2):
        net = copy.deepcopy(first)
        opt = train.HipAdam(net.parameters(), lr=1e-3, weight_decay=1e-6) if hip_step else torch.optim.Adam(net.parameters(), lr=1e-3, weight_decay=1e-6)
        rows, launches = [], trainops.MapLossFunction.n_forward
        net.train()
        with train.deterministic_library_convs(not hip_step):
            losses = train.optimize_maps("fling", net, opt, data, 2, 5, np.random.default_rng(3), hip_step=hip_step, rank_weight=0.5,
                                         map_loss=True, stats=rows)
        net.eval()
        assert trainops.MapLossFunction.n_forward == launches + 2
        runs.append((losses, rows, net))
    (losses, rows, net), (losses_again, rows_again, net_again) = runs
    assert len(losses) == 2 and np.isfinite(losses).all() and losses == losses_again and rows == rows_again
    a, b, start = net.state_dict(), net_again.state_dict(), first.state_dict()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert any(not torch.equal(a[k], start[k]) for k in a if k.endswith("weight")) and int(net.steps) == 2
    rng = np.random.default_rng(3)
    for loss, row in zip(losses, rows):
        _, offsets, positions, _ = data.draw_maps(5, rng)
        assert row["labels"] == int(offsets[-1]) > 4096 and row["images"] == 5 and row["images_with_pairs"] == 5
        assert row["pairs"] == gref.host_pairs(data.labels[positions], mref.expanded_bounds(offsets)) > 0
        assert row["loss"] == loss and row["rank"] > 0.0 and 0.0 <= row["map_pair_accuracy"] <= 1.0
