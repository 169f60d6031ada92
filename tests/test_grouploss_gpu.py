"""fs_group_loss (csrc/fs_grouploss.hip) on the GPU against the float64 restatement of grouploss_reference.py, its exact
properties, trainops.GroupLossFunction's backward, and optimize(rank_weight > 0) end to end.

The bound for every output is the issue's: |got - ref| <= (n + 16) 2^-24 A with the restatement's n addends of absolute sum A.
Largest |got - ref| / bound observed on an MI355X over all cases of this file: 0.194 (a dpred component at B = 4096, mixed
lengths); loss and mse stay below 0.068, rank below 0.071.  The float32 torch statement on the host: 0.122."""
import copy

import numpy as np
import pytest
import torch

import grouploss_reference as gref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, TAU = 0.5, 0.1

SIZES = (1, 2, 5, 64, 65, 256, 257, 1024, 4096)
CASES = [(B, kind) for B in SIZES for kind in ("singletons", "whole", "mixed", "fours")]
CASES += [(257, (60, 70)), (1024, (60, 70)),          # across the boundary of the first two waves
          (1024, (250, 262)), (4096, (250, 262)),     # across a 256-thread boundary
          (4096, (1020, 1030)),                       # across the block: samples 1024.. are a thread's second sample
          (4096, (3000, 4096))]                       # a long segment at the end of the largest batch
_ratios = {}


def _launch(pred, label, bounds, w=W, tau=TAU, gap=0.0, scale=1.0):
    from flingbot_amd import trainops

    p, y = torch.from_numpy(np.ascontiguousarray(pred, np.float32)).to(DEV), torch.from_numpy(np.ascontiguousarray(label, np.float32)).to(DEV)
    b = torch.from_numpy(np.ascontiguousarray(bounds, np.int32)).to(DEV)
    dpred, stats = trainops.GroupLossFunction._launch(p, y, b, w, tau, gap, scale)
    torch.cuda.synchronize()
    return dpred.cpu().numpy(), stats.cpu().numpy()


def _compare(name, dpred, stats, ref):
    """Every output against the restatement within the bound; P and C exactly.  Returns the largest |got - ref| / bound."""
    assert stats[3] == ref["pairs"] and stats[4] == ref["concordant"] and not stats[5:].any(), name
    worst = 0.0
    for k, out in enumerate(("loss", "mse", "rank")):
        value, n, A = ref[out]
        err, tol = abs(float(stats[k]) - value), float(gref.bound(n, A))
        print(f"{name}: {out} {stats[k]:.9g} ref {value:.12g} err {err:.3e} bound {tol:.3e}")
        assert err <= tol, (name, out, err, tol)
        worst = max(worst, err / tol if tol else 0.0)
    value, n, A = ref["dpred"]
    err, tol = np.abs(dpred.astype(np.float64) - value), gref.bound(n, A)
    ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), 0.0)
    print(f"{name}: dpred largest err / bound {ratio.max():.3f} at {int(ratio.argmax())}")
    assert (err <= tol).all(), (name, "dpred", int(np.argmax(err - tol)), float(err.max()))
    return max(worst, float(ratio.max()))


@pytest.mark.parametrize("B,kind", CASES, ids=[f"{B}-{kind if isinstance(kind, str) else '%d_%d' % kind}" for B, kind in CASES])
def test_kernel_against_the_float64_restatement(gpu_required, B, kind):
    pred, label = gref.batch(B, seed=B + 7)
    bounds = gref.layout(B, kind, seed=B)
    ref = gref.group_loss_f64(pred, label, bounds, W, TAU, 0.0)
    dpred, stats = _launch(pred, label, bounds)
    _ratios[(B, kind)] = _compare(f"B={B} {kind}", dpred, stats, ref)
    if kind == "singletons" or B == 1:
        assert ref["pairs"] == 0
    elif B >= 5:
        assert ref["pairs"] > 0
    # a second launch on equal inputs: equal bits
    again, stats_again = _launch(pred, label, bounds)
    assert np.array_equal(dpred.view(np.uint32), again.view(np.uint32)) and np.array_equal(stats.view(np.uint32), stats_again.view(np.uint32))
    print(f"largest err / bound so far over {len(_ratios)} cases: {max(_ratios.values()):.3f}")


@pytest.mark.parametrize("B,kind", [(5, "singletons"), (257, "singletons"), (64, "whole")])
def test_without_pairs_the_ranking_term_is_absent(gpu_required, B, kind):
    """P = 0 (singletons, or one segment of equal labels): rank has the bits of +0.0 and dpred those of a launch with w = 0."""
    pred, label = gref.batch(B, seed=B)
    if kind == "whole":
        label[:] = 0.25
    bounds = gref.layout(B, kind)
    dpred, stats = _launch(pred, label, bounds, w=W)
    plain, plain_stats = _launch(pred, label, gref.layout(B, "mixed"), w=0.0)
    assert stats[3] == 0 and stats[2:3].view(np.uint32)[0] == 0 and stats[0] == stats[1] == plain_stats[1]
    assert np.array_equal(dpred.view(np.uint32), plain.view(np.uint32))
    want = (np.float32(2.0) * (pred - label) / np.float32(B)).astype(np.float32)
    assert np.array_equal(dpred, want)


def test_gradient_scale_is_exact(gpu_required):
    pred, label = gref.batch(257, seed=1)
    bounds = gref.layout(257, "mixed", seed=4)
    one, stats = _launch(pred, label, bounds, scale=1.0)
    half, stats_half = _launch(pred, label, bounds, scale=0.5)
    assert stats[3] > 0 and np.array_equal(half, np.float32(0.5) * one) and np.array_equal(stats, stats_half)
    assert one.any()


def test_edge_values(gpu_required):
    # ties form no pair; min_gap drops the close ones
    y = np.float32([0.0, 0.05, 0.2, 0.2, 0.2, 0.0])
    p = np.float32([0.1, 0.0, 0.3, -0.1, 0.3, 0.1])
    bounds = gref.layout(6, "whole")
    edge = float(np.float32(0.2)) - float(np.float32(0.05))    # a gap at which label_j + gap lands on (or next to) label_i
    for gap in (0.0, 0.1, edge, 0.2):
        ref = gref.group_loss_f64(p, y, bounds, W, TAU, gap)
        dpred, stats = _launch(p, y, bounds, gap=gap)
        _compare(f"ties, gap {gap}", dpred, stats, ref)
    assert gref.host_pairs(y, bounds) == 11 and gref.host_pairs(y, bounds, 0.1) == 9 and gref.host_pairs(y, bounds, 0.2) == 6
    # |dp| / tau = 1e4, both signs: finite, the gradient saturated at 0 and at w / (P tau)
    for sign in (1.0, -1.0):
        y2, p2 = np.float32([1.0, 0.0]), np.float32([sign * 500.0, -sign * 500.0])
        ref = gref.group_loss_f64(p2, y2, gref.layout(2, "whole"), W, TAU, 0.0)
        dpred, stats = _launch(p2, y2, gref.layout(2, "whole"))
        assert np.isfinite(dpred).all() and np.isfinite(stats).all()
        _compare(f"saturated {sign:+.0f}", dpred, stats, ref)
        assert stats[2] == (0.0 if sign > 0 else 1e4)
    # tau = 1e-3: ordinary batches become saturated ones
    pred, label = gref.batch(65, seed=9)
    bounds = gref.layout(65, "fours")
    ref = gref.group_loss_f64(pred, label, bounds, W, 1e-3, 0.0)
    _compare("tau 1e-3", *_launch(pred, label, bounds, tau=1e-3), ref)
    # a large |x| that is NOT saturated: the addends are tiny and still good
    pred, label = gref.batch(64, seed=10, spread=3.0)
    ref = gref.group_loss_f64(pred, label, gref.layout(64, "whole"), W, TAU, 0.0)
    _compare("spread 3", *_launch(pred, label, gref.layout(64, "whole")), ref)
    # one NaN label: NaN loss, a clean return, and the NaN in no pair
    pred, label = gref.batch(65, seed=11)
    label[7] = np.nan
    bounds = gref.layout(65, "whole")
    dpred, stats = _launch(pred, label, bounds)
    keep = np.arange(65) != 7
    assert np.isnan(stats[0]) and np.isnan(stats[1]) and np.isfinite(stats[2])
    assert stats[3] == gref.host_pairs(label[keep], gref.layout(64, "whole")) > 0
    assert np.isnan(dpred[7]) and np.isfinite(dpred[keep]).all()
    assert torch.zeros(1, device=DEV).item() == 0.0


def test_a_malformed_table_is_refused_and_clamped(gpu_required):
    """The Python side refuses it (ValueError); the kernel, given it all the same, clamps and returns."""
    from flingbot_amd import trainops

    pred, label = gref.batch(5, seed=2)
    bad = np.int32([[-3, 9], [4, 2], [0, 100000], [-2147483648, 2147483647], [7, 8]])
    p = torch.from_numpy(pred).to(DEV).requires_grad_(True)
    with pytest.raises(ValueError):
        trainops.GroupLossFunction.apply(p, torch.from_numpy(label).to(DEV), torch.from_numpy(bad).to(DEV), W, TAU, 0.0)
    dpred, stats = _launch(pred, label, bad)
    clamped = np.int32([[0, 5], [4, 4], [0, 5], [0, 5], [5, 5]])
    ref = gref.group_loss_f64(pred, label, clamped, W, TAU, 0.0)
    assert stats[3] == ref["pairs"] and np.isfinite(dpred).all()


def test_autograd(gpu_required):
    """backward with a non-unit grad_output is grad_output * dpred; the host statement and the kernel agree within the bound."""
    from flingbot_amd import trainops

    B = 65
    pred, label = gref.batch(B, seed=12)
    bounds = gref.layout(B, "mixed", seed=5)
    ref = gref.group_loss_f64(pred, label, bounds, W, TAU, 0.0)
    dpred, stats = _launch(pred, label, bounds)
    p = torch.from_numpy(pred).to(DEV).requires_grad_(True)
    before = trainops.GroupLossFunction.n_forward
    loss, got_stats = trainops.GroupLossFunction.apply(p, torch.from_numpy(label).to(DEV), torch.from_numpy(bounds).to(DEV), W, TAU, 0.0)
    assert trainops.GroupLossFunction.n_forward == before + 1 and not got_stats.requires_grad and loss.requires_grad
    assert loss.item() == stats[0] and np.array_equal(got_stats.cpu().numpy(), stats)
    (loss * 3.5).backward()
    assert np.array_equal(p.grad.cpu().numpy(), np.float32(3.5) * dpred)
    # the CPU path: the same formula in float32 torch ops
    q = torch.from_numpy(pred).requires_grad_(True)
    host_loss, host_stats = trainops.GroupLossFunction.apply(q, torch.from_numpy(label), torch.from_numpy(bounds), W, TAU, 0.0)
    host_loss.backward()
    _compare("host float32", q.grad.numpy(), host_stats.numpy(), ref)
    for k, out in enumerate(("loss", "mse", "rank")):
        assert abs(float(host_stats[k]) - float(stats[k])) <= gref.bound(ref[out][1], ref[out][2])
    assert (np.abs(q.grad.numpy().astype(np.float64) - dpred) <= gref.bound(ref["dpred"][1], ref["dpred"][2])).all()
    # the torch statement runs on the GPU too (what the kernel is timed against): the same pairs, the same numbers to float32
    r = torch.from_numpy(pred).to(DEV).requires_grad_(True)
    t_loss, t_stats = trainops.group_loss_torch(r, torch.from_numpy(label).to(DEV), torch.from_numpy(bounds).to(DEV), W, TAU, 0.0)
    t_loss.backward()
    t_stats = t_stats.cpu().numpy()
    assert t_stats[3] == stats[3] and t_stats[4] == stats[4]
    assert np.allclose(t_stats[:3], stats[:3], rtol=1e-5, atol=0) and np.allclose(r.grad.cpu().numpy(), dpred, rtol=1e-4, atol=1e-7)


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def _toy_set(seed=0):
    from flingbot_amd.replay import ExperienceSet

    rng = np.random.default_rng(seed)
    obs = rng.random((16, 4, 64, 64), dtype=np.float32)
    masks = np.zeros((16, 64, 64), bool)
    masks[np.arange(16), rng.integers(8, 56, 16), rng.integers(8, 56, 16)] = True
    labels = (rng.standard_normal(16) * 0.1).astype(np.float32)
    return ExperienceSet.from_arrays(obs, masks, labels, groups=np.repeat(np.arange(4), 4))


@pytest.mark.parametrize("hip_step", [True, False])
def test_optimize_end_to_end(gpu_required, hip_step):
    """16 entries in 4 groups of 4; two updates at B = 8 with rank_weight 0.5, twice from identical initial weights: identical
    parameter bits, losses and statistics; the parameters moved; `pairs` is the host count for the batches drawn."""
    from flingbot_amd import nets, train, trainops

    data = _toy_set().to_device(DEV)
    torch.manual_seed(21)
    first = nets.SpatialValueNet(rgb_only=True, device=DEV).to(DEV)
    runs = []
    for _ in range(2):
        net = copy.deepcopy(first)
        opt = train.HipAdam(net.parameters(), lr=1e-3, weight_decay=1e-6) if hip_step else torch.optim.Adam(net.parameters(), lr=1e-3, weight_decay=1e-6)
        rows, launches = [], trainops.GroupLossFunction.n_forward
        net.train()
        with train.deterministic_library_convs(not hip_step):
            losses = train.optimize("fling", net, opt, data, 2, 8, np.random.default_rng(3), hip_step=hip_step, rank_weight=0.5, stats=rows)
        net.eval()
        assert trainops.GroupLossFunction.n_forward == launches + 2
        runs.append((losses, rows, net))
    (losses, rows, net), (losses_again, rows_again, net_again) = runs
    assert len(losses) == 2 and np.isfinite(losses).all() and losses == losses_again and rows == rows_again
    a, b, start = net.state_dict(), net_again.state_dict(), first.state_dict()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert any(not torch.equal(a[k], start[k]) for k in a if k.endswith("weight")) and int(net.steps) == 2
    rng = np.random.default_rng(3)
    for loss, row in zip(losses, rows):
        idx, bounds, _ = data.draw_groups(8, rng)
        assert row["pairs"] == gref.host_pairs(data.labels[idx], bounds) > 0 and 0 <= row["concordant"] <= row["pairs"]
        assert row["loss"] == loss and row["rank"] > 0.0 and np.isfinite([row["mse"], row["rank"]]).all()


def test_sample_groups_is_the_gather_of_draw_groups(gpu_required):
    data = _toy_set(seed=4).to_device(DEV)
    obs, mask, label, bounds = data.sample_groups(8, np.random.default_rng(6))
    idx, table, params = data.draw_groups(8, np.random.default_rng(6))
    want = data.gather(idx, params)
    assert bounds.dtype == torch.int32 and bounds.device == obs.device and np.array_equal(bounds.cpu().numpy(), table)
    assert np.array_equal(bounds.host, table)
    assert torch.equal(obs, want[0]) and torch.equal(mask, want[1]) and torch.equal(label, want[2])
    assert np.array_equal(label.cpu().numpy(), data.labels[idx])
