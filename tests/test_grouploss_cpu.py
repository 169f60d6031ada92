"""The grouped ranking loss without a GPU: trainops.group_loss_torch against the float64 restatement (grouploss_reference.py) and
against finite differences, its edge batches, ExperienceSet.groups / draw_groups, optimize with and without the ranking term on
a host policy, lookahead.pair_agreement, and the fs_group_loss entry point's header line, export and argument checks."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import grouploss_reference as gref
from test_lane_train_cpu import TASKS, _episode_records, _lane_record, _lane_stats
from test_train_cpu import HostSet, _policy, _same_bits, _write_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 64


def _torch64(pred, label, bounds, w, tau, gap):
    from flingbot_amd import trainops

    p = torch.tensor(np.asarray(pred, np.float64), requires_grad=True)
    loss, stats = trainops.group_loss_torch(p, torch.tensor(np.asarray(label, np.float64)), bounds, w, tau, gap)
    (grad,) = torch.autograd.grad(loss, p)
    return loss.item(), stats.numpy(), grad.numpy(), p


# ---- the torch statement against the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("B,kind", [(1, "whole"), (2, "whole"), (5, "mixed"), (16, "fours"), (37, "mixed"), (37, "whole"),
                                    (37, "singletons"), (80, (60, 70))])
@pytest.mark.parametrize("gap", [0.0, 0.05])
def test_torch_statement_in_float64_is_the_restatement(B, kind, gap):
    pred, label = gref.batch(B, seed=B)
    bounds = gref.layout(B, kind, seed=B)
    ref = gref.group_loss_f64(pred, label, bounds, 0.5, 0.1, gap)
    loss, stats, grad, _ = _torch64(pred, label, bounds, 0.5, 0.1, gap)
    for k, name in enumerate(("loss", "mse", "rank")):
        assert abs(stats[k] - ref[name][0]) <= 1e-13 * max(1.0, ref[name][2]), name
    assert loss == stats[0] and stats[3] == ref["pairs"] and stats[4] == ref["concordant"] and not stats[5:].any()
    assert np.abs(grad - ref["dpred"][0]).max() <= 1e-13 * max(1.0, ref["dpred"][2].max())


def test_autograd_gradient_agrees_with_central_differences():
    from flingbot_amd import trainops

    B = 12
    pred, label = gref.batch(B, seed=3)
    bounds = gref.layout(B, "fours")
    y = torch.tensor(label.astype(np.float64))
    _, _, grad, _ = _torch64(pred, label, bounds, 0.7, 0.1, 0.0)
    h = 1e-6
    for i in range(B):
        vals = []
        for sign in (1.0, -1.0):
            p = torch.tensor(pred.astype(np.float64))
            p[i] += sign * h
            vals.append(trainops.group_loss_torch(p, y, bounds, 0.7, 0.1, 0.0)[0].item())
        assert abs((vals[0] - vals[1]) / (2 * h) - grad[i]) <= 1e-7 * max(1.0, abs(grad[i])), i


def test_edge_batches():
    B = 8
    pred, label = gref.batch(B, seed=5)
    mse_grad = 2.0 * (pred.astype(np.float64) - label.astype(np.float64)) / B
    # all singletons: no pair, rank exactly 0, the gradient is the regression's
    loss, stats, grad, _ = _torch64(pred, label, gref.layout(B, "singletons"), 0.5, 0.1, 0.0)
    assert stats[2] == 0.0 and stats[3] == 0 and loss == stats[1] and np.array_equal(grad, mse_grad)
    # one segment holding the whole batch: every pair of different labels, once
    loss, stats, grad, _ = _torch64(pred, label, gref.layout(B, "whole"), 0.5, 0.1, 0.0)
    want = sum(1 for i in range(B) for j in range(B) if label[i] > label[j])
    assert stats[3] == want > 0 and stats[2] > 0.0 and loss > stats[1]
    # equal labels: no pair
    loss, stats, grad, _ = _torch64(pred, np.full(B, 0.25, np.float32), gref.layout(B, "whole"), 0.5, 0.1, 0.0)
    assert stats[3] == 0 and stats[2] == 0.0
    # min_gap excludes the close pairs only
    y = np.float32([0.0, 0.05, 0.2, 0.2])
    p = np.float32([0.1, 0.0, 0.3, -0.1])
    _, s0, _, _ = _torch64(p, y, gref.layout(4, "whole"), 0.5, 0.1, 0.0)
    _, s1, _, _ = _torch64(p, y, gref.layout(4, "whole"), 0.5, 0.1, 0.1)
    assert s0[3] == 5 and s1[3] == 4 and s0[4] == 2 and s1[4] == 2        # (1, 0) is the pair the gap drops; it was discordant


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_saturated_margins_stay_finite(sign):
    """|dp| / tau = 1e4 with the better sample far ahead (the pair costs nothing, no gradient) and far behind (the pair costs
    |x|, the gradient is the full weight / (P tau))."""
    y = np.float32([1.0, 0.0])
    p = np.float32([sign * 500.0, -sign * 500.0])                          # dp = +-1000, tau = 0.1
    loss, stats, grad, _ = _torch64(p, y, gref.layout(2, "whole"), 0.5, 0.1, 0.0)
    assert np.isfinite(loss) and np.isfinite(grad).all() and stats[3] == 1 and stats[4] == (1 if sign > 0 else 0)
    rank_grad = grad - 2.0 * (p.astype(np.float64) - y) / 2
    if sign > 0:
        assert stats[2] == 0.0 and np.array_equal(rank_grad, [0.0, 0.0])
    else:
        assert abs(stats[2] - 1e4) <= 1e-8 and np.allclose(rank_grad, [-0.5 / 0.1, 0.5 / 0.1], rtol=1e-12, atol=0)
    ref = gref.group_loss_f64(p, y, gref.layout(2, "whole"), 0.5, 0.1, 0.0)
    assert np.isfinite(ref["loss"][0]) and np.allclose(ref["dpred"][0], grad, rtol=1e-12, atol=0)


def test_a_nan_label_makes_the_loss_nan():
    pred, label = gref.batch(8, seed=6)
    label[3] = np.nan
    loss, stats, _, _ = _torch64(pred, label, gref.layout(8, "whole"), 0.5, 0.1, 0.0)
    clean = gref.host_pairs(np.delete(label, 3), gref.layout(7, "whole"))
    assert np.isnan(loss) and np.isnan(stats[0]) and np.isnan(stats[1]) and stats[3] == clean   # the NaN joins no pair


def test_group_loss_function_on_the_host_is_the_torch_statement():
    from flingbot_amd import trainops

    pred, label = gref.batch(9, seed=8)
    bounds = torch.from_numpy(gref.layout(9, "mixed", seed=2))
    p = torch.tensor(pred, requires_grad=True)
    loss, stats = trainops.GroupLossFunction.apply(p, torch.tensor(label), bounds, 0.5, 0.1, 0.0)
    assert loss.shape == () and stats.shape == (8,) and not stats.requires_grad
    (3.0 * loss).backward()
    q = torch.tensor(pred, requires_grad=True)
    want, want_stats = trainops.group_loss_torch(q, torch.tensor(label), bounds, 0.5, 0.1, 0.0)
    (3.0 * want).backward()
    assert torch.equal(loss, want.detach()) and torch.equal(stats, want_stats) and torch.allclose(p.grad, q.grad, rtol=1e-6, atol=0)
    for bad in ([[0, 2], [0, 1]], [[0, 1], [0, 2]], [[1, 2], [1, 2]], [[0, 3], [0, 3]]):       # a table that is not one
        with pytest.raises(ValueError):
            trainops.GroupLossFunction.apply(torch.zeros(2), torch.zeros(2), torch.tensor(bad, dtype=torch.int32), 0.5, 0.1, 0.0)
    for w, tau, gap in ((-1.0, 0.1, 0.0), (0.5, 0.0, 0.0), (0.5, 0.1, -0.1), (float("nan"), 0.1, 0.0), (0.5, float("inf"), 0.0)):
        with pytest.raises(ValueError):
            trainops.GroupLossFunction.apply(torch.zeros(2), torch.zeros(2), torch.tensor([[0, 2], [0, 2]]), w, tau, gap)


# ---- groups -------------------------------------------------------------------------------------------------------------------
def _lane_files(tmp_path):
    """lanes.npz: the eight hand-made lane-steps of test_lane_train_cpu plus one lane without arrays; plain.npz: three
    ordinary entries; again.npz: the same (task, step) pairs once more, as a later round writes them."""
    from flingbot_amd import lookahead, taskio

    stats = _lane_stats()
    ghost = _lane_record(1, 0, 3, 1.2, 1.3, (26, 27))
    ghost["experience"] = [None]                                           # a lane whose step had no valid action: no arrays
    stats["lane_records"].insert(6, ghost)
    stats["lookahead"]["steps"][1][0]["candidates"] = [{}] * 4
    lanes, plain, again = (str(tmp_path / n) for n in ("lanes.npz", "plain.npz", "again.npz"))
    assert lookahead.save_replay(lanes, stats, TASKS) == 9
    assert taskio.save_replay(plain, _episode_records(), TASKS, first_episode=100) == 3
    assert lookahead.save_replay(again, _lane_stats(), TASKS, first_record=200) == 8
    return lanes, plain, again


def test_groups_follow_task_and_step_within_one_file(tmp_path):
    from flingbot_amd.replay import ExperienceSet

    lanes, plain, again = _lane_files(tmp_path)
    data = ExperienceSet(lanes, obs_color_jitter=False)
    assert len(data) == 8 and data.n_without_arrays == 1
    assert data.groups.dtype == np.int64 and data.groups.tolist() == [0, 0, 0, 1, 1, 1, 2, 2]    # (task, step): (0,0) (1,0) (0,1)
    # lane_ranks filters first: what is left of a group is the group
    assert ExperienceSet(lanes, lane_ranks=[1, 2]).groups.tolist() == [0, 0, 1, 1, 2]
    assert ExperienceSet(lanes, lane_ranks=[0]).groups.tolist() == [0, 1, 2]
    # an ordinary file: every entry on its own
    assert ExperienceSet(plain).groups.tolist() == [0, 1, 2]
    # the same (task, step) in a second file is another group; extend equals all-at-once
    both = ExperienceSet([lanes, plain, again], obs_color_jitter=False)
    assert both.groups.tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 3, 4, 5, 6, 6, 6, 7, 7, 7, 8, 8]
    grown = ExperienceSet(lanes, obs_color_jitter=False)
    assert grown.extend([plain]) == 3 and grown.extend([again]) == 8
    assert np.array_equal(grown.groups, both.groups) and grown.keys == both.keys and np.array_equal(grown.labels, both.labels)
    assert [m.tolist() for m in grown.group_members()] == [m.tolist() for m in both.group_members()]
    # from_arrays: given groups, or one per entry
    obs, masks = np.zeros((4, 4, D, D), np.float32), np.zeros((4, D, D), bool)
    assert ExperienceSet.from_arrays(obs, masks, np.zeros(4)).groups.tolist() == [0, 1, 2, 3]
    assert ExperienceSet.from_arrays(obs, masks, np.zeros(4), groups=[7, 7, 2, 7]).groups.tolist() == [7, 7, 2, 7]
    with pytest.raises(ValueError):
        ExperienceSet.from_arrays(obs, masks, np.zeros(4), groups=[1, 2])


def _toy_set(n_groups=4, per_group=4, seed=0, **kw):
    from flingbot_amd.replay import ExperienceSet

    rng = np.random.default_rng(seed)
    n = n_groups * per_group
    obs = rng.random((n, 4, D, D), dtype=np.float32)
    masks = np.zeros((n, D, D), bool)
    masks[np.arange(n), rng.integers(8, 56, n), rng.integers(8, 56, n)] = True
    labels = (rng.standard_normal(n) * 0.1).astype(np.float32)
    return ExperienceSet.from_arrays(obs, masks, labels, groups=np.repeat(np.arange(n_groups), per_group), **kw)


def test_draw_groups():
    from flingbot_amd.replay import ExperienceSet

    obs, masks = np.zeros((10, 4, D, D), np.float32), np.zeros((10, D, D), bool)
    groups = [5, 9, 5, 5, 2, 9, 2, 2, 2, 11]                               # first appearance: 5, 9, 2, 11
    data = ExperienceSet.from_arrays(obs, masks, np.arange(10), groups=groups)
    members = [m.tolist() for m in data.group_members()]
    assert members == [[0, 2, 3], [1, 5], [4, 6, 7, 8], [9]]
    seen_repeat = False
    for seed in range(40):
        idx, bounds, params = data.draw_groups(7, np.random.default_rng(seed))
        again = data.draw_groups(7, np.random.default_rng(seed))
        assert np.array_equal(idx, again[0]) and np.array_equal(bounds, again[1])
        assert all(np.array_equal(params[k], again[2][k]) for k in params) and params["order"].shape == (7, 4)
        assert idx.dtype == np.int64 and idx.shape == (7,) and bounds.dtype == np.int32 and bounds.shape == (7, 2)
        # the same draws, replayed by hand
        rng, at, segments = np.random.default_rng(seed), 0, []
        while at < 7:
            m = members[int(rng.integers(0, 4))][:7 - at]
            segments.append((at, at + len(m), m))
            at += len(m)
        for n, (lo, hi, m) in enumerate(segments):
            assert idx[lo:hi].tolist() == m and (bounds[lo:hi] == (lo, hi)).all()
            whole = m in members
            assert whole or n == len(segments) - 1                         # only the last segment can be cut
        firsts = [s[2][0] for s in segments]
        if any(a == b for a, b in zip(firsts, firsts[1:])):                # one group twice in a row: two segments
            seen_repeat = True
    assert seen_repeat
    quiet = ExperienceSet.from_arrays(obs, masks, np.arange(10), groups=groups, obs_color_jitter=False)
    assert quiet.draw_groups(3, np.random.default_rng(0))[2] is None
    with pytest.raises(ValueError):
        ExperienceSet([]).draw_groups(2, np.random.default_rng(0))


# ---- optimize -----------------------------------------------------------------------------------------------------------------
class HostGroupSet(HostSet):
    """HostSet with sample_groups: the same draws as ExperienceSet.sample_groups, served by item_host."""

    def sample_groups(self, batch_size, rng):
        idx, bounds, params = self.data.draw_groups(batch_size, rng)
        obs, mask, label = self.data.item_host(idx, params)
        return torch.from_numpy(obs), torch.from_numpy(mask), torch.from_numpy(label), torch.from_numpy(bounds)


def _todays_loop_body(value_net, optimizer, data, num_updates, batch_size, rng):
    """train.optimize's loop as it stood before the ranking term (hip_step=False), statement for statement."""
    losses = []
    device = next(value_net.parameters()).device
    for _ in range(int(num_updates)):
        obs, action_mask, label = data.sample(batch_size, rng)
        value_pred_dense = value_net(obs.to(device, non_blocking=True))
        value_pred = torch.masked_select(value_pred_dense.squeeze(), action_mask.to(device, non_blocking=True))
        loss = torch.nn.functional.mse_loss(value_pred, label.to(device, non_blocking=True))
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        value_net.steps += 1
        losses.append(loss.cpu().item())
    return losses


def test_optimize_with_weight_zero_is_todays_loop(tmp_path, monkeypatch):
    from flingbot_amd import replay, train, trainops

    path = str(tmp_path / "set.npz")
    _write_set(path, 6, seed=1)
    data = HostGroupSet(replay.ExperienceSet(path, action_primitive="fling"))
    monkeypatch.setattr(HostGroupSet, "sample_groups", lambda *a: pytest.fail("weight 0 draws with sample()"))
    monkeypatch.setattr(trainops.GroupLossFunction, "forward", lambda *a: pytest.fail("weight 0 uses mse_loss"))
    mine, ref = _policy(3), _policy(3)
    opt_mine, opt_ref = train.make_optimizer(mine), train.make_optimizer(ref)
    mine.train(); ref.train()
    rows = []
    got = train.optimize("fling", mine.value_nets["fling"], opt_mine, data, 3, 4, np.random.default_rng(11), rank_weight=0, stats=rows)
    want = _todays_loop_body(ref.value_nets["fling"], opt_ref, data, 3, 4, np.random.default_rng(11))
    mine.eval(); ref.eval()
    assert got == want and len(got) == 3 and rows == []
    _same_bits(mine, ref)
    sig = inspect.signature(train.optimize).parameters
    assert (sig["rank_weight"].default, sig["rank_temperature"].default, sig["rank_min_gap"].default) == (0.0, 0.1, 0.0)
    sig = inspect.signature(train.run).parameters
    assert (sig["rank_weight"].default, sig["rank_temperature"].default, sig["rank_min_gap"].default) == (0.0, 0.1, 0.0)
    assert "guess" in train.optimize.__doc__
    for bad in (dict(rank_weight=-1.0), dict(rank_weight=float("nan")), dict(rank_temperature=0.0), dict(rank_min_gap=-0.5)):
        with pytest.raises(ValueError):
            train.optimize("fling", mine.value_nets["fling"], opt_mine, data, 1, 4, np.random.default_rng(0), **bad)


def test_optimize_with_the_ranking_term_on_a_host_policy():
    from flingbot_amd import train

    raw = _toy_set(4, 4, seed=2)
    data = HostGroupSet(raw)
    pol, fresh = _policy(5), _policy(5)
    opt = train.make_optimizer(pol)
    pol.train()
    rows = []
    losses = train.optimize("fling", pol.value_nets["fling"], opt, data, 2, 8, np.random.default_rng(4), rank_weight=0.5, stats=rows)
    pol.eval()
    assert len(losses) == 2 == len(rows) and np.isfinite(losses).all() and int(pol.value_nets["fling"].steps) == 2
    rng = np.random.default_rng(4)
    for loss, row in zip(losses, rows):
        idx, bounds, _ = raw.draw_groups(8, rng)
        assert set(row) == {"loss", "mse", "rank", "pairs", "concordant"} and np.isfinite([row[k] for k in row]).all()
        assert row["pairs"] == gref.host_pairs(raw.labels[idx], bounds) > 0 and 0 <= row["concordant"] <= row["pairs"]
        assert row["loss"] == loss and abs(loss - (row["mse"] + 0.5 * row["rank"])) <= 1e-6 * loss and row["rank"] > 0
    moved = [k for k, v in pol.state_dict().items() if not torch.equal(v, fresh.state_dict()[k])]
    assert any(k.endswith("conv1.weight") for k in moved)
    # a set without lanes: every segment one sample, no pair, the regression alone
    lone = HostGroupSet(_toy_set(16, 1, seed=3))
    rows = []
    pol.train()
    losses = train.optimize("fling", pol.value_nets["fling"], opt, lone, 1, 8, np.random.default_rng(1), rank_weight=0.5, stats=rows)
    pol.eval()
    assert rows[0]["pairs"] == 0 and rows[0]["rank"] == 0.0 and rows[0]["loss"] == rows[0]["mse"] == losses[0]


def test_command_line_flags():
    from flingbot_amd import train

    a = train.build_parser().parse_args(["--log", "x", "--tasks", "y"])
    assert (a.rank_weight, a.rank_temperature, a.rank_min_gap) == (0.0, 0.1, 0.0)
    a = train.build_parser().parse_args(["--log", "x", "--tasks", "y", "--rank-weight", "0.5", "--rank-temperature", "0.05",
                                         "--rank-min-gap", "0.01"])
    assert (a.rank_weight, a.rank_temperature, a.rank_min_gap) == (0.5, 0.05, 0.01)
    for bad in (["--rank-weight", "-0.5"], ["--rank-weight", "nan"], ["--rank-temperature", "0"], ["--rank-temperature", "inf"],
                ["--rank-min-gap", "-1"]):
        with pytest.raises(SystemExit):
            train.main(["--log", "x", "--tasks", "y"] + bad)


def test_pair_agreement():
    from flingbot_amd import lookahead

    c = lambda value, reward: dict(value=value, reward=reward)   # noqa: E731
    steps = [[dict(candidates=[c(0.9, 0.1), c(0.5, 0.3), c(0.2, 0.1)], followed_rank=0),     # 0.3 > 0.1 twice: one concordant
              dict(candidates=[c(0.4, 0.2)], followed_rank=0)],                                # a lone lane: no pair
             [dict(candidates=[], followed_rank=0),
              dict(candidates=[c(0.7, 0.5), c(0.6, 0.45)], followed_rank=0)]]                  # one pair, concordant
    assert lookahead.pair_agreement(steps) == (3, 2)
    assert lookahead.pair_agreement(steps, min_gap=0.1) == (2, 1)
    assert lookahead.pair_agreement(steps, min_gap=1.0) == (0, 0) and lookahead.pair_agreement([]) == (0, 0)


# ---- header and library -------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_point():
    from flingbot_amd import build, sim as fsim

    with open(os.path.join(ROOT, "include", "flingsim.h")) as fh:
        header = fh.read()
    assert re.search(r"^int fs_group_loss\(", header, re.M)
    lib = fsim.load_library()
    assert lib.fs_group_loss is not None and "fs_group_loss" in lib._fs_symbols
    assert "fs_grouploss.hip" in build.LIB_SOURCES


def test_entry_point_refuses_bad_scalars_and_pointers():
    """FS_ERR_ARG before any HIP call: the pointers are host addresses that are never dereferenced."""
    from flingbot_amd import sim as fsim

    lib = fsim.load_library()
    buf = np.zeros(4096, np.float32)
    at = lambda k: C.c_void_p(buf.ctypes.data + 64 * k)   # noqa: E731
    ok = dict(pred=at(0), label=at(1), bounds=at(2), batch=4, w=0.5, tau=0.1, gap=0.0, s=1.0, dpred=at(3), stats=at(4))
    call = lambda **a: lib.fs_group_loss(a["pred"], a["label"], a["bounds"], a["batch"], a["w"], a["tau"], a["gap"], a["s"],   # noqa: E731
                                         a["dpred"], a["stats"], None)
    nan, inf = float("nan"), float("inf")
    cases = [dict(batch=0), dict(batch=-3), dict(batch=4097), dict(w=-0.1), dict(w=nan), dict(w=inf), dict(tau=0.0), dict(tau=-0.1),
             dict(tau=nan), dict(tau=inf), dict(gap=-1e-9), dict(gap=nan), dict(gap=inf), dict(s=nan), dict(s=inf), dict(s=-inf)]
    cases += [{k: C.c_void_p(None)} for k in ("pred", "label", "bounds", "dpred", "stats")]
    cases += [{k: C.c_void_p(buf.ctypes.data + 2)} for k in ("pred", "label", "bounds", "dpred", "stats")]
    for kw in cases:
        assert call(**{**ok, **kw}) == -1, kw                               # FS_ERR_ARG
        assert b"fs_group_loss" in lib.fs_last_error(), kw
