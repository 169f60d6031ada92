"""The host half of the look-ahead rollouts (flingbot_amd/lookahead.py, ActionSelector.candidates' walk): no GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the candidate walk over one observation's map winners ---------------------------------------------------------------
def _walk(index, value, k, refuse=(), same=()):
    """walk_winners with a validator that refuses the flat indices in `refuse` and gives the flat indices of each group in
    `same` one identity (one primitive and pixel pair)."""
    from flingbot_amd.action import walk_winners

    seen = []

    def validate(flat):
        seen.append(flat)
        if flat in refuse:
            return None
        ident = next((("group", g) for g, members in enumerate(same) if flat in members), ("own", flat))
        return ident, f"action{flat}"

    taken, refused = walk_winners(np.array(index), np.array(value, np.float32), k, validate)
    return [item for item, _ in taken], [float(v) for _, v in taken], refused, seen


def test_walk_orders_by_value_then_index():
    index = [[40, 10, -1], [30, 20, 50]]           # [P = 2][T = 3]; one map without a valid candidate
    value = [[0.5, 0.9, 9.0], [0.9, 0.7, 0.5]]     # (its value must never be looked at)
    items, values, refused, seen = _walk(index, value, 6)
    # 0.9 twice: the lower flattened index first; 0.5 twice likewise
    assert items == ["action10", "action30", "action20", "action40", "action50"] and refused is None
    assert values == [np.float32(v) for v in (0.9, 0.9, 0.7, 0.5, 0.5)]
    assert seen == [10, 30, 20, 40, 50]            # fewer than k: every winner was visited, none twice


def test_walk_stops_at_k_without_validating_further():
    items, _, refused, seen = _walk([[40, 10, 60], [30, 20, 50]], [[0.5, 0.9, 0.1], [0.8, 0.7, 0.6]], 2)
    assert items == ["action10", "action30"] and refused is None and seen == [10, 30]


def test_walk_drops_duplicates_and_keeps_looking():
    # 10 and 30 are one action (the same primitive and pretransform pixel pair reached through two transforms)
    items, _, refused, _ = _walk([[40, 10, 60], [30, 20, 50]], [[0.5, 0.9, 0.1], [0.8, 0.7, 0.6]], 3, same=[{10, 30}])
    assert items == ["action10", "action20", "action50"] and refused is None
    # candidate 0 is never a duplicate: it is the best winner, whatever follows
    items, _, _, _ = _walk([[40, 10, 60], [30, 20, 50]], [[0.5, 0.9, 0.1], [0.8, 0.7, 0.6]], 1, same=[{10, 30, 20, 50, 40, 60}])
    assert items == ["action10"]


def test_walk_reports_what_the_host_refuses():
    items, _, refused, seen = _walk([[40, 10, 60], [30, 20, 50]], [[0.5, 0.9, 0.1], [0.8, 0.7, 0.6]], 3, refuse={30})
    assert refused == 30 and items == ["action10"] and seen == [10, 30]   # the caller masks the entry and asks again


def test_walk_of_nothing():
    assert _walk([[-1, -1]], [[0.0, 0.0]], 3)[:3] == ([], [], None)
    assert _walk([[5, 7]], [[0.1, 0.2]], 0)[:3] == ([], [], None)


# ---- slots, followed rank, means ------------------------------------------------------------------------------------------
def test_group_slots_and_followed_rank():
    from flingbot_amd import lookahead

    assert lookahead.group_slots(6, 3) == [[0, 2, 4], [1, 3, 5]]
    assert lookahead.group_slots(7, 3) == [[0, 2, 4], [1, 3, 5]]          # a slot that fills no group stays empty
    assert lookahead.group_slots(4, 1) == [[0], [1], [2], [3]]
    with pytest.raises(ValueError):
        lookahead.group_slots(2, 3)
    assert lookahead.choose_followed([0.1, 0.3, 0.3], "policy") == 0
    assert lookahead.choose_followed([0.1, 0.3, 0.3], "best") == 1        # ties: the lowest rank
    assert lookahead.choose_followed([0.3, 0.3], "best") == 0
    assert lookahead.choose_followed([-0.2, -0.1], "best") == 1
    assert lookahead.choose_followed([], "best") == 0                      # no valid candidate: the trunk
    with pytest.raises(ValueError):
        lookahead.choose_followed([0.1], "worst")


def test_summarize_means():
    from flingbot_amd import lookahead

    c = lambda *r: dict(candidates=[dict(reward=v) for v in r], followed_rank=0)   # noqa: E731
    steps = [[c(0.2, 0.4, 0.1), c(0.3)], [c(-1.0, -3.0), c()]]      # task 1 has flatten_area 2; its last step had no candidate
    s = lookahead.summarize(steps, [1.0, 2.0], 3)
    assert s["n_steps"] == 3 and s["n_lane_steps"] == 6
    assert s["regret"] == pytest.approx((0.2 + 0.0 + 0.0) / 3) and s["regret"] >= 0
    assert s["rank0_best_frac"] == pytest.approx(2 / 3)
    assert s["mean_reward_per_rank"] == [pytest.approx((0.2 + 0.3 - 0.5) / 3), pytest.approx((0.4 - 1.5) / 2), pytest.approx(0.1)]
    empty = lookahead.summarize([[c()]], [1.0], 2)
    assert empty["regret"] is None and empty["mean_reward_per_rank"] == [None, None] and empty["n_steps"] == 0


# ---- lane records -> replay file ------------------------------------------------------------------------------------------
def _lane_record(task, step, rank, pre, post, pixel, primitive="fling", arrays=True):
    D = 64
    exp = None
    if arrays:
        mask = np.zeros((D, D), bool)
        mask[pixel] = True
        exp = dict(observations=np.full((4, D, D), 0.25 + rank, np.float32), actions=mask,
                   value_map=np.zeros((D, D), np.float32), max_indices=np.array([3, *pixel], np.int64), rotation=10.0, scale=1.5)
    return dict(coverage=[pre, post], actions=[primitive], rewards=[post - pre], preaction_coverage=[pre], experience=[exp],
                task=task, step=step, rank=rank)


def test_save_replay_expands_the_task_list(tmp_path):
    from flingbot_amd import lookahead, taskio
    from flingbot_amd.replay import ExperienceSet

    tasks = [dict(cloth_mass=0.5, flatten_area=2.0, task_difficulty="easy", initial_coverage=1.0),
             dict(cloth_mass=0.7, flatten_area=4.0, task_difficulty="hard", initial_coverage=1.2)]
    recs = [_lane_record(0, 0, 0, 1.0, 1.5, (10, 11)), _lane_record(0, 0, 1, 1.0, 1.2, (12, 13)),
            _lane_record(1, 0, 0, 1.2, 2.2, (20, 21)), _lane_record(1, 0, 1, 1.2, 0.8, (22, 23)),
            _lane_record(1, 0, 2, 1.2, 1.2, (24, 25)), _lane_record(1, 1, 0, 2.2, 3.0, (30, 31), arrays=False)]
    assert [t["flatten_area"] for t in lookahead.expand_tasks(recs, tasks)] == [2.0, 2.0, 4.0, 4.0, 4.0, 4.0]
    path = str(tmp_path / "lanes.npz")
    assert lookahead.save_replay(path, dict(lane_records=recs), tasks) == 6
    with pytest.raises(ValueError):
        lookahead.save_replay(path + "x", dict(records=[]), tasks)
    z = np.load(path)
    keys = [str(k) for k in z["keys"]]
    assert keys == [f"{i:09d}_step00_last" for i in range(6)]             # every lane-step is a one-action episode
    assert [float(z[f"{k}/max_coverage"]) for k in keys] == [2.0, 2.0, 4.0, 4.0, 4.0, 4.0]
    assert [str(z[f"{k}/task_difficulty"]) for k in keys] == ["easy", "easy", "hard", "hard", "hard", "hard"]
    # K labels per observation, each normalised by ITS task's flattened area
    ds = ExperienceSet(path, obs_color_jitter=False)
    assert len(ds.keys) == 5 and ds.n_without_arrays == 1 and ds.n_invalid == 0
    want = np.array([0.5 / 2, 0.2 / 2, 1.0 / 4, -0.4 / 4, 0.0], np.float64).astype(np.float32)
    assert np.array_equal(ds.labels, want)
    assert [tuple(int(v[0]) for v in np.nonzero(m)) for m in ds.masks] == [(10, 11), (12, 13), (20, 21), (22, 23), (24, 25)]
    assert np.array_equal(ds.observations[:, 0, 0, 0], np.float32([0.25, 1.25, 0.25, 1.25, 2.25]))
    stats = taskio.collect_stats(path)
    assert np.allclose(np.sort(stats["delta_coverage/easy/distribution"]), np.sort([0.25, 0.1]))
    assert np.allclose(np.sort(stats["delta_coverage/hard/distribution"]), np.sort([0.25, -0.1, 0.0, 0.2]))
    assert stats["action_primitive/percent_fling"] == 1.0
    assert list(stats["episode_length/hard/distribution"]) == [0, 0, 0, 0]


# ---- the command line -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,message", [
    (["--lookahead", "3", "--gpus", "2"], "one GPU"),
    (["--lookahead", "3", "--report", "out"], "--report"),
    (["--lookahead", "3", "--dump-visualizations", "out"], "--dump-visualizations"),
    (["--lookahead", "0"], "K >= 1"),
    (["--lookahead", "8", "--slots", "4"], "--slots"),
    (["--lookahead", "2", "--follow", "worst"], "--follow"),
])
def test_command_line_refusals(capsys, monkeypatch, extra, message):
    from flingbot_amd import evaluate

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    ap = evaluate.build_parser()
    with pytest.raises(SystemExit) as err:
        evaluate.parse_lookahead_options(ap, ap.parse_args(["--tasks", "set.npz"] + extra))
    assert err.value.code == 2 and message in capsys.readouterr().err


def test_command_line_accepts_lookahead(monkeypatch):
    from flingbot_amd import evaluate

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    ap = evaluate.build_parser()
    a = evaluate.parse_lookahead_options(ap, ap.parse_args(["--tasks", "set.npz", "--lookahead", "4", "--follow", "best"]))
    assert a.lookahead == 4 and a.follow == "best"
    a = evaluate.parse_lookahead_options(ap, ap.parse_args(["--tasks", "set.npz", "--gpus", "2", "--report", "x"]))
    assert a.lookahead is None and a.follow == "policy"      # without --lookahead nothing is checked here, as before


# ---- header and library ---------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    from flingbot_amd import sim as fsim

    with open(os.path.join(ROOT, "include", "flingsim.h")) as fh:
        header = fh.read()
    assert re.search(r"\bint fs_fork\(fs_ctx \*ctx, int n, const int \*src, const int \*dst\);", header)
    assert re.search(r"\bint fs_transform_winners\(const float \*d_values, int n, int n_primitives,", header)
    assert re.search(r"\bsize_t fs_transform_winners_work_bytes\(int n, int n_primitives, int n_transforms\);", header)
    lib = fsim.load_library()
    for name in ("fs_fork", "fs_transform_winners", "fs_transform_winners_work_bytes"):
        assert hasattr(lib, name) and name in lib._fs_symbols
    assert lib.fs_transform_winners_work_bytes(0, 2, 6) == 0
    need = lib.fs_transform_winners_work_bytes(3, 2, 6)
    assert need >= 3 * 6 * 9 * 8 + 3 * 2 * 6 * 16                       # the matrices and one (value, index) per map
    # host-side refusals need no device: a null context, and bad arguments of the stateless call
    assert lib.fs_fork(None, 1, None, None) == -1 and b"fs_fork" in lib.fs_last_error()
    assert lib.fs_transform_winners(None, 1, 1, None, 1, 32, 4, 4, 4, None, None, 48, 1.0, None, None, None, 1.0, 0.3, 0.02,
                                    None, None, None, None) == -1
    assert b"fs_transform_winners" in lib.fs_last_error()
