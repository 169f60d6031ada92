"""Training on look-ahead lanes, the parts that need no GPU: train.plan_round against a literal restatement of the loop it
replaced, the `extra` scalars of taskio.save_replay, ExperienceSet(lane_ranks=...) and the keys of lookahead.save_replay."""
import itertools

import numpy as np
import pytest

D = 64


def _old_loop(size_before, n, warmup, update_frequency, save_ckpt):
    """train.run's loop over a round's n entries as it stood before plan_round, statement for statement, with the three
    actions recorded instead of done."""
    i, size = size_before, size_before + n
    out = []
    for _ in range(n):
        decay = update = checkpoint = False
        if i > warmup:
            decay = True
        if size > warmup:
            if i % update_frequency == 0:
                update = True
            if i % save_ckpt == 0:
                checkpoint = True
        i += 1
        out.append((decay, update, checkpoint))
    return out


@pytest.mark.parametrize("entries_before,warmup,update_frequency,save_ckpt",
                         list(itertools.product((0, 3, 130), (0, 2, 128), (1, 3), (1, 4))))
def test_plan_round_without_lanes_is_the_old_loop(entries_before, warmup, update_frequency, save_ckpt):
    from flingbot_amd import train

    for n in (0, 1, 6):
        got = train.plan_round(entries_before, [0] * n, warmup, update_frequency, save_ckpt)
        assert [tuple(bool(v) for v in row) for row in got] == _old_loop(entries_before, n, warmup, update_frequency, save_ckpt)


def test_plan_round_decays_once_per_observation():
    from flingbot_amd import train

    ranks = [0, 1, 2, 0, 1, 0]
    for before, warmup in ((0, 0), (0, 2), (3, 2), (3, 128), (130, 128)):
        plan = train.plan_round(before, ranks, warmup, 1, 4)
        decays = [t for t, row in enumerate(plan) if row[0]]
        assert decays == [t for t, r in enumerate(ranks) if r == 0 and before + t > warmup], (before, warmup)
        size = before + len(ranks)
        # updates and checkpoints count per label, whatever its rank
        assert [bool(row[1]) for row in plan] == [size > warmup] * len(ranks)
        assert [bool(row[2]) for row in plan] == [size > warmup and (before + t) % 4 == 0 for t in range(len(ranks))]
    assert [t for t, row in enumerate(train.plan_round(0, ranks, 0, 1, 4)) if row[0]] == [3, 5]    # (entry 0: i = 0 is not > warmup)
    assert [t for t, row in enumerate(train.plan_round(3, ranks, 2, 1, 4)) if row[0]] == [0, 3, 5]


# ---- files --------------------------------------------------------------------------------------------------------------------
TASKS = [dict(cloth_mass=0.5, flatten_area=2.0, task_difficulty="easy", initial_coverage=1.0),
         dict(cloth_mass=0.7, flatten_area=4.0, task_difficulty="hard", initial_coverage=1.2)]


def _arrays(pixel, fill):
    mask = np.zeros((D, D), bool)
    mask[pixel] = True
    return dict(observations=np.full((4, D, D), fill, np.float32), actions=mask, value_map=np.zeros((D, D), np.float32),
                max_indices=np.array([3, *pixel], np.int64), rotation=10.0, scale=1.5)


def _lane_record(task, step, rank, pre, post, pixel):
    return dict(coverage=[pre, post], actions=["fling"], rewards=[post - pre], preaction_coverage=[pre],
                experience=[_arrays(pixel, 0.25 + rank)], task=task, step=step, rank=rank)


def _episode_records():
    return [dict(coverage=[1.0, 1.5, 1.75], actions=["fling", "fling"], rewards=[0.5, 0.25], preaction_coverage=[1.0, 1.5],
                 experience=[_arrays((1, 2), 0.5), _arrays((3, 4), 0.75)]),
            dict(coverage=[1.2, 2.2], actions=["fling"], rewards=[1.0], preaction_coverage=[1.2], experience=[_arrays((5, 6), 1.0)])]


def test_save_replay_extra_is_additive(tmp_path):
    from flingbot_amd import taskio

    plain, tagged = str(tmp_path / "plain.npz"), str(tmp_path / "tagged.npz")
    recs = _episode_records()
    assert taskio.save_replay(plain, recs, TASKS) == 3
    with_extra = [dict(recs[0], extra=dict(lane_rank=2, note=7.5)), recs[1]]
    assert taskio.save_replay(tagged, with_extra, TASKS) == 3
    a, b = np.load(plain), np.load(tagged)
    keys = [str(k) for k in a["keys"]]
    assert keys == ["000000000_step00", "000000000_step01_last", "000000001_step00_last"] and keys == [str(k) for k in b["keys"]]
    # today's file: exactly the scalars, the arrays, `keys` and `format` -- nothing else
    want = {"keys", "format"} | {f"{k}/{f}" for k in keys for f in taskio.REPLAY_SCALARS + taskio.REPLAY_ARRAYS}
    assert set(a.files) == want
    # with extra: the same contents plus the record's scalars under every key of THAT record
    added = {f"{k}/{f}" for k in keys[:2] for f in ("lane_rank", "note")}
    assert set(b.files) == want | added
    for name in a.files:
        assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), name
    assert int(b["000000000_step01_last/lane_rank"]) == 2 and float(b["000000000_step00/note"]) == 7.5
    assert np.array_equal(np.sort(taskio.collect_stats(plain)["delta_coverage/easy/distribution"]),
                          np.sort(taskio.collect_stats(tagged)["delta_coverage/easy/distribution"]))
    with pytest.raises(ValueError):
        taskio.save_replay(str(tmp_path / "bad.npz"), [dict(recs[0], extra=dict(rewards=1.0))], TASKS[:1])


def _lane_stats():
    """8 lane-steps by hand: task 0 two steps of 3 and 2 lanes, task 1 one step of 3 lanes; step-major, task, rank."""
    recs = [_lane_record(0, 0, 0, 1.0, 1.5, (10, 11)), _lane_record(0, 0, 1, 1.0, 1.2, (12, 13)), _lane_record(0, 0, 2, 1.0, 0.9, (14, 15)),
            _lane_record(1, 0, 0, 1.2, 2.2, (20, 21)), _lane_record(1, 0, 1, 1.2, 0.8, (22, 23)), _lane_record(1, 0, 2, 1.2, 2.4, (24, 25)),
            _lane_record(0, 1, 0, 1.5, 1.6, (30, 31)), _lane_record(0, 1, 1, 1.5, 1.9, (32, 33))]
    steps = [[dict(candidates=[{}] * 3, followed_rank=0), dict(candidates=[{}] * 2, followed_rank=1)],
             [dict(candidates=[{}] * 3, followed_rank=2)]]
    return dict(lane_records=recs, lookahead=dict(steps=steps))


def test_lane_files_and_lane_ranks(tmp_path):
    from flingbot_amd import lookahead, taskio
    from flingbot_amd.replay import ExperienceSet

    stats = _lane_stats()
    lanes, plain = str(tmp_path / "lanes.npz"), str(tmp_path / "plain.npz")
    assert lookahead.save_replay(lanes, stats, TASKS) == 8
    assert "extra" not in stats["lane_records"][0]                        # the caller's records are left as they were
    assert taskio.save_replay(plain, _episode_records(), TASKS) == 3
    z = np.load(lanes)
    keys = [str(k) for k in z["keys"]]
    assert keys == [f"{i:09d}_step00_last" for i in range(8)]
    got = [[int(z[f"{k}/{f}"]) for f in ("lane_task", "lane_step", "lane_rank", "lane_followed")] for k in keys]
    assert got == [[0, 0, 0, 1], [0, 0, 1, 0], [0, 0, 2, 0], [1, 0, 0, 0], [1, 0, 1, 0], [1, 0, 2, 1], [0, 1, 0, 0], [0, 1, 1, 1]]
    everything = ExperienceSet(lanes, obs_color_jitter=False)
    assert len(everything) == 8 and everything.n_filtered == 0 and everything.lane_ranks is None
    first = ExperienceSet(lanes, obs_color_jitter=False, lane_ranks=[0])
    assert first.keys == [keys[0], keys[3], keys[6]] and first.n_filtered == 5
    want = np.array([(1.5 - 1.0) / 2.0, (2.2 - 1.2) / 4.0, (1.6 - 1.5) / 2.0], np.float64).astype(np.float32)
    assert np.array_equal(first.labels, want)                             # float64 arithmetic, stored as float32
    assert np.array_equal(first.observations[:, 0, 0, 0], np.float32([0.25, 0.25, 0.25]))
    rest = ExperienceSet(lanes, obs_color_jitter=False, lane_ranks=(1, 2))
    assert rest.keys == [keys[1], keys[2], keys[4], keys[5], keys[7]] and rest.n_filtered == 3
    assert sorted(first.keys + rest.keys) == everything.keys
    assert [tuple(int(v[0]) for v in np.nonzero(m)) for m in rest.masks] == [(12, 13), (14, 15), (22, 23), (24, 25), (32, 33)]
    # an ordinary file: every entry is the policy's own action, rank 0
    assert len(ExperienceSet(plain, lane_ranks=None)) == 3 and len(ExperienceSet(plain, lane_ranks=[0])) == 3
    none = ExperienceSet(plain, lane_ranks=[1, 2])
    assert len(none) == 0 and none.n_filtered == 3
    # both kinds in one set, and extend() filters like the constructor
    mixed = ExperienceSet([plain], lane_ranks=[0], obs_color_jitter=False)
    assert mixed.extend([lanes]) == 3 and len(mixed) == 6
    # collect_stats keeps reading both
    assert np.allclose(np.sort(taskio.collect_stats(lanes)["delta_coverage/easy/distribution"]), np.sort([0.25, 0.1, -0.05, 0.05, 0.2]))
    assert len(taskio.collect_stats(plain)["delta_coverage/easy/distribution"]) == 2


def test_lane_keys_do_not_collide_over_rounds(tmp_path):
    from flingbot_amd import lookahead
    from flingbot_amd.replay import ExperienceSet

    a, b = str(tmp_path / "replay_00000.npz"), str(tmp_path / "replay_00001.npz")
    stats = _lane_stats()
    stats["lane_records"] = stats["lane_records"][:5]
    assert lookahead.save_replay(a, stats, TASKS) == 5
    assert lookahead.save_replay(b, _lane_stats(), TASKS, first_record=5) == 8
    ka, kb = ([str(k) for k in np.load(p)["keys"]] for p in (a, b))
    assert ka == [f"{i:09d}_step00_last" for i in range(5)] and kb == [f"{i:09d}_step00_last" for i in range(5, 13)]
    assert not set(ka) & set(kb)
    both = ExperienceSet([a, b], obs_color_jitter=False)
    assert len(both) == 13 and len(set(both.keys)) == 13
    assert int(np.load(b)["000000005_step00_last/lane_rank"]) == 0 and int(np.load(b)["000000007_step00_last/lane_rank"]) == 2
