"""lookahead.run_episodes(lanes="sampled") end to end, on the fixtures of tests/test_lookahead_gpu.py: two generated tasks, k = 3
lanes per episode in six slots of one context.  Lane 0 stays the net's arg-max, so follow="policy" must still reproduce
evaluate.run_episodes EXACTLY; the other lanes are a keyed draw -- a function of the seed -- of on-cloth actions."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K, ROTATIONS, SCALES, SEED = 3, 3, (1.0, 1.5), 2


def _env_policy(slots, **env_kwargs):
    from flingbot_amd import nets, sim as fsim
    from flingbot_amd.env import BatchedFlingEnv

    ctx = fsim.FlingSim(n_envs=slots, solver=0)
    env = BatchedFlingEnv(ctx, image_dim=128, num_rotations=ROTATIONS, scale_factors=SCALES, episode_length=2, **env_kwargs)
    torch.manual_seed(SEED)
    policy = nets.MaximumValuePolicy(action_primitives=["fling"], num_rotations=ROTATIONS, scale_factors=list(env.scale_factors),
                                     obs_dim=64, pix_grasp_dist=8, pix_drag_dist=8, pix_place_dist=5, rgb_only=True,
                                     depth_only=False, action_expl_prob=0.0, action_expl_decay=1.0, value_expl_prob=0.0,
                                     value_expl_decay=1.0, device="cuda:0")
    return ctx, env, policy


@pytest.fixture(scope="module")
def tasks(gpu_required):
    from flingbot_amd import sim as fsim, tasks as ftasks

    random.seed(SEED); np.random.seed(SEED)
    gen = fsim.FlingSim(n_envs=2, solver=0)
    made = ftasks.generate_tasks(gen, [ftasks.draw_task_parameters(min_cloth_size=24, strict_min_edge_length=24, max_cloth_size=32)
                                       for _ in range(2)])
    gen.close()
    assert all(t is not None for t in made)
    return made


def _sampled(tasks, seed, follow="policy", **kwargs):
    from flingbot_amd import lookahead

    env_kwargs = dict(record_experience=True) if kwargs.pop("record", False) else {}
    ctx, env, policy = _env_policy(2 * K, **env_kwargs)
    try:
        return lookahead.run_episodes(policy, env, tasks, K, follow=follow, seed=seed, lanes="sampled", **kwargs)
    finally:
        ctx.close()


def _lanes(stats, field):
    return [[[c[field] for c in s["candidates"]] for s in steps] for steps in stats["lookahead"]["steps"]]


@pytest.fixture(scope="module")
def sampled_run(tasks):
    """One sampled run that every test below reads (recorded, so that the dump can be checked too)."""
    return _sampled(tasks, 7, lane_temperature=0.05, lane_separation=2, record=True)


def test_follow_policy_still_equals_run_episodes(gpu_required, tasks, sampled_run):
    from flingbot_amd import evaluate

    ctx, env, policy = _env_policy(2)
    want = evaluate.run_episodes(policy, env, tasks, seed=7)
    ctx.close()
    got = sampled_run
    assert np.array_equal(got["coverage_steps"], want["coverage_steps"])
    assert np.array_equal(got["episode_length"], want["episode_length"])
    assert [r["actions"] for r in got["records"]] == [r["actions"] for r in want["records"]]
    assert [r["coverage"] for r in got["records"]] == [r["coverage"] for r in want["records"]]
    assert got["action_primitive_counts"] == want["action_primitive_counts"]
    for key in ("init_coverage", "final_coverage", "best_coverage", "episode_delta_coverage", "delta_coverage_steps"):
        assert np.array_equal(got[key], want[key]), key
    look = got["lookahead"]
    assert look["lanes"] == "sampled" and look["lane_temperature"] == 0.05 and look["refused"] >= 0
    executed = [len(s["candidates"]) for steps in look["steps"] for s in steps]
    assert max(executed) == K, "a run that never executed every lane shows nothing"
    assert all(s["followed_rank"] == 0 for steps in look["steps"] for s in steps)
    for steps in look["steps"]:
        for s in steps:
            cands = s["candidates"]
            assert all("sample_key" in c for c in cands)
            if cands:   # lane 0 is the arg-max: no lane has a higher value, and its key is its value
                assert cands[0]["value"] == max(c["value"] for c in cands) and cands[0]["sample_key"] == cands[0]["value"]
            assert len({(c["transform_index"], *c["pixel"]) for c in cands}) == len(cands)


def test_same_seed_same_lanes_other_seed_other_lanes(gpu_required, tasks, sampled_run):
    again = _sampled(tasks, 7, lane_temperature=0.05, lane_separation=2)
    for field in ("flat_index", "value", "sample_key", "reward"):
        assert _lanes(again, field) == _lanes(sampled_run, field), field
    assert np.array_equal(again["coverage_steps"], sampled_run["coverage_steps"])
    other = _sampled(tasks, 8, lane_temperature=0.05, lane_separation=2)
    assert _lanes(other, "flat_index") != _lanes(sampled_run, "flat_index")


def test_uniform_draw_does_not_follow_the_values(gpu_required, tasks):
    """All three lanes drawn (sample_first): a step's values are in descending order with probability 1 / 6, four steps with
    (1 / 6)^4 -- with lane 0 greedy it would be 1 / 2 per step, and one seed in sixteen would show nothing."""
    got = _sampled(tasks, 7, lane_temperature=float("inf"), sample_first=True)
    assert got["lookahead"]["lane_temperature"] == "inf"
    values = [v for per_task in _lanes(got, "value") for v in per_task if len(v) >= 2]
    assert values and any(v != sorted(v, reverse=True) for v in values), "at inf the lanes' values come in no order"


def test_executed_sampled_lanes_grasp_cloth(gpu_required, tasks, sampled_run):
    drawn = [c for steps in sampled_run["lookahead"]["steps"] for s in steps for c in s["candidates"] if c["rank"] > 0]
    assert drawn, "no sampled lane was executed"
    assert all(c["grasp_cloth"] == [True, True] for c in drawn)


def test_dump_is_readable_by_experience_set(gpu_required, tasks, sampled_run, tmp_path):
    from flingbot_amd import lookahead
    from flingbot_amd.replay import ExperienceSet

    n = sum(len(s["candidates"]) for steps in sampled_run["lookahead"]["steps"] for s in steps)
    path = str(tmp_path / "sampled_lanes.npz")
    assert lookahead.save_replay(path, sampled_run, tasks) == n == len(sampled_run["lane_records"])
    ds = ExperienceSet(path, obs_color_jitter=False)
    assert len(ds.keys) == n and ds.n_invalid == 0 and ds.n_without_arrays == 0
    flat = np.array([t["flatten_area"] for t in tasks])
    want = np.array([(r["coverage"][1] - r["coverage"][0]) / flat[r["task"]] for r in sampled_run["lane_records"]]).astype(np.float32)
    assert np.array_equal(ds.labels, want)


def test_explicit_winners_is_the_default(gpu_required, tasks):
    from flingbot_amd import lookahead

    runs = []
    for kwargs in ({}, dict(lanes="winners")):
        ctx, env, policy = _env_policy(2 * K)
        runs.append(lookahead.run_episodes(policy, env, tasks, K, follow="best", seed=7, **kwargs))
        ctx.close()
    a, b = runs
    assert a["lookahead"] == b["lookahead"] and set(a["lookahead"]) == {"k", "follow", "steps", "regret", "rank0_best_frac",
                                                                      "mean_reward_per_rank", "n_steps", "n_lane_steps"}
    assert np.array_equal(a["coverage_steps"], b["coverage_steps"]) and a["action_primitive_counts"] == b["action_primitive_counts"]
    assert all("sample_key" not in c for steps in a["lookahead"]["steps"] for s in steps for c in s["candidates"])


def test_sampled_needs_a_seed(gpu_required, tasks):
    from flingbot_amd import lookahead

    ctx, env, policy = _env_policy(2 * K)
    try:
        with pytest.raises(ValueError, match="seed"):
            lookahead.run_episodes(policy, env, tasks, K, lanes="sampled")
        with pytest.raises(ValueError, match="lanes"):
            lookahead.run_episodes(policy, env, tasks, K, lanes="best", seed=1)
    finally:
        ctx.close()
