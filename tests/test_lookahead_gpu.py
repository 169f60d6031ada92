"""lookahead.run_episodes end to end: two generated tasks, k = 3 lanes per episode in six slots of one context.
follow="policy" must reproduce evaluate.run_episodes on a fresh two-slot context EXACTLY -- forks and lanes disturb
nothing -- and follow="best" must follow the arg-max of the recorded rewards and leave one lane record per executed
lane-step, readable by replay.ExperienceSet."""
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


def test_follow_policy_equals_run_episodes(gpu_required, tasks):
    from flingbot_amd import evaluate, lookahead

    ctx, env, policy = _env_policy(2)
    want = evaluate.run_episodes(policy, env, tasks)
    ctx.close()
    ctx, env, policy = _env_policy(2 * K)
    got = lookahead.run_episodes(policy, env, tasks, K, follow="policy")
    ctx.close()
    assert all(net._hip is not None for net in policy.value_nets.values())
    assert np.array_equal(got["coverage_steps"], want["coverage_steps"])
    assert np.array_equal(got["episode_length"], want["episode_length"])
    assert [r["actions"] for r in got["records"]] == [r["actions"] for r in want["records"]]
    assert [r["coverage"] for r in got["records"]] == [r["coverage"] for r in want["records"]]
    assert got["action_primitive_counts"] == want["action_primitive_counts"]
    for key in ("init_coverage", "final_coverage", "best_coverage", "episode_delta_coverage", "delta_coverage_steps"):
        assert np.array_equal(got[key], want[key]), key
    look = got["lookahead"]
    executed = [len(s["candidates"]) for steps in look["steps"] for s in steps]
    assert max(executed) >= 2, "a run that never executed a second lane shows nothing"
    assert all(s["followed_rank"] == 0 for steps in look["steps"] for s in steps)
    assert got["simulation_steps"] > want["simulation_steps"]            # the lanes' steps are counted too
    assert "lane_records" not in got


def test_follow_best_records_every_lane(gpu_required, tasks, tmp_path):
    from flingbot_amd import lookahead
    from flingbot_amd.replay import ExperienceSet

    ctx, env, policy = _env_policy(2 * K, record_experience=True)
    got = lookahead.run_episodes(policy, env, tasks, K, follow="best")
    flat = np.array([t["flatten_area"] for t in tasks])
    trunks_cover = got["final_coverage"]
    look = got["lookahead"]
    assert look["k"] == K and look["follow"] == "best" and len(look["steps"]) == 2
    n_lane_steps = 0
    for i, steps in enumerate(look["steps"]):
        assert len(steps) == got["episode_length"][i]
        for s, entry in enumerate(steps):
            cands = entry["candidates"]
            assert 0 <= len(cands) <= K and [c["rank"] for c in cands] == list(range(len(cands)))
            n_lane_steps += len(cands)
            if not cands:
                assert entry["followed_rank"] == 0
                continue
            rewards = [c["reward"] for c in cands]
            assert entry["followed_rank"] == int(np.argmax(rewards))     # np.argmax: the first of equal maxima
            assert got["records"][i]["rewards"][s] == rewards[entry["followed_rank"]]
            keys = [(-c["value"], c["flat_index"]) for c in cands]
            assert keys == sorted(keys) and len({(c["transform_index"], *c["pixel"]) for c in cands}) == len(cands)
            assert all(c["primitive"] == "fling" and 0 <= c["transform_index"] < ROTATIONS * len(SCALES) for c in cands)
    executed = [len(s["candidates"]) for steps in look["steps"] for s in steps]
    assert max(executed) >= 2, "a run that never executed a second lane shows nothing"
    assert look["regret"] >= 0 and 0 <= look["rank0_best_frac"] <= 1 and look["n_lane_steps"] == n_lane_steps
    assert len(look["mean_reward_per_rank"]) == K
    # the followed trajectory is what the simulator holds now: the final coverage is some slot's of the task's group
    cov = np.array(ctx.coverage())
    for i, group in enumerate(lookahead.group_slots(2 * K, K)):
        assert trunks_cover[i] in cov[group] / flat[i]
    ctx.close()
    # one record per executed lane-step, with the arrays of ITS candidate
    recs = got["lane_records"]
    assert len(recs) == n_lane_steps
    for r in recs:
        entry = look["steps"][r["task"]][r["step"]]["candidates"][r["rank"]]
        assert r["rewards"] == [entry["reward"]] and r["coverage"][1] - r["coverage"][0] == entry["reward"]
        y, z = entry["pixel"]
        assert r["experience"][0]["actions"][y, z] and r["experience"][0]["actions"].sum() == 1
        assert int(r["experience"][0]["max_indices"][0]) == entry["transform_index"]
    same_state = [r["coverage"][0] for r in recs if r["task"] == 0 and r["step"] == 0]
    assert len(set(same_state)) == 1                                    # K labels from ONE identical state
    path = str(tmp_path / "lanes.npz")
    assert lookahead.save_replay(path, got, tasks) == n_lane_steps
    ds = ExperienceSet(path, obs_color_jitter=False)
    assert len(ds.keys) == n_lane_steps and ds.n_invalid == 0 and ds.n_without_arrays == 0
    want = np.array([(r["coverage"][1] - r["coverage"][0]) / flat[r["task"]] for r in recs]).astype(np.float32)
    assert np.array_equal(ds.labels, want)
