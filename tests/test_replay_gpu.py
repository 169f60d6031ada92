"""fs_replay_sample (csrc/fs_replay.hip) through replay.ExperienceSet.sample against the host chain bit for bit, and the
collection of experience through both evaluation loops."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D = 64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jitter_golden.npz")
TASK = {"cloth_mass": 0.5, "flatten_area": 2.0, "task_difficulty": "hard", "initial_coverage": 0.5}


def _write_set(path, observations, rng):
    """A replay file whose entries carry `observations` [N, 4, D, D], one mask pixel and one reward each."""
    from flingbot_amd import taskio

    records = []
    for k, obs in enumerate(observations):
        mask = np.zeros((D, D), bool)
        y, z = int(rng.integers(D)), int(rng.integers(D))
        mask[y, z] = True
        pre, post = float(rng.random()), float(rng.random())
        records.append(dict(coverage=[pre, post], actions=["fling"], rewards=[post - pre], preaction_coverage=[pre],
                            experience=[dict(observations=obs, actions=mask, value_map=np.zeros((D, D), np.float32),
                                             max_indices=np.array([k % 7, y, z]), rotation=0.0, scale=1.0)]))
    taskio.save_replay(path, records, [TASK] * len(records))


def _observations(rng, n):
    """Recorded stacks the way prepare_image leaves them: colours mostly inside [0, 1] with some overshoot on both sides,
    exact 0 / 1 runs, a flat and a near-gray image; depth around 2."""
    obs = rng.random((n, 4, D, D), dtype=np.float32)
    obs[:, :3] = obs[:, :3] * np.float32(1.1) - np.float32(0.05)
    obs[:, 3] = np.float32(1.9) + np.float32(0.1) * obs[:, 3]
    obs[0, :3] = np.float32(0.18)
    obs[1, :3] = np.float32(0.4) + (rng.random((3, D, D), dtype=np.float32) - np.float32(0.5)) * np.float32(0.01)
    obs[2, :3, :8] = 0.0
    obs[2, :3, 8:16] = 1.0
    obs[2, 0, 16:24] = 1.0
    return obs


@pytest.mark.parametrize("batch", [1, 7, 128])
@pytest.mark.parametrize("mode", ["rgb_jitter", "rgb_plain", "depth_only", "four_channel"])
def test_sample_is_bit_identical_to_the_host_chain(gpu_required, tmp_path, batch, mode):
    from flingbot_amd import replay

    rng = np.random.default_rng(100 + batch)
    path = str(tmp_path / "set.npz")
    _write_set(path, _observations(rng, 37), rng)
    kwargs = dict(rgb_jitter=dict(), rgb_plain=dict(obs_color_jitter=False), depth_only=dict(rgb_only=False, depth_only=True),
                  four_channel=dict(rgb_only=False))[mode]
    data = replay.ExperienceSet(path, **kwargs).to_device("cuda:0")
    assert len(data) == 37 and data.jitters == (mode == "rgb_jitter")
    channels = dict(rgb_jitter=3, rgb_plain=3, depth_only=1, four_channel=4)[mode]
    for seed in (1, 2):
        # sample() draws on the host from rng: the same rng state gives the indices and parameters it used
        idx, params = data.draw(batch, np.random.default_rng(seed))
        obs, mask, label = data.sample(batch, np.random.default_rng(seed))
        assert obs.is_cuda and mask.is_cuda and label.is_cuda
        assert obs.dtype == torch.float32 and tuple(obs.shape) == (batch, channels, D, D)
        assert mask.dtype == torch.bool and tuple(mask.shape) == (batch, D, D)
        assert label.dtype == torch.float32 and tuple(label.shape) == (batch,)
        want_obs, want_mask, want_label = data.item_host(idx, params)
        got = obs.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want_obs.view(np.uint32)), \
            f"{int((got != want_obs).sum())} of {got.size} values differ, max {np.abs(got - want_obs).max():.3e}"
        assert np.array_equal(mask.cpu().numpy(), want_mask) and (mask.sum(dim=(1, 2)) == 1).all()
        assert np.array_equal(label.cpu().numpy().view(np.uint32), want_label.view(np.uint32))
        if mode != "rgb_jitter":    # the recorded floats, unchanged (overshoot and all)
            off, cnt = data.channels
            assert np.array_equal(got.view(np.uint32), data.observations[idx, off:off + cnt].view(np.uint32))
        else:
            assert params is not None and not np.array_equal(got, data.observations[idx, :3])


def test_fixture_cases_through_the_kernel(gpu_required, tmp_path):
    """The Pillow outputs of tests/golden/jitter_golden.npz, produced by the kernel."""
    from flingbot_amd import replay

    z = np.load(GOLDEN, allow_pickle=False)
    imgs, index, want = z["images"], z["image_index"], z["outputs"]
    rgb = ((imgs.astype(np.float32) + np.float32(0.5)) / np.float32(255.0)).transpose(0, 3, 1, 2)   # quantises back to imgs
    obs = np.concatenate([rgb, np.full((len(imgs), 1, D, D), 2.0, np.float32)], axis=1)
    path = str(tmp_path / "fixture.npz")
    _write_set(path, obs, np.random.default_rng(0))
    data = replay.ExperienceSet(path).to_device("cuda:0")
    got, _, _ = data.gather(index, {"order": z["order"], "factors": z["factors"]})
    got = got.cpu().numpy()
    for k in range(len(want)):
        assert np.array_equal(got[k], want[k].transpose(2, 0, 1).astype(np.float32) / np.float32(255.0)), (k, z["order"][k], z["factors"][k])


def test_sample_refuses_what_it_does_not_serve(gpu_required, tmp_path):
    from flingbot_amd import replay, taskio

    rng = np.random.default_rng(5)
    path = str(tmp_path / "set.npz")
    _write_set(path, _observations(rng, 4), rng)
    data = replay.ExperienceSet(path).to_device("cuda:0")
    with pytest.raises(IndexError):
        data.gather([0, 4])
    with pytest.raises(ValueError):
        data.gather([0, 1], replay.draw_jitter(rng, 3))
    small = dict(coverage=[0.1, 0.2], actions=["fling"], rewards=[0.1], preaction_coverage=[0.1],
                 experience=[dict(observations=np.zeros((4, 32, 32), np.float32), actions=np.eye(32, dtype=bool) & (np.arange(32) == 3),
                                  value_map=np.zeros((32, 32), np.float32), max_indices=np.array([0, 3, 3]), rotation=0.0, scale=1.0)])
    taskio.save_replay(str(tmp_path / "small.npz"), [small], [TASK])
    other = replay.ExperienceSet(str(tmp_path / "small.npz"))
    assert len(other) == 1
    with pytest.raises(ValueError):
        other.to_device("cuda:0")           # D = 64 only


def _records_equal(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert set(ra) == set(rb), (set(ra), set(rb))
        for key in ra:
            if key != "experience":
                assert ra[key] == rb[key], (key, ra[key], rb[key])
                continue
            assert len(ra[key]) == len(rb[key]) == len(ra["actions"])
            for xa, xb in zip(ra[key], rb[key]):
                assert (xa is None) == (xb is None)
                if xa is None:
                    continue
                assert set(xa) == set(xb)
                for name in xa:
                    va, vb = np.asarray(xa[name]), np.asarray(xb[name])
                    assert va.dtype == vb.dtype and va.shape == vb.shape and np.array_equal(va, vb), name


def test_collection_is_identical_through_both_loops(gpu_required, tmp_path):
    """Three small generated tasks, two actions each, exploration on at fixed probabilities under seed 3: run_tasks in 2
    slots, run_tasks in 3 slots and run_episodes leave identical records, arrays included; each recorded observation is
    entry max_indices[0] of the stack that produced it, the mask pixel is max_indices[1:]; and with both probabilities 0 and
    no recording the records have the parent's keys."""
    import random

    from flingbot_amd import nets, replay, sim as fsim, taskio, tasks as ftasks
    from flingbot_amd.env import BatchedFlingEnv
    from flingbot_amd.evaluate import run_episodes, run_tasks

    random.seed(1); np.random.seed(1); torch.manual_seed(1)
    n = 3
    gen = fsim.FlingSim(n_envs=n, solver=0)
    tasks = ftasks.generate_tasks(gen, [ftasks.draw_task_parameters(min_cloth_size=24, strict_min_edge_length=24, max_cloth_size=32) for _ in range(n)])
    gen.close()

    def policy_with(action_prob, value_prob, env):
        torch.manual_seed(7)
        return nets.MaximumValuePolicy(action_primitives=["fling"], num_rotations=12, scale_factors=list(env.scale_factors),
                                       obs_dim=64, pix_grasp_dist=8, pix_drag_dist=8, pix_place_dist=5, rgb_only=True,
                                       depth_only=False, action_expl_prob=action_prob, action_expl_decay=1.0,
                                       value_expl_prob=value_prob, value_expl_decay=1.0, device="cuda:0")

    runs, seen = [], []
    for slots, loop in ((2, run_tasks), (3, run_tasks), (3, run_episodes)):
        ctx = fsim.FlingSim(n_envs=slots, solver=0)
        env = BatchedFlingEnv(ctx, image_dim=128, episode_length=2, record_experience=True)
        policy = policy_with(0.5, 0.5, env)
        if loop is run_episodes:
            # keep every stack the policy saw, to check the recorded observations against
            act = policy.act

            def spying_act(obs, keep_on_device=False, keys=None):
                seen.extend((key, o.clone()) for key, o in zip(keys, obs))
                return act(obs, keep_on_device=keep_on_device, keys=keys)
            policy.act = spying_act
        stats = loop(policy, env, tasks, seed=3)
        assert all(net._hip is not None for net in policy.value_nets.values())
        runs.append(stats["records"])
        ctx.close()
    _records_equal(runs[0], runs[1])
    _records_equal(runs[0], runs[2])
    stacks = {key: o for key, o in seen}
    recorded = 0
    for ti, rec in enumerate(runs[2]):
        assert len(rec["experience"]) == len(rec["actions"]) >= 1
        for step, (action, arrays) in enumerate(zip(rec["actions"], rec["experience"])):
            assert (arrays is None) == (action is None)
            if arrays is None:
                continue
            recorded += 1
            x, y, z = (int(v) for v in arrays["max_indices"])
            assert arrays["observations"].dtype == np.float32 and arrays["observations"].shape == (4, 64, 64)
            assert np.array_equal(arrays["observations"], stacks[(3, ti, step)][x].cpu().numpy())
            assert arrays["actions"].dtype == bool and arrays["actions"].sum() == 1 and arrays["actions"][y, z]
            assert arrays["value_map"].dtype == np.float32 and arrays["value_map"].shape == (64, 64)
            assert 8 <= y < 56 and 8 <= z < 56 and 0 <= x < 96     # inside pix_grasp_dist, one of 12 x 8 transforms
    assert recorded >= 3
    # the file, and the set it becomes
    path = str(tmp_path / "collected.npz")
    taskio.save_replay(path, runs[0], tasks)
    data = replay.ExperienceSet(path, action_primitive="fling").to_device("cuda:0")
    assert len(data) == recorded and data.n_invalid == 0
    obs, mask, label = data.sample(8, np.random.default_rng(0))
    assert tuple(obs.shape) == (8, 3, 64, 64) and bool((mask.sum(dim=(1, 2)) == 1).all()) and bool(torch.isfinite(label).all())

    # both probabilities 0, no recording: the parent's record format, key for key, and seeded or not makes no difference
    plain = []
    for seed in (None, 3):
        ctx = fsim.FlingSim(n_envs=2, solver=0)
        env = BatchedFlingEnv(ctx, image_dim=128, episode_length=2)
        plain.append(run_tasks(policy_with(0.0, 0.0, env), env, tasks, **({} if seed is None else dict(seed=seed)))["records"])
        ctx.close()
    for rec in plain[0]:
        assert set(rec) == {"coverage", "actions", "rewards", "preaction_coverage"}
    _records_equal(plain[0], plain[1])
