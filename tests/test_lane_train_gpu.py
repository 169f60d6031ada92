"""train.run(lookahead=2, follow="best", hip_step=True): two tasks per round, two rounds, four slots.  One entry per executed
lane-step, the updates plan_round plans, two runs from one seed identical in every replay array and checkpoint tensor, a
resumed third call, and the command line."""
import json
import os
import random
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K, N, SLOTS, WARMUP, BATCH = 2, 2, 4, 2, 4


@pytest.fixture(scope="module")
def tasks(gpu_required):
    from flingbot_amd import sim as fsim, tasks as ftasks

    random.seed(1); np.random.seed(1); torch.manual_seed(1)
    gen = fsim.FlingSim(n_envs=N, solver=0)
    made = ftasks.generate_tasks(gen, [ftasks.draw_task_parameters(min_cloth_size=24, strict_min_edge_length=24, max_cloth_size=32)
                                       for _ in range(N)])
    gen.close()
    assert all(t is not None for t in made)
    return made


def _fresh(env):
    from flingbot_amd import nets, train

    torch.manual_seed(7)
    policy = nets.MaximumValuePolicy(action_primitives=["fling"], num_rotations=12, scale_factors=list(env.scale_factors),
                                     obs_dim=64, pix_grasp_dist=8, pix_drag_dist=8, pix_place_dist=5, rgb_only=True,
                                     depth_only=False, action_expl_prob=0.5, action_expl_decay=0.9, value_expl_prob=0.5,
                                     value_expl_decay=0.9, device=DEV)
    return policy, train.make_optimizer(policy, hip=True)


@pytest.fixture(scope="module")
def lane_runs(tasks, tmp_path_factory):
    """Two runs of two rounds from scratch with one seed, then a third call that resumes the first run's directory."""
    from flingbot_amd import sim as fsim, train
    from flingbot_amd.env import BatchedFlingEnv

    base = tmp_path_factory.mktemp("lane_train")
    logs = [str(base / "a"), str(base / "b")]
    outs, steps = [], []
    ctx = fsim.FlingSim(n_envs=SLOTS, solver=0)
    try:
        env = BatchedFlingEnv(ctx, image_dim=128, episode_length=2, record_experience=True)
        for log_dir in logs:
            policy, opt = _fresh(env)
            outs.append(train.run(policy, opt, env, tasks, log_dir, rounds=2, tasks_per_round=N, seed=3, batch_size=BATCH,
                                  warmup=WARMUP, hip_step=True, lookahead=K, follow="best"))
            steps.append(int(policy.steps()))
        shutil.copy(os.path.join(logs[0], train.LATEST), str(base / "a_after_two_rounds.pth"))   # (the third call rewrites it)
        policy, opt = _fresh(env)
        resumed = train.run(policy, opt, env, tasks, logs[0], rounds=1, tasks_per_round=N, seed=3, batch_size=BATCH,
                            warmup=WARMUP, hip_step=True, lookahead=K, follow="best")
        with pytest.raises(ValueError, match="lookahead"):
            train.run(policy, opt, env, tasks, logs[1], rounds=1, tasks_per_round=N, seed=3, lookahead=SLOTS + 1)
        with pytest.raises(ValueError, match="lookahead"):
            train.run(policy, opt, env, tasks, logs[1], rounds=1, tasks_per_round=N, seed=3, lookahead=0)
    finally:
        ctx.close()
    return dict(logs=logs, outs=outs, steps=steps, resumed=resumed, after_two=str(base / "a_after_two_rounds.pth"))


def test_entries_and_updates_are_the_lane_steps(lane_runs):
    from flingbot_amd import train

    out, log_dir = lane_runs["outs"][0], lane_runs["logs"][0]
    files = train.replay_files(log_dir)
    assert [os.path.basename(p) for p in files[:2]] == ["replay_00000.npz", "replay_00001.npz"]
    before, updates = 0, 0
    for row, path in zip(out["rounds"], files):
        z = np.load(path, allow_pickle=False)
        keys = [str(k) for k in z["keys"]]
        look = row["lookahead"]
        assert set(look) == {"k", "follow", "regret", "rank0_best_frac", "mean_reward_per_rank", "n_steps", "n_lane_steps"}
        assert look["k"] == K and look["follow"] == "best" and look["regret"] >= 0 and len(look["mean_reward_per_rank"]) == K
        assert len(keys) == look["n_lane_steps"] == row["new_entries"] and look["n_lane_steps"] >= look["n_steps"] > 0
        assert keys == [f"{before + t:09d}_step00_last" for t in range(len(keys))]           # keys count on over the rounds
        ranks = [int(z[f"{k}/lane_rank"]) for k in keys]
        assert ranks.count(0) == look["n_steps"] and set(ranks) <= set(range(K))
        # one followed lane per step and task
        where = [(int(z[f"{k}/lane_task"]), int(z[f"{k}/lane_step"])) for k in keys]
        followed = [int(z[f"{k}/lane_followed"]) for k in keys]
        assert sum(followed) == len(set(where)) == look["n_steps"]
        plan = train.plan_round(before, ranks, WARMUP, 1, 512)
        # every planned update ran one batch per primitive -- once the set holds a batch
        sizes = [before + len(keys)] * len(keys)
        want = sum(1 for (_, update, _), size in zip(plan, sizes) if update and size >= BATCH)
        assert row["updates"] == want
        updates += want
        before += len(keys)
        assert row["entries"] == before
    assert lane_runs["steps"][0] == updates and updates > 0
    assert sum(r["lookahead"]["n_lane_steps"] for r in out["rounds"]) > sum(r["lookahead"]["n_steps"] for r in out["rounds"]), \
        "a run that never executed a second lane shows nothing"
    lines = [json.loads(line) for line in open(os.path.join(log_dir, train.TRAIN_LOG))]
    rounds = [line for line in lines if "lookahead" in line]
    assert [line["round"] for line in rounds] == [0, 1, 2] and rounds[0]["lookahead"] == out["rounds"][0]["lookahead"]


def test_two_runs_from_one_seed_are_identical(lane_runs):
    from flingbot_amd import train

    logs = lane_runs["logs"]
    for name in ("replay_00000.npz", "replay_00001.npz"):
        a, b = (np.load(os.path.join(d, name), allow_pickle=False) for d in logs)
        assert set(a.files) == set(b.files) and len(a["keys"]) > 0
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (name, k)
    assert lane_runs["steps"][0] == lane_runs["steps"][1]
    # the checkpoints after two rounds (the first run's was set aside before its third round), and every numbered one
    names = sorted(f for f in os.listdir(logs[1]) if f.startswith("ckpt_"))
    assert names and all(os.path.exists(os.path.join(logs[0], f)) for f in names)
    pairs = [(lane_runs["after_two"], os.path.join(logs[1], train.LATEST))] + [tuple(os.path.join(d, f) for d in logs) for f in names]
    for f, (pa, pb) in zip(["after two rounds"] + names, pairs):
        ca, cb = torch.load(pa, map_location="cpu"), torch.load(pb, map_location="cpu")
        assert len(ca["optimizer"]["state"]) > 0
        for k, v in ca["net"].items():
            assert torch.equal(v, cb["net"][k]), (f, k)
        sa, sb = ca["optimizer"]["state"], cb["optimizer"]["state"]
        assert list(sa) == list(sb)
        for k in sa:
            for part in sa[k]:
                assert torch.equal(sa[k][part], sb[k][part]), (f, k, part)
    assert [r["lookahead"] for r in lane_runs["outs"][0]["rounds"]] == [r["lookahead"] for r in lane_runs["outs"][1]["rounds"]]


def test_third_call_resumes_at_round_two(lane_runs):
    from flingbot_amd import train

    resumed, log_dir = lane_runs["resumed"], lane_runs["logs"][0]
    files = train.replay_files(log_dir)
    assert resumed["first_round"] == 2 and [r["round"] for r in resumed["rounds"]] == [2] and len(files) == 3
    sizes = [len(np.load(p, allow_pickle=False)["keys"]) for p in files]
    assert resumed["rounds"][0]["entries"] == sum(sizes) and resumed["rounds"][0]["new_entries"] == sizes[2]
    first = str(np.load(files[2], allow_pickle=False)["keys"][0])
    assert first == f"{sizes[0] + sizes[1]:09d}_step00_last"


def test_command_line(tasks, tmp_path, capsys):
    from flingbot_amd import taskio, train

    path = str(tmp_path / "tasks.npz")
    taskio.save_tasks(path, tasks)
    log_dir = str(tmp_path / "run")
    # refused before the GPU is touched: the parser's own error
    with pytest.raises(SystemExit) as err:
        train.main(["--log", log_dir, "--tasks", path, "--lookahead", "3", "--slots", "2"])
    assert err.value.code == 2 and "--slots" in capsys.readouterr().err and not os.path.exists(log_dir)
    with pytest.raises(SystemExit):
        train.main(["--log", log_dir, "--tasks", path, "--lookahead", "0"])
    capsys.readouterr()
    train.main(["--log", log_dir, "--tasks", path, "--lookahead", "2", "--follow", "best", "--slots", "4", "--tasks-per-round", "2",
                "--rounds", "1", "--episode-length", "1", "--warmup", "1", "--batch_size", "2", "--hip-step",
                "--action_expl_prob", "0.5", "--value_expl_prob", "0.5"])
    row = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert row["round"] == 0 and row["lookahead"]["k"] == 2 and row["lookahead"]["follow"] == "best"
    assert row["new_entries"] == row["lookahead"]["n_lane_steps"] > 0
    assert len(np.load(os.path.join(log_dir, "replay_00000.npz"), allow_pickle=False)["keys"]) == row["new_entries"]
