"""Evaluation and training on task sets that mix quad-mesh shirts with grid cloths: BatchedFlingEnv, evaluate.run_episodes /
run_tasks and train.run on six tasks -- shirt A twice, shirt B twice (tests/golden/mesh_task_golden.npz) and two small grids
(tests/golden/task_golden.npz), interleaved -- on fewer slots than tasks, so that a slot's cloth changes kind (and particle
count, adjacency form and rest-pose filter form) from one episode to the next."""
import os

import numpy as np
import pytest
import torch

from mesh_task_helpers import GOLD, golden

pytestmark = pytest.mark.gpu

_MESH_FIELDS = ("mesh_verts", "mesh_stretch_edges", "mesh_bend_edges", "mesh_shear_edges", "mesh_faces")
_REF = {}


def mixed_tasks():
    """[shirt A, grid, shirt B (hard), grid, shirt A, shirt B (easy)] as generator dictionaries, straight from the fixtures."""
    g, gg = golden(), np.load(os.path.join(GOLD, "task_golden.npz"))

    def mesh(ci):
        t = {k: g[f"c{ci}_{k}"] for k in ("particle_pos", "particle_vel", "shape_pos", "phase", "cloth_size", "cloth_stiff") + _MESH_FIELDS}
        t.update({k: float(g[f"c{ci}_{k}"]) for k in ("flatten_area", "initial_coverage", "cloth_mass")})
        t.update(flip_mesh=0, task_difficulty=str(g[f"c{ci}_task_difficulty"]))
        return t

    def grid(ti):
        t = {k: gg[f"t{ti}_{k}"] for k in ("particle_pos", "particle_vel", "shape_pos", "phase", "cloth_size", "cloth_stiff")}
        t.update({k: float(gg[f"t{ti}_{k}"]) for k in ("flatten_area", "initial_coverage", "cloth_mass")})
        t.update(flip_mesh=0, task_difficulty=str(gg[f"t{ti}_difficulty"]), **{k: np.array([]) for k in _MESH_FIELDS})
        return t

    kinds = {ci: (str(g[f"c{ci}_mesh"]), str(g[f"c{ci}_difficulty"])) for ci in range(int(g["n_cases"]))}
    a = [ci for ci, k in kinds.items() if k[0] == "a"]
    b_hard = [ci for ci, k in kinds.items() if k == ("b", "hard")][0]
    b_easy = [ci for ci, k in kinds.items() if k == ("b", "easy")][0]
    tasks = [mesh(a[0]), grid(0), mesh(b_hard), grid(1), mesh(a[1]), mesh(b_easy)]
    assert [len(t["mesh_verts"]) > 0 for t in tasks] == [True, False, True, False, True, True]
    return tasks


def _policy(env, seed=1, **explore):
    from flingbot_amd import nets

    torch.manual_seed(seed)
    kw = dict(action_expl_prob=0.0, action_expl_decay=1.0, value_expl_prob=0.0, value_expl_decay=1.0)
    kw.update(explore)
    return nets.MaximumValuePolicy(action_primitives=list(env.actions), num_rotations=12, scale_factors=list(env.scale_factors),
                                   obs_dim=64, pix_grasp_dist=8, pix_drag_dist=8, pix_place_dist=5, rgb_only=True,
                                   depth_only=False, device="cuda:0", **kw)


def _env(slots):
    from flingbot_amd import sim as fsim
    from flingbot_amd.env import BatchedFlingEnv

    ctx = fsim.FlingSim(n_envs=slots, solver=0)
    return ctx, BatchedFlingEnv(ctx, image_dim=128, episode_length=2, record_experience=True)


def alone_records():
    """Every task run on its own in a fresh one-slot context: the reference the shared-slot runs are compared with (made once)."""
    from flingbot_amd.evaluate import run_tasks

    if "records" not in _REF:
        tasks, records = mixed_tasks(), []
        for t in tasks:
            ctx, env = _env(1)
            stats = run_tasks(_policy(env), env, [t])
            assert ctx.n_particles(0) == len(t["particle_pos"]) // 4
            ctx.close()
            records.append(stats["records"][0])
        assert sum(len(r["actions"]) for r in records) >= len(tasks) and any(a == "fling" for r in records for a in r["actions"])
        _REF["records"] = records
    return _REF["records"]


def assert_same_record(got, want, what):
    assert got["actions"] == want["actions"], what
    for k in ("coverage", "rewards", "preaction_coverage"):
        assert np.array_equal(np.array(got[k], np.float64).view(np.uint64), np.array(want[k], np.float64).view(np.uint64)), (what, k)
    assert len(got["experience"]) == len(want["experience"]) == len(want["actions"])
    for k, (x, y) in enumerate(zip(got["experience"], want["experience"])):
        assert (x is None) == (y is None), (what, k)
        if x is not None:
            assert set(x) == set(y)
            for f in x:
                xa, ya = np.asarray(x[f]), np.asarray(y[f])
                assert xa.dtype == ya.dtype and xa.shape == ya.shape and xa.tobytes() == ya.tobytes(), (what, k, f)


def test_lockstep_loop_on_shared_slots_equals_tasks_alone(gpu_required):
    """run_episodes, two tasks at a time on ONE two-slot context: slot 1 holds grid, grid, then a mesh; slot 0 three meshes of
    different sizes."""
    from flingbot_amd.evaluate import run_episodes

    tasks, want = mixed_tasks(), alone_records()
    ctx, env = _env(2)
    policy = _policy(env)
    for first in range(0, len(tasks), 2):
        stats = run_episodes(policy, env, tasks[first:first + 2])
        for k, rec in enumerate(stats["records"]):
            assert ctx.n_particles(k) == len(tasks[first + k]["particle_pos"]) // 4
            assert_same_record(rec, want[first + k], f"lock-step, task {first + k}")
            steps = len(rec["actions"])
            flat = tasks[first + k]["flatten_area"]
            assert np.array_equal(stats["coverage_steps"][:steps + 1, k], np.array(rec["coverage"]) / flat)
    ctx.close()


@pytest.mark.parametrize("slots,kwargs", [(2, {}), (1, {}), (2, dict(pipeline=False, prebuild=False))])
def test_continuous_loop_on_shared_slots_equals_tasks_alone(gpu_required, slots, kwargs):
    """run_tasks on fewer slots than tasks (pipelined with prebuilt scenes, and the blocking scheduler with scenes built in
    place).  One slot runs the whole set in order: mesh -> grid -> mesh -> grid -> mesh -> mesh, i.e. grid -> mesh -> grid."""
    from flingbot_amd.evaluate import run_tasks

    tasks, want = mixed_tasks(), alone_records()
    ctx, env = _env(slots)
    stats = run_tasks(_policy(env), env, tasks, **kwargs)
    assert ctx.advance_in_flight() == 0 and stats["task_indices"].tolist() == list(range(len(tasks)))
    ctx.close()
    flat = np.array([t["flatten_area"] for t in tasks])
    for i, rec in enumerate(stats["records"]):
        assert_same_record(rec, want[i], f"continuous, {slots} slot(s), task {i}")
        steps = len(rec["actions"])
        assert int(stats["episode_length"][i]) == steps
        assert np.array_equal(stats["coverage_steps"][:steps + 1, i], np.array(rec["coverage"]) / flat[i])
    assert np.isfinite(stats["final_coverage"]).all()


@pytest.mark.parametrize("hip_step", [False, True])
def test_train_round_on_mixed_set(gpu_required, tmp_path, hip_step):
    """One round of train.run on the six tasks over two slots with exploration on: it finishes, makes exactly one update per
    primitive, writes a replay file whose episodes carry the task's own flatten_area as max_coverage (the shirts' is the drawn
    mesh_flatten_area), and a second run from scratch with the same seed leaves identical files."""
    from flingbot_amd import taskio, train

    tasks = mixed_tasks()
    logs = [str(tmp_path / "a"), str(tmp_path / "b")]
    outs = []
    for log_dir in logs:
        ctx, env = _env(2)
        try:
            policy = _policy(env, seed=7, action_expl_prob=0.5, action_expl_decay=0.9, value_expl_prob=0.5, value_expl_decay=0.9)
            opt = train.make_optimizer(policy, hip=hip_step)
            outs.append(train.run(policy, opt, env, tasks, log_dir, rounds=1, tasks_per_round=len(tasks), seed=3, batch_size=2,
                                  warmup=2, update_frequency=10 ** 6, hip_step=hip_step))
            steps = int(policy.steps())
        finally:
            ctx.close()
        row = outs[-1]["rounds"][0]
        assert row["new_entries"] > 2 and row["updates"] == len(policy.value_nets) == 1 and steps >= 1 and np.isfinite(row["mean_loss"])
    assert outs[0]["rounds"][0]["new_entries"] == outs[1]["rounds"][0]["new_entries"]
    files = []
    for log_dir in logs:
        assert [os.path.basename(p) for p in train.replay_files(log_dir)] == ["replay_00000.npz"]
        z = np.load(train.replay_files(log_dir)[0], allow_pickle=False)
        files.append({k: z[k] for k in z.files})
    a, b = files
    assert set(a) == set(b) and any(k.endswith("/observations") for k in a)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
    # percent coverage = coverage / flatten_area, per episode with the task's own area
    finals = []
    for key in (str(k) for k in a["keys"]):
        ep = int(key.split("_")[0])
        assert float(a[f"{key}/max_coverage"]) == tasks[ep]["flatten_area"]
        assert float(a[f"{key}/init_coverage"]) == tasks[ep]["initial_coverage"]
        if key.endswith("_last"):
            finals.append(float(a[f"{key}/postaction_coverage"]) / tasks[ep]["flatten_area"])
    assert {int(str(k).split("_")[0]) for k in a["keys"]} == set(range(len(tasks)))
    stats = taskio.collect_stats(train.replay_files(logs[0])[0], num_points=10 ** 6)
    got = np.concatenate([stats.get(f"final_coverage/{level}/distribution", np.zeros(0)) for level in ("easy", "hard")])
    assert len(finals) == len(tasks) and np.array_equal(np.sort(got), np.sort([f for f in finals if f >= 0.05]))


def test_filmed_mesh_episode(gpu_required, tmp_path):
    """--dump-visualizations on a slot that runs a grid and then a shirt: both episodes are filmed from the top camera during
    movep and leave <root>/<task>/top.png; the replay file names the directory next to the shirt's own flatten_area."""
    from PIL import Image

    from flingbot_amd import sim as fsim, taskio
    from flingbot_amd.env import BatchedFlingEnv
    from flingbot_amd.evaluate import run_tasks

    tasks = mixed_tasks()[1:3] + mixed_tasks()[4:5]            # grid, shirt B, shirt A
    ctx = fsim.FlingSim(n_envs=1, solver=0)
    env = BatchedFlingEnv(ctx, image_dim=128, episode_length=1, dump_visualizations=True, frame_size=(64, 64),
                          visualization_root=str(tmp_path / "films"))
    stats = run_tasks(_policy(env), env, tasks)
    assert ctx.advance_in_flight() == 0 and all(ctx.capture_count(e) == 0 for e in range(1))
    ctx.close()
    assert len(stats["records"]) == 3
    filmed = [i for i, rec in enumerate(stats["records"]) if rec["actions"] == ["fling"]]
    assert any(i > 0 for i in filmed)          # a shirt among them (an episode without a valid action moves nothing: no film)
    for i in filmed:
        rec = stats["records"][i]
        film = os.path.join(rec["visualization_dir"], "top.png")
        assert os.path.dirname(rec["visualization_dir"]) == str(tmp_path / "films") and os.path.exists(film)
        with Image.open(film) as im:
            assert im.size == (64, 64) and im.n_frames > 10, (i, im.n_frames)
            im.seek(im.n_frames // 2)
            frame = np.asarray(im.convert("RGB"))
        assert frame.std() > 0            # something is in the picture
    assert len({stats["records"][i]["visualization_dir"] for i in filmed}) == len(filmed)
    path = str(tmp_path / "replay.npz")
    taskio.save_replay(path, stats["records"], tasks)
    z = np.load(path, allow_pickle=False)
    for i, key in enumerate(str(k) for k in z["keys"]):      # one action per episode: entry i is episode i
        if i in filmed:
            assert str(z[f"{key}/visualization_dir"]) == stats["records"][i]["visualization_dir"]
        assert float(z[f"{key}/max_coverage"]) == tasks[i]["flatten_area"]
