"""dump_visualizations on the device: frames captured inside the movep launch sequences (fs_capture_*, the capture form
of the rasteriser) are byte for byte the renders of the same states, do not touch the simulation, come out the same from
all three drivers, use a scratch of their own, and the evaluation loop writes them as one animated file per filmed task."""
import os
import random

import numpy as np
import pytest

from fling_helpers import GOLD, picker_centres

pytestmark = pytest.mark.gpu


def _golden():
    return np.load(os.path.join(GOLD, "capture_golden.npz"))


def _params(dx, dz):
    return np.array([0, 0.2, 0, dx, dz, 0.9, 0.9, 0.9, 2, 0, 2, 0, np.pi / 2, -np.pi / 2, 0, 720, 720, 0.3, 0])


def _grid(dx, dz):
    xs = (np.arange(dx) - (dx - 1) / 2) * 0.00625
    zs = (np.arange(dz) - (dz - 1) / 2) * 0.00625
    return xs, zs


def _flat_cloth(ctx, e, dx, dz, pickers=True):
    """A flat dx x dz cloth at rest height in slot e (the fixture's scene for 32 x 32), optionally with the two pickers."""
    env = ctx.env(e)
    env.set_scene(_params(dx, dz))
    env.step(1)
    xs, zs = _grid(dx, dz)
    xx, zz = np.meshgrid(xs, zs)
    pos = np.zeros((dx * dz, 4), np.float32)
    pos[:, 0], pos[:, 1], pos[:, 2], pos[:, 3] = xx.ravel(), 0.0125, zz.ravel(), env.get_positions().reshape(-1, 4)[0, 3]
    env.set_positions(pos.ravel())
    env.set_velocities(np.zeros(3 * dx * dz, np.float32))
    if pickers:
        for c in picker_centres():
            env.add_sphere(0.02, c, [1, 0, 0, 0])
        st = np.array(env.get_shape_states()).reshape(-1, 14)
        for i, c in enumerate(picker_centres()):
            st[i] = np.hstack([c, c, [1, 0, 0, 0], [1, 0, 0, 0]])
        env.set_shape_states(st)
        ctx.picker_reset(e, picker_radius=0.02)


def _flipped_rgb(ctx, e, w, h):
    rgba, _ = ctx.render(e)
    return np.flip(rgba.reshape(h, w, 4), 0)[:, :, :3]


@pytest.mark.parametrize("size", [(720, 720), (96, 64)])
@pytest.mark.parametrize("solver", [1, 2])
def test_captured_frames_are_renders(gpu_required, solver, size):
    """Slot A: one movep with capture on.  Slot B: the same trajectory one simulation step at a time, downloaded with
    render() wherever the schedule puts a frame.  One picker grasps a cloth corner, both are in view."""
    from flingbot_amd import sim as fsim

    w, h = size
    ctx = fsim.FlingSim(n_envs=2, solver=solver)
    xs, zs = _grid(32, 32)
    for e in range(2):
        _flat_cloth(ctx, e, 32, 32)
        cp = ctx.get_camera_params(e)
        ctx.set_camera_params(e, [*cp[2:8], w, h])
    down = np.array([[[xs[0], 0.02, zs[0]], [0.15, 0.1, 0.1]]] * 2)
    ctx.movep([0, 1], down, [[0, 0]] * 2, speed=2e-2)                  # both slots: picker 0 onto the corner particle
    ctx.capture_enable(0, w, h)
    up = np.array([[-0.1, 0.22, -0.05], [0.2, 0.15, 0.05]])
    start = ctx.get_shape_states(1).reshape(-1, 14)[:, :3].copy()
    grasp = [1, 0]
    iters = ctx.movep(0, up, [grasp], speed=5e-3)
    hold = ctx.get_shape_states(0).reshape(-1, 14)[:, :3].copy()        # float32 targets = the pickers' positions: no step
    iters_hold = ctx.movep(0, hold.astype(np.float32), [grasp], speed=1e-2, min_steps=10)
    assert int(iters) > 20 and int(iters_hold) == 11                     # (the hold: iterations 0 .. 10 take no step)
    frames = ctx.capture_take(0)
    assert ctx.capture_count(0) == 0 and ctx.capture_count(1) == 0
    plan = fsim.host_plan_movep(start, up, 5e-3)
    assert plan["iterations"] == int(iters) and len(plan["capture_after"]) == -(-int(iters) // 4) and plan["status"] == 1
    assert frames.shape == (len(plan["capture_after"]) + 3, h, w, 3) and frames.dtype == np.uint8
    assert ctx.picked(0)[0] >= 0 and ctx.picked(0)[1] == -1                # the previous-transform rule is exercised while moving
    want, at, done, loop = [], 0, 0, 0
    due = plan["capture_after"].tolist()
    while True:
        while at < len(due) and due[at] == done:
            want.append(_flipped_rgb(ctx, 1, w, h))
            at += 1
        if done == plan["steps"]:
            break
        prog, status, steps = ctx.advance([1], [0], [up], [grasp], [5e-3], [1000], [-1], [0], [loop], cap_min=1, cap=1)
        assert int(steps[0]) == 1
        loop, done = int(prog[0]), done + 1
    assert at == len(due)
    want += [_flipped_rgb(ctx, 1, w, h)] * 3                               # the hold: three repeats of the unchanged state
    for k, img in enumerate(want):
        assert np.array_equal(frames[k], img), (k, int((frames[k] != img).sum()))
    assert len({f.tobytes() for f in frames[:len(due)]}) > len(due) // 2   # (the film moves)
    assert np.array_equal(ctx.get_positions(0).view(np.uint32), ctx.get_positions(1).view(np.uint32))
    # refusals are host-side argument checks
    with pytest.raises(fsim.FlingSimError):
        ctx.capture_enable(0, 0, 64)
    with pytest.raises(fsim.FlingSimError):
        ctx.capture_enable(5, 64, 64)
    ctx.capture_disable(0)
    # frames that wait survive a disable, but not a change of the frame size (their bytes would be reinterpreted)
    ctx.capture_enable(0, w, h)
    ctx.movep(0, up, [grasp], speed=1e-2, min_steps=5)
    ctx.capture_disable(0)
    assert ctx.capture_count(0) == 2
    ctx.capture_enable(0, w, h)
    assert ctx.capture_count(0) == 2
    ctx.capture_disable(0)
    ctx.capture_enable(0, 48, 32)
    assert ctx.capture_count(0) == 0 and ctx.capture_take(0).shape == (0, 32, 48, 3)
    ctx.close()


def test_capture_does_not_touch_the_simulation(gpu_required):
    from flingbot_amd import sim as fsim

    sizes = [(24, 24), (32, 32), (40, 28)]
    out = {}
    for film in (True, False):
        ctx = fsim.FlingSim(n_envs=3, solver=0)
        for e, (dx, dz) in enumerate(sizes):
            _flat_cloth(ctx, e, dx, dz)
        if film:
            ctx.capture_enable(0, 64, 48)
            ctx.capture_enable(2, 80, 80)
        seq0 = ctx.advance_timing()["sequences"]
        tg = [[[_grid(dx, dz)[0][0], 0.02, _grid(dx, dz)[1][0]], [0.1 + 0.01 * e, 0.1, 0.1]] for e, (dx, dz) in enumerate(sizes)]
        it1 = ctx.movep([0, 1, 2], tg, [[0, 0]] * 3, speed=1e-2)
        up = [[[-0.05, 0.2 + 0.02 * e, 0.0], [0.2, 0.1, 0.1]] for e in range(3)]
        it2 = ctx.movep([0, 1, 2], up, [[1, 0]] * 3, speed=4e-3)
        # the same through the chunk executor, one blocking chunk after another
        back = np.array([[[0.0, 0.1, 0.0], [0.1, 0.1, 0.0]]] * 3)
        start, live, it3 = np.zeros(3, np.int32), [0, 1, 2], np.zeros(3, np.int32)
        while live:
            k = len(live)
            prog, status, steps = ctx.advance(live, [0] * k, back[live], [[1, 0]] * k, [6e-3] * k, [1000] * k, [-1] * k, [0] * k,
                                              start[live], cap_min=5, cap=9)
            for q, e in enumerate(list(live)):
                start[e] = prog[q]
                if status[q] != 0:
                    it3[e] = prog[q]
                    live.remove(e)
        out[film] = dict(pos=[ctx.get_positions(e) for e in range(3)], vel=[ctx.get_velocities(e) for e in range(3)],
                         shapes=[ctx.get_shape_states(e) for e in range(3)], iters=(it1, it2, it3),
                         seq=ctx.advance_timing()["sequences"] - seq0,
                         frames=[ctx.capture_take(e) if film else None for e in range(3)])
        ctx.close()
    a, b = out[True], out[False]
    for e in range(3):
        for key in ("pos", "vel", "shapes"):
            assert np.array_equal(a[key][e].view(np.uint32), b[key][e].view(np.uint32)), (key, e)
    assert a["seq"] == b["seq"] > 0   # same chunks, same launch sequences (capture renders are not sequences: no cost figure)
    for k in range(3):
        assert a["iters"][k].tolist() == b["iters"][k].tolist()
    closed = [sum(-(-int(a["iters"][k][e]) // 4) for k in range(3)) for e in range(3)]
    assert a["frames"][0].shape == (closed[0], 48, 64, 3) and a["frames"][2].shape == (closed[2], 80, 80, 3)
    assert a["frames"][1].shape[0] == 0


class _StepByStep:
    """A FlingSim whose advance() runs one simulation step per call and notes, for every frame the call captured, the
    particle sample of the state after it (a call of one step captures either before its step -- then it takes none: the
    pickers sit on their targets -- or after it, so the state after the call is the state of each of its frames)."""

    def __init__(self, sim, filmed, sample_ids):
        self._sim, self._filmed, self._ids = sim, filmed, sample_ids
        self.samples = {e: [] for e in filmed}
        self._seen = {e: 0 for e in filmed}

    def __getattr__(self, name):
        return getattr(self._sim, name)

    def advance(self, envs, *args, cap_min=1, cap=1, **kw):
        out = self._sim.advance(envs, *args, cap_min=1, cap=1, **kw)
        for e in self._filmed:
            new = self._sim.capture_count(e) - self._seen[e]
            if new:
                self.samples[e] += [self._sim.get_positions(e).reshape(-1, 4)[self._ids, :3].copy()] * new
                self._seen[e] += new
        return out


def test_all_drivers_film_the_same(gpu_required):
    """SimEnv.step with a fling (preaction, pick_and_fling, postaction) on four cloths of different sizes -- the first is
    the fixture's scene -- through the lock-step primitives, the blocking scheduler, the pipelined one with short chunks and
    a scheduler run of one step per call that reads the particles at every frame."""
    from flingbot_amd import schedule as sch, sim as fsim
    from flingbot_amd.primitives import FlingPrimitives

    g = _golden()
    sizes = [(32, 32), (24, 24), (28, 36), (40, 40)]
    frames, samples = {}, None
    for driver in ("lockstep", "programs", "pipelined", "stepwise"):
        ctx = fsim.FlingSim(n_envs=4, solver=0)
        for e, (dx, dz) in enumerate(sizes):
            _flat_cloth(ctx, e, dx, dz, pickers=False)
        sim = _StepByStep(ctx, [0], g["sample_ids"]) if driver == "stepwise" else ctx
        prim = FlingPrimitives(sim, range(4), dump_visualizations=True, frame_size=(64, 48))
        prim.setup_pickers()
        assert all(ctx.capture_count(e) == 0 for e in range(4))           # nothing of the reset is filmed
        p1 = [[_grid(dx, dz)[0][0], 0.0, _grid(dx, dz)[1][0]] for dx, dz in sizes]
        p2 = [[_grid(dx, dz)[0][-1], 0.0, _grid(dx, dz)[1][0]] for dx, dz in sizes]
        prim.preaction()
        if driver == "lockstep":
            prim.pick_and_fling(p1, p2, [True] * 4, [True] * 4)
            prim.postaction()
        elif driver == "pipelined":
            progs = {e: sch.action_then_settle(sch.Episode(prim, e), sch.pick_and_fling(sch.Episode(prim, e), p1[e], p2[e], True, True))
                     for e in range(4)}
            sch.run_programs(prim, progs, cap_min=1, cap=4, pipeline=True, depth=2)
        else:
            prim.act_scheduled({e: ("fling", p1[e], p2[e], True, True) for e in range(4)})
        frames[driver] = [prim.take_frames(e) for e in range(4)]
        if driver == "stepwise":
            samples = np.array(sim.samples[0], np.float32)
        assert np.array_equal(ctx.get_positions(0).view(np.uint32), g["c1_final_pos"].view(np.uint32)), driver
        ctx.close()
    keep = g["c1_f_discarded"] == 0
    for driver in frames:
        assert frames[driver][0].shape == (int(keep.sum()), 48, 64, 3), driver
        for e in range(4):
            assert np.array_equal(frames[driver][e], frames["lockstep"][e]), (driver, e)
    assert len({f.shape[0] for f in frames["lockstep"]}) > 1              # (different cloths: different films)
    assert np.array_equal(samples.view(np.uint32), g["c1_f_sample"][keep].view(np.uint32))


def test_capture_scratch_is_private(gpu_required):
    """While a chunk with captures is open on the main stream, the observation stage renders another episode on the
    service lane: both results equal those of runs that did not overlap."""
    import torch
    from flingbot_amd import sim as fsim

    def run(film, observe):
        ctx = fsim.FlingSim(n_envs=3, solver=0)
        for e in range(3):
            _flat_cloth(ctx, e, 32, 32)
        ctx.movep([2], [[[0.0, 0.05, 0.0], [0.1, 0.05, 0.05]]], [[0, 0]], speed=2e-2)
        if film:
            ctx.capture_enable(0, 720, 720)
        tg = np.array([[[-0.1, 0.3, -0.1], [0.2, 0.3, 0.1]]] * 2)
        tk, prog, status, steps = ctx.advance_begin([0, 1], [0, 0], tg, [[0, 0]] * 2, [4e-3] * 2, [1000] * 2, [-1] * 2, [0] * 2,
                                                    [0, 0], cap_min=48, cap=48)
        obs = None
        if observe:
            ctx.service_lane(True)
            if film:
                with pytest.raises(fsim.FlingSimError):     # a rewrite of an episode the chunk moves: refused on the lane
                    ctx.capture_disable(0)
            o, bbox = ctx.observe_batch([2], 128)
            obs = (o.cpu().numpy(), bbox.copy())
            ctx.service_lane(False)
        ctx.advance_end(tk, prog, status, steps)
        torch.cuda.synchronize()
        out = dict(obs=obs, frames=ctx.capture_take(0) if film else None, pos=ctx.get_positions(0), steps=int(steps[0]))
        ctx.close()
        return out

    both, alone, plain = run(True, True), run(True, False), run(False, True)
    assert both["steps"] == 48 and both["frames"].shape == (12, 720, 720, 3)
    assert np.array_equal(both["frames"], alone["frames"])
    assert np.array_equal(both["obs"][0].view(np.uint32), plain["obs"][0].view(np.uint32)) and np.array_equal(both["obs"][1], plain["obs"][1])
    assert np.array_equal(both["pos"].view(np.uint32), plain["pos"].view(np.uint32))


def test_evaluation_loop_films_the_first_tasks(gpu_required, tmp_path):
    import torch
    from PIL import Image

    from flingbot_amd import evaluate, nets, sim as fsim, taskio, tasks as ftasks
    from flingbot_amd.env import BatchedFlingEnv

    random.seed(3); np.random.seed(3); torch.manual_seed(3)
    n = 12
    gen = fsim.FlingSim(n_envs=n, solver=0)
    tasks = ftasks.generate_tasks(gen, [ftasks.draw_task_parameters(min_cloth_size=20, strict_min_edge_length=20, max_cloth_size=30)
                                        for _ in range(n)])
    gen.close()
    assert all(t is not None for t in tasks)
    policy = None

    def run(root):
        nonlocal policy
        ctx = fsim.FlingSim(n_envs=6, solver=0)
        kw = {} if root is None else dict(dump_visualizations=True, visualize=[0, 1, 2], frame_size=(120, 120),
                                          visualization_root=str(root))
        env = BatchedFlingEnv(ctx, image_dim=128, episode_length=2, **kw)
        if policy is None:
            policy = nets.MaximumValuePolicy(action_primitives=["fling"], num_rotations=12, scale_factors=list(env.scale_factors),
                                             obs_dim=64, pix_grasp_dist=8, pix_drag_dist=8, pix_place_dist=5, rgb_only=True,
                                             depth_only=False, action_expl_prob=0.0, action_expl_decay=1.0, value_expl_prob=0.0,
                                             value_expl_decay=1.0, device="cuda:0")
        stats = evaluate.run_tasks(policy, env, tasks)
        ctx.close()
        return stats["records"]

    plain, film1, film2 = run(None), run(tmp_path / "a"), run(tmp_path / "b")
    strip = lambda r: {k: v for k, v in r.items() if k != "visualization_dir"}   # noqa: E731
    for i in range(3, n):
        assert film1[i] == plain[i], i                                   # the nine others: exactly as without the option
    for i in range(3):
        assert strip(film1[i]) == strip(film2[i]), i                     # the filmed ones: reproducible
        assert film1[i]["visualization_dir"] == str(tmp_path / "a" / evaluate.film_name(tasks, i))
    assert ["visualization_dir" in r for r in film1] == [True] * 3 + [False] * 9
    assert sorted(os.listdir(tmp_path / "a")) == sorted(evaluate.film_name(tasks, i) for i in range(3))
    for i in range(3):
        counts = []
        for root in ("a", "b"):
            d = tmp_path / root / evaluate.film_name(tasks, i)
            assert os.listdir(d) == [taskio.VIDEO_NAME]
            with Image.open(d / taskio.VIDEO_NAME) as im:
                assert im.size == (120, 120) and im.n_frames > 10
                im.seek(im.n_frames - 1)
                counts.append((im.n_frames, np.asarray(im.convert("RGB")).tobytes()))
        assert counts[0] == counts[1]
    path = str(tmp_path / "replay.npz")
    taskio.save_replay(path, film1, tasks)
    z = np.load(path)
    assert sum(1 for k in z.files if k.endswith("/visualization_dir")) == sum(len(film1[i]["actions"]) for i in range(3))


def test_second_reset_of_a_slot_films_nothing_of_the_reset(gpu_required, tmp_path):
    """BatchedFlingEnv.reset / step_actions (the lock-step driver) twice on the same slots, the second cloths LARGER: nothing of
    a reset is filmed, the film is closed when the episode ends, and the second film is the one a fresh environment makes."""
    import torch  # noqa: F401
    from PIL import Image

    from flingbot_amd import sim as fsim, taskio, tasks as ftasks
    from flingbot_amd.env import BatchedFlingEnv

    random.seed(11); np.random.seed(11)
    gen = fsim.FlingSim(n_envs=4, solver=0)
    small = ftasks.generate_tasks(gen, [ftasks.draw_task_parameters(min_cloth_size=20, strict_min_edge_length=20, max_cloth_size=24)
                                        for _ in range(2)])
    large = ftasks.generate_tasks(gen, [ftasks.draw_task_parameters(min_cloth_size=34, strict_min_edge_length=34, max_cloth_size=40)
                                        for _ in range(2)])
    gen.close()
    assert all(t is not None for t in small + large)
    assert min(len(t["particle_pos"]) for t in large) > max(len(t["particle_pos"]) for t in small)

    def act(env, root):
        """One scripted fling per episode (episode_length 1: the episode ends, its film is closed)."""
        chosen = {}
        for e in env.envs:
            pos = ctx_of[env].get_positions(e).reshape(-1, 4)[:, :3]
            a, b = pos[np.argmin(pos[:, 0])].copy(), pos[np.argmax(pos[:, 0])].copy()
            chosen[e] = ("fling", dict(p1=a.astype(np.float64), p2=b.astype(np.float64), p1_grasp_cloth=True, p2_grasp_cloth=True))
        env.step_actions(list(env.envs), chosen)
        assert all(env.terminate.values())
        out = {}
        for e in env.envs:
            assert env.visualization_dirs[e] == str(root / f"episode{e:05d}")
            with Image.open(root / f"episode{e:05d}" / taskio.VIDEO_NAME) as im:
                frames = []
                for k in range(im.n_frames):
                    im.seek(k)
                    frames.append(np.asarray(im.convert("RGB")).copy())
            out[e] = np.array(frames)
        return out

    ctx_of = {}

    def make(root):
        ctx = fsim.FlingSim(n_envs=2, solver=0)
        env = BatchedFlingEnv(ctx, image_dim=128, episode_length=1, dump_visualizations=True, frame_size=(64, 64),
                              visualization_root=str(root))
        ctx_of[env] = ctx
        return ctx, env

    ctx, env = make(tmp_path / "twice")
    env.reset(small)
    assert [ctx.capture_count(e) for e in range(2)] == [0, 0]
    first = act(env, tmp_path / "twice")
    for e in range(2):   # an episode that ended leaves nothing behind: capture off, no frame waiting
        assert ctx.capture_count(e) == 0
    env.reset(large)                                       # same slots, more particles: must neither raise nor film
    assert [ctx.capture_count(e) for e in range(2)] == [0, 0]
    second = act(env, tmp_path / "twice")
    ctx.close()
    ctx2, env2 = make(tmp_path / "fresh")
    env2.reset(large)
    fresh = act(env2, tmp_path / "fresh")
    ctx2.close()
    for e in range(2):
        assert first[e].shape[0] > 10 and second[e].shape[1:] == (64, 64, 3)
        assert np.array_equal(second[e], fresh[e]), e      # it starts with the first movep of the action, like a first film
    # and when the earlier episode did NOT end (its film still open, frames still waiting), the next reset drops them
    ctx3, env3 = make(tmp_path / "open")
    env3.episode_length = 5
    env3.reset(small)
    env3.prim.movep([0, 1], [[[0.3, 0.4, -0.3], [-0.3, 0.4, -0.3]]] * 2, speed=2e-2)
    assert ctx3.capture_count(0) > 0
    env3.episode_length = 1
    env3.reset(large)
    assert [ctx3.capture_count(e) for e in range(2)] == [0, 0]
    again = act(env3, tmp_path / "open")
    ctx3.close()
    for e in range(2):
        assert np.array_equal(again[e], fresh[e]), e
