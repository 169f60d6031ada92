"""dump_visualizations without a GPU: the capture schedule of the library's movep planner, the flag's physics in
flingbot_amd.primitives / schedule (default speed 1e-2, the three holds) and the film writer, against
tests/golden/capture_golden.npz -- recorded from the REFERENCE's own SimEnv with the flag set (make_capture_golden.py)."""
import os

import numpy as np
import pytest

from fling_helpers import GOLD, OracleBatch


def _golden():
    return np.load(os.path.join(GOLD, "capture_golden.npz"))


def _moveps(g):
    """Every recorded SimEnv.movep call: (case, index, start, targets in the caller's dtype, speed, min_steps, limit)."""
    for c in range(int(g["n_cases"])):
        for m in range(len(g[f"c{c}_m_iters"])):
            speed = g[f"c{c}_m_speed"][m]
            speed = float(g["default_speed"]) if np.isnan(speed) else float(speed)   # None under the flag: default_speed
            tg = g[f"c{c}_m_targets"][m]
            tg = tg.astype(np.float32) if g[f"c{c}_m_f32"][m] else tg
            ms = int(g[f"c{c}_m_min_steps"][m])
            yield c, m, g[f"c{c}_m_start"][m], tg, speed, (None if ms < 0 else ms), int(g[f"c{c}_m_limit"][m])


def test_fixture_holds_what_the_issue_asks_for():
    g = _golden()
    assert os.path.getsize(os.path.join(GOLD, "capture_golden.npz")) < 300 * 1024
    speeds = np.concatenate([g[f"c{c}_m_speed"] for c in range(4)])
    mins = np.concatenate([g[f"c{c}_m_min_steps"] for c in range(4)])
    assert np.isnan(speeds).sum() >= 6 and ((mins == 10) & np.isnan(speeds)).sum() == 3   # three no-speed moves, three holds
    assert g["c0_m_raised"].tolist() == [0, 0, 0, 1] and g["c0_m_iters"].tolist()[1:] == [60, 21, 10]
    assert g["c0_m_steps"][2] == 0                                 # the min_steps=20 movep that starts on target never steps
    for c in range(4):
        assert (g[f"c{c}_f_discarded"][g[f"c{c}_f_movep"] == 0] == 1).all()   # reset's own reset_end_effectors: dropped
        assert (g[f"c{c}_f_discarded"][g[f"c{c}_f_movep"] > 0] == 0).all()


def test_host_plan_reproduces_the_reference_schedule():
    from flingbot_amd import sim as fsim

    g = _golden()
    n = 0
    for c, m, start, tg, speed, ms, limit in _moveps(g):
        p = fsim.host_plan_movep(start, tg, speed, limit=limit, min_steps=ms)
        iters = int(g[f"c{c}_m_iters"][m])
        sel = g[f"c{c}_f_movep"] == m
        assert p["iterations"] == iters and p["steps"] == int(g[f"c{c}_m_steps"][m]), (c, m)
        assert p["status"] == (2 if g[f"c{c}_m_raised"][m] else 1), (c, m)
        assert p["capture_iter"].tolist() == g[f"c{c}_f_iter"][sel].tolist(), (c, m)
        assert len(p["capture_iter"]) == -(-iters // 4), (c, m)                       # ceil(I / 4)
        # the simulation-step counter at every frame: the movep's steps before it + capture_after
        first = int(g[f"c{c}_f_simstep"][sel][0] - p["capture_after"][0]) if sel.any() else 0
        assert (first + p["capture_after"]).tolist() == g[f"c{c}_f_simstep"][sel].tolist(), (c, m)
        n += 1
    assert n >= 50


@pytest.mark.parametrize("cap", [1, 3, 8, 64])
def test_host_plan_in_pieces_equals_one_piece(cap):
    from flingbot_amd import sim as fsim

    g = _golden()
    for c, m, start, tg, speed, ms, limit in _moveps(g):
        whole = fsim.host_plan_movep(start, tg, speed, limit=limit, min_steps=ms)
        pos, it, steps, pts, pieces = start, 0, 0, [], 0
        while True:
            p = fsim.host_plan_movep(pos, tg, speed, limit=limit, min_steps=ms, start=it, max_steps=cap)
            pts += [(steps + int(a), int(i)) for a, i in zip(p["capture_after"], p["capture_iter"])]
            assert p["steps"] <= cap
            pos, it, steps, pieces = p["end_pos"], p["iterations"], steps + p["steps"], pieces + 1
            if p["status"] != 0:
                break
            assert pieces < 2000
        assert (it, steps, p["status"]) == (whole["iterations"], whole["steps"], whole["status"]), (c, m)
        assert pts == list(zip(whole["capture_after"].tolist(), whole["capture_iter"].tolist())), (c, m)
        assert np.array_equal(pos.view(np.uint32), whole["end_pos"].view(np.uint32)), (c, m)


class RecordingOracle(OracleBatch):
    """OracleBatch that records instead of rendering: oracle/picker.py's movep calls pick_place_step once per loop
    iteration, so wrapping that call and counting from `start` gives the loop index the reference films by."""

    def __init__(self, n, scene_params, init_pos, sample_ids):
        super().__init__(n, scene_params, init_pos, pickers=False)
        self.sample_ids = sample_ids
        self.filmed, self.frames, self.moveps, self.sim_steps_of = set(), {}, {}, {}
        self.capture_log = []
        for e in range(n):
            self.frames[e], self.moveps[e], self.sim_steps_of[e] = [], [], 0
            self._wrap(e)

    def _wrap(self, e):
        o, t = self.sims[e], self.tools[e]
        o_step, t_pps, t_movep = o.step, t.pick_place_step, t.movep

        def step(n=1):
            self.sim_steps_of[e] += n
            return o_step(n)

        def pick_place_step(action):
            taken = t_pps(action)
            index = self._loop[e]
            self._loop[e] += 1
            self.moveps[e][-1]["iters"] = index + 1
            self.moveps[e][-1]["steps"] += taken
            if e in self.filmed and index % 4 == 0:
                self.frames[e].append(dict(movep=len(self.moveps[e]) - 1, iter=index, simstep=self.sim_steps_of[e],
                                           pickers=np.array(o.get_shape_states(), np.float32).reshape(-1, 14)[:, :3].copy(),
                                           sample=o.get_positions().reshape(-1, 4)[self.sample_ids, :3].copy()))
            return taken

        def movep(pos, grasp_states, start=0, **kw):
            if start == 0:
                self.moveps[e].append(dict(iters=0, steps=0))
            self._loop[e] = start
            return t_movep(pos, grasp_states, start=start, **kw)

        self._loop = getattr(self, "_loop", {})
        o.step, t.pick_place_step, t.movep = step, pick_place_step, movep

    def capture_enable(self, e, width, height):
        self.capture_log.append(("enable", int(e), int(width), int(height), self.sim_steps_of[int(e)]))
        self.filmed.add(int(e))

    def capture_disable(self, e):
        self.capture_log.append(("disable", int(e)))
        self.filmed.discard(int(e))

    def capture_take(self, e):
        out, self.frames[int(e)] = self.frames[int(e)], []
        return out


def _check_case(g, c, sim, e, frames):
    keep = g[f"c{c}_f_discarded"] == 0
    assert len(frames) == int(keep.sum()), (c, len(frames), int(keep.sum()))
    for key in ("movep", "iter", "simstep"):
        assert [f[key] for f in frames] == g[f"c{c}_f_{key}"][keep].tolist(), (c, key)
    pick = np.array([f["pickers"] for f in frames], np.float32)
    samp = np.array([f["sample"] for f in frames], np.float32)
    assert np.array_equal(pick.view(np.uint32), g[f"c{c}_f_pickers"][keep].view(np.uint32)), c
    assert np.array_equal(samp.view(np.uint32), g[f"c{c}_f_sample"][keep].view(np.uint32)), c
    assert [m["iters"] for m in sim.moveps[e]] == g[f"c{c}_m_iters"].tolist(), c
    assert [m["steps"] for m in sim.moveps[e]] == g[f"c{c}_m_steps"].tolist(), c
    assert np.array_equal(sim.sims[e].get_positions().view(np.uint32), g[f"c{c}_final_pos"].view(np.uint32)), c
    assert np.array_equal(np.array(sim.sims[e].get_shape_states(), np.float32).view(np.uint32),
                          g[f"c{c}_final_shapes"].view(np.uint32)), c


def _bring_up(g, n):
    from flingbot_amd.primitives import FlingPrimitives

    sim = RecordingOracle(n, g["scene_params"], g["init_pos"], g["sample_ids"])
    prim = FlingPrimitives(sim, range(n), dump_visualizations=True, frame_size=(96, 64))
    prim.setup_pickers()
    # filmed from the end of the reset on: after reset_end_effectors (166 steps) and the reset's own step
    # (before it: capture off for the slots, in case an earlier episode left it on)
    assert sim.capture_log == [("disable", e) for e in range(n)] + [("enable", e, 96, 64, 167) for e in range(n)]
    assert all(sim.frames[e] == [] for e in range(n))
    return sim, prim


@pytest.mark.parametrize("driver", ["lockstep", "programs"])
def test_primitives_with_the_flag_reproduce_the_reference(driver):
    """Cases of the fixture, each on its own oracle-backed episode: 0 three single moveps, 1 SimEnv.step with a fling
    (preaction, pick_and_fling_primitive, postaction), 2 pick_stretch_drag_primitive, 3 pick_and_place_primitive."""
    from concurrent.futures import ThreadPoolExecutor

    from flingbot_amd.primitives import FlingPrimitives

    g = _golden()
    sim, prim = _bring_up(g, 4)
    subs = {e: FlingPrimitives(sim, [e], dump_visualizations=True, frame_size=(96, 64)) for e in range(4)}

    def case0():
        p = subs[0]
        p.movep([0], [[[0.3, 0.4, -0.3], [-0.3, 0.4, -0.3]]], speed=5e-3)
        p.movep([0], np.array([p.picker_positions(0)]), speed=5e-4, min_steps=20)   # float32 targets, on target
        with pytest.raises(RuntimeError):
            p.movep([0], [[[0.0, 0.2, 0.0], [-0.1, 0.2, 0.0]]], speed=5e-3, limit=10)

    case0()
    acts = {1: ("fling", g["fling_p1"].copy(), g["fling_p2"].copy(), True, True),
            2: ("stretchdrag", g["stretchdrag_p1"].copy(), g["stretchdrag_p2"].copy(), True, True),
            3: ("place", g["place_p1"].copy(), g["place_p2"].copy(), True, True)}
    if driver == "lockstep":
        def fling():
            subs[1].preaction([1])
            subs[1].pick_and_fling([acts[1][1]], [acts[1][2]], [True], [True])
            subs[1].postaction([1])

        with ThreadPoolExecutor(3) as pool:
            jobs = [pool.submit(fling), pool.submit(subs[2].pick_stretch_drag, [acts[2][1]], [acts[2][2]], [True], [True]),
                    pool.submit(subs[3].pick_and_place, [acts[3][1]], [acts[3][2]], [True], [True])]
            for j in jobs:
                j.result()
    else:
        prim.preaction([1])
        prim.act_scheduled({2: acts[2], 3: acts[3]}, envs=[2, 3], settle=False, cap_min=3, cap=7)
        prim.act_scheduled({1: acts[1]}, envs=[1], settle=True, cap_min=8, cap=64)
    for c in range(4):
        _check_case(g, c, sim, c, (subs[c] if driver == "lockstep" else prim).take_frames(c))
    assert sum(kind == "disable" for kind, *_ in sim.capture_log) == 4      # those of the reset; nothing stops the film later


def test_flag_off_changes_nothing():
    from flingbot_amd import schedule as sch
    from flingbot_amd.primitives import FlingPrimitives

    class Stub:
        def __init__(self):
            self.speeds, self.last_movep_steps = [], 0

        def movep(self, envs, targets, grasp, speed=None, **kw):
            self.speeds.append((speed, kw.get("min_steps")))

        def __getattr__(self, name):
            raise AssertionError(f"unexpected simulator call {name}")

    tg = [[0.0, 0.1, 0.0], [0.1, 0.1, 0.0]]
    off, on = FlingPrimitives(Stub(), [0]), FlingPrimitives(Stub(), [0], dump_visualizations=True)
    assert off.visualize == [] and on.visualize == [0] and off.take_frames(0) is None
    off.start_capture(), off.stop_capture()            # no capture call reaches the simulator
    for prim, want in ((off, 0.1), (on, 1e-2)):
        prim.movep([0], [tg])
        prim.movep([0], [tg], speed=5e-3)
        assert prim.sim.speeds == [(want, None), (5e-3, None)]
        ep = sch.Episode(prim, 0)
        assert next(sch._movep(ep, tg))[2] == want and next(sch._movep(ep, tg, speed=2e-3))[2] == 2e-3
    assert list(sch._hold(sch.Episode(off, 0), tg)) == []
    held = list(sch._hold(sch.Episode(on, 0), tg))
    assert len(held) == 1 and held[0][2] == 1e-2 and held[0][3] == 10
    off.fling_primitive([0], [0.2], [0.3], 6e-3)
    on.sim.speeds.clear()
    on.fling_primitive([0], [0.2], [0.3], 6e-3)
    assert len(on.sim.speeds) == len(off.sim.speeds) - 2 + 1 and (1e-2, 10) in on.sim.speeds and (0.1, 10) not in off.sim.speeds


def test_frame_dump_writes_an_animated_png(tmp_path):
    from PIL import Image

    from flingbot_amd import taskio

    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (7, 10, 14, 3), dtype=np.uint8)
    dump = taskio.FrameDump(tmp_path / "ep")
    dump.append(frames[:3])
    dump.append(frames[3:3])      # an action that moved nothing
    dump.append(frames[3:])
    assert sorted(os.listdir(tmp_path / "ep" / ".frames")) == ["000000.npy", "000001.npy"]
    assert dump.finish() == str(tmp_path / "ep")
    assert os.listdir(tmp_path / "ep") == [taskio.VIDEO_NAME]
    with Image.open(tmp_path / "ep" / taskio.VIDEO_NAME) as im:
        assert im.n_frames == 7 and im.size == (14, 10)
        for k in range(7):
            im.seek(k)
            assert np.array_equal(np.asarray(im.convert("RGB")), frames[k]), k
            assert abs(im.info["duration"] - 1000.0 / 24.0) < 1e-6
    empty = taskio.FrameDump(tmp_path / "none")
    assert empty.finish() is None


def test_replay_carries_visualization_dir(tmp_path):
    from flingbot_amd import taskio

    rec = lambda **kw: dict(coverage=[0.1, 0.2, 0.3], actions=["fling", None], rewards=[0.1, 0.1],   # noqa: E731
                            preaction_coverage=[0.1, 0.2], **kw)
    task = dict(cloth_mass=0.5, flatten_area=0.4, task_difficulty="hard", initial_coverage=0.1)
    path = str(tmp_path / "replay.npz")
    assert taskio.save_replay(path, [rec(visualization_dir="/films/a"), rec()], [task, task]) == 4
    z = np.load(path)
    assert str(z["000000000_step00/visualization_dir"]) == "/films/a" == str(z["000000000_step01_last/visualization_dir"])
    assert "000000001_step00/visualization_dir" not in z.files
    stats = taskio.collect_stats(path)
    plain = str(tmp_path / "plain.npz")
    taskio.save_replay(plain, [rec(), rec()], [task, task])
    want = taskio.collect_stats(plain)
    assert stats.keys() == want.keys() and all(np.array_equal(stats[k], want[k]) for k in want)


def test_evaluate_options_map_onto_the_environment():
    import inspect

    from flingbot_amd import evaluate
    from flingbot_amd.env import BatchedFlingEnv

    ap = evaluate.build_parser()
    plain = evaluate.parse_film_options(ap, ap.parse_args(["--tasks", "set.npz"]))
    assert plain.dump_visualizations is None and evaluate.film_env_kwargs(plain) == {}
    a = evaluate.parse_film_options(ap, ap.parse_args(["--tasks", "set.npz", "--dump-visualizations", "films"]))
    assert evaluate.film_env_kwargs(a) == dict(dump_visualizations=True, visualize=list(range(8)), frame_size=(720, 720),
                                               visualization_root="films")
    a = evaluate.parse_film_options(ap, ap.parse_args(["--tasks", "set.npz", "--dump-visualizations", "films", "--visualize", "3",
                                                       "--frame-size", "240"]))
    kw = evaluate.film_env_kwargs(a)
    assert kw["visualize"] == [0, 1, 2] and kw["frame_size"] == (240, 240)
    assert set(kw) <= set(inspect.signature(BatchedFlingEnv.__init__).parameters)
    with pytest.raises(SystemExit):
        evaluate.parse_film_options(ap, ap.parse_args(["--tasks", "set.npz", "--frame-size", "4"]))

    class T:
        name = "abc123"
    assert evaluate.film_name([T(), dict()], 0) == "abc123" and evaluate.film_name([T(), dict()], 1) == "task00001"

    class Odd:
        name = "../a b/c"
    assert evaluate.film_name([Odd()], 0) == ".._a_b_c" and os.sep not in evaluate.film_name([Odd()], 0)
    Odd.name = ".."
    assert evaluate.film_name([Odd()], 0) == "task00000"
