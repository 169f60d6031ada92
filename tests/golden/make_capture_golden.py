"""Generates tests/golden/capture_golden.npz: what the REFERENCE's own SimEnv does under `dump_visualizations = True`
(environment/simEnv.py:739-769 movep's speed switch and frame schedule, :277-280 / :300-301 / :395-397 the three holds,
:677-681 the frames reset discards), recorded by running its code on the oracle-backed `pyflex` stand-in that
make_golden.py step_vectors() uses, with `environment.simEnv.get_image` replaced by a recorder.

    python tests/golden/make_capture_golden.py

The reference is imported at run time from its checkout (read-only; it never travels to the GPU machine) -- only numbers go
into the fixture.  Per 32 x 32 cloth case:
    m_*   one row per SimEnv.movep call: the pickers' float32 positions at entry, targets (float64 values + whether the
          caller's array was float32), speed / min_steps as passed (NaN / -1 = None), limit, loop iterations
          (= action_tool.step calls), simulation steps, whether MoveJointsException was raised
    f_*   one row per recorded frame: index of its movep, loop index, the case's simulation-step counter, picker positions,
          a fixed sample of 64 particle positions, and `discarded` = taken before reset emptied env_video_frames
    wait_steps   simulation steps SimEnv.step spent outside movep (wait_until_stable); 0 in the recorded fling -- the cloth
                 is already still when the wait looks -- so the fixture does not exercise "no frame during the wait"
Cases: 0 = three single moveps after the reset (one that ends on target, one with min_steps=20 that starts on its float32
targets, one that runs into limit=10); 1 = SimEnv.step with a scripted fling (pick_and_fling_primitive + postaction: the
reset / step boundary); 2 = pick_stretch_drag_primitive; 3 = pick_and_place_primitive.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("FLINGBOT_REFERENCE", "/root/reference")
N_SAMPLE = 64


def main():
    sys.path.insert(0, ROOT)
    from oracle import OracleSim

    if not hasattr(np, "alltrue"):
        np.alltrue = np.all
    import scipy.ndimage  # noqa: F401
    import torch  # noqa: F401

    class _Any:
        def __init__(self, *a, **k): pass
        def __call__(self, *a, **k): return _Any()
        def __getattr__(self, name): return _Any()

    def anystub(name):
        m = types.ModuleType(name)

        def _ga(attr):
            if attr.startswith("__"):
                raise AttributeError(attr)
            return _Any()
        m.__getattr__ = _ga
        m.__path__ = []
        m.__file__ = "<stub %s>" % name
        sys.modules[name] = m
        return m

    for name in ("h5py", "filelock", "imageio", "trimesh", "OpenEXR", "Imath", "cv2", "PIL", "skimage", "skimage.morphology",
                 "matplotlib", "matplotlib.pyplot", "ray", "pyflex"):
        if name != "pyflex":
            try:
                __import__(name)
                continue
            except Exception:
                pass
        anystub(name)
    sys.modules["ray"].remote = lambda f: f
    box = {}
    pf = sys.modules["pyflex"]
    for name in ("get_positions", "set_positions", "get_velocities", "set_velocities", "get_shape_states",
                 "set_shape_states", "add_sphere", "get_phases", "set_phases"):
        setattr(pf, name, (lambda nm: lambda *a, **k: getattr(box["o"], nm)(*a, **k))(name))
    count = {"steps": 0}

    def _step(*a, **k):
        count["steps"] += 1
        box["o"].step(1)
    pf.step = _step
    for m in [k for k in sys.modules if k == "environment" or k.startswith("environment.") or k in ("flex_utils", "nets")]:
        del sys.modules[m]
    sys.path.insert(0, REF)
    from environment import flex_utils as ref_fu
    from environment import simEnv as ref_simenv
    from environment.exceptions import MoveJointsException
    ref_simenv.prepare_image = lambda *a, **k: "transformed_obs"
    SimEnv = ref_simenv.SimEnv

    sp = np.array([0, 0.2, 0, 32, 32, 0.9, 0.9, 0.9, 2, 0, 2, 0, np.pi / 2, -np.pi / 2, 0, 720, 720, 0.3, 0])
    dim = 32
    xs = (np.arange(dim) - (dim - 1) / 2) * 0.00625
    xx, zz = np.meshgrid(xs, xs)
    sample = np.linspace(0, dim * dim - 1, N_SAMPLE).astype(np.int64)
    out = {"scene_params": sp, "sample_ids": sample, "n_cases": np.array(4), "default_speed": np.array(1e-2),
           "fling_p1": np.array([xs[0], 0.0, xs[0]]), "fling_p2": np.array([xs[-1], 0.0, xs[0]]),
           "stretchdrag_p1": np.array([xs[3], 0.0, xs[20]]), "stretchdrag_p2": np.array([xs[-4], 0.0, xs[20]]),
           "place_p1": np.array([xs[5], 0.0, xs[5]]), "place_p2": np.array([xs[5] + 0.1, 0.0, xs[5]])}

    for ci in range(4):
        orc = OracleSim()
        box["o"] = orc
        orc.set_scene(sp)
        orc.step(1)
        n = orc.n
        w = orc.get_positions().reshape(-1, 4)[0, 3]
        pos = np.zeros((n, 4), np.float32)
        pos[:, 0], pos[:, 1], pos[:, 2], pos[:, 3] = xx.ravel(), 0.0125, zz.ravel(), w
        orc.set_positions(pos.ravel())
        orc.set_velocities(np.zeros(3 * n, np.float32))
        out["init_pos"] = pos
        env = SimEnv.__new__(SimEnv)
        env.gui, env.gui_step, env.dump_visualizations = False, 0, True
        env.default_speed, env.grasp_height, env.fling_speed, env.fixed_fling_height = 1e-2, 0.02, 6e-3, -1
        env.stretchdrag_dist = 0.3
        env.particle_radius = 0.00625
        env.grasp_states = [False, False]
        env.env_video_frames = {}
        env.episode_memory = _Any()
        env.current_task = _Any()
        env.obs_dim, env.parallelize_prepare_image, env.ray_handle = 64, False, {"val": "handle"}
        env.episode_length = 5
        env.action_handlers = {"fling": env.pick_and_fling_primitive, "stretchdrag": env.pick_stretch_drag_primitive,
                               "drag": env.pick_and_drag_primitive, "place": env.pick_and_place_primitive}
        env.get_obs = lambda: "obs"
        env.get_transformations = lambda: []
        env.on_episode_end = lambda *a, **k: None
        env.reset = lambda: ("reset", None)
        env.action_tool = ref_fu.PickerPickPlace(num_picker=2, particle_radius=0.00625, picker_radius=0.02,
                                                 picker_low=(-5, 0, -5), picker_high=(5, 5, 5))
        moveps, frames = [], []
        state = {"discard": 1}
        count["steps"] = 0

        tool_step = env.action_tool.step

        def counted_step(*a, _ts=tool_step, **k):   # one call per loop iteration of movep: its count is the loop index + 1
            moveps[-1]["iters"] += 1
            return _ts(*a, **k)
        env.action_tool.step = counted_step

        def recorder(*a, **k):
            m = moveps[-1]
            frames.append(dict(movep=len(moveps) - 1, iter=m["iters"] - 1, simstep=count["steps"], discarded=state["discard"],
                               pickers=np.array(orc.get_shape_states(), np.float32).reshape(-1, 14)[:, :3].copy(),
                               sample=orc.get_positions().reshape(-1, 4)[sample, :3].copy()))
            return (np.zeros((1, 1, 3), np.uint8), None)
        ref_simenv.get_image = recorder

        ref_movep = SimEnv.movep

        def movep(pos_, speed=None, limit=1000, min_steps=None, eps=1e-4, _env=env):
            tg = np.array(pos_)
            moveps.append(dict(start=np.array(orc.get_shape_states(), np.float32).reshape(-1, 14)[:, :3].copy(),
                               targets=tg.astype(np.float64), f32=int(tg.dtype == np.float32),
                               speed=np.nan if speed is None else float(speed), min_steps=-1 if min_steps is None else int(min_steps),
                               limit=int(limit), iters=0, steps0=count["steps"], raised=0))
            try:
                return ref_movep(_env, pos_, speed=speed, limit=limit, min_steps=min_steps, eps=eps)
            except MoveJointsException:
                moveps[-1]["raised"] = 1
                raise
            finally:
                moveps[-1]["steps"] = count["steps"] - moveps[-1]["steps0"]
        env.movep = movep

        # SimEnv.reset after set_scene (simEnv.py:674-681), the last statement included: the frames so far are dropped
        env.current_timestep, env.terminate = 0, False
        env.init_coverage = ref_fu.get_current_covered_area(env.particle_radius)
        env.action_tool.reset([0.2, 0.5, 0.0])
        env.reset_end_effectors()
        env.step_simulation()
        env.set_grasp(False)
        env.env_video_frames = {}
        state["discard"] = 0
        wait_steps = 0
        if ci == 0:
            env.movep([[0.3, 0.4, -0.3], [-0.3, 0.4, -0.3]], speed=5e-3)
            env.movep(list(env.action_tool._get_pos()[0]), speed=5e-4, min_steps=20)
            try:
                env.movep([[0.0, 0.2, 0.0], [-0.1, 0.2, 0.0]], speed=5e-3, limit=10)
            except MoveJointsException:
                pass
        elif ci == 1:
            env.get_max_value_valid_action = lambda vm: ("fling", dict(
                p1=out["fling_p1"].copy(), p2=out["fling_p2"].copy(), p1_grasp_cloth=True, p2_grasp_cloth=True))
            s0 = count["steps"]
            env.step(None)
            wait_steps = count["steps"] - s0 - sum(m["steps"] for m in moveps if m["steps0"] >= s0)
            out[f"c{ci}_terminate"] = np.array(bool(env.terminate))
        elif ci == 2:
            env.pick_stretch_drag_primitive(out["stretchdrag_p1"].copy(), out["stretchdrag_p2"].copy(), True, True)
        else:
            env.pick_and_place_primitive(out["place_p1"].copy(), out["place_p2"].copy(), True, True)
        n_kept = len(env.env_video_frames.get("top", []))
        assert n_kept == sum(1 for f in frames if not f["discarded"]), (n_kept, len(frames))
        for key in ("start", "targets", "f32", "speed", "min_steps", "limit", "iters", "steps", "raised"):
            out[f"c{ci}_m_{key}"] = np.array([m[key] for m in moveps])
        for key in ("movep", "iter", "simstep", "discarded"):
            out[f"c{ci}_f_{key}"] = np.array([f[key] for f in frames], np.int32)
        out[f"c{ci}_f_pickers"] = np.array([f["pickers"] for f in frames], np.float32)
        out[f"c{ci}_f_sample"] = np.array([f["sample"] for f in frames], np.float32)
        out[f"c{ci}_wait_steps"] = np.array(wait_steps)
        out[f"c{ci}_final_pos"] = orc.get_positions().copy()
        out[f"c{ci}_final_shapes"] = np.array(orc.get_shape_states(), np.float32)
        out[f"c{ci}_grasp"] = np.array([bool(g) for g in env.grasp_states])
        print("case", ci, "moveps", len(moveps), "frames", len(frames), "kept", n_kept, "sim steps", count["steps"],
              "iterations", [m["iters"] for m in moveps], "wait", wait_steps)
    path = os.path.join(HERE, "capture_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
