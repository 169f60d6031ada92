"""What the per-episode appearance costs (flingbot_amd/appearance.py; EXPERIMENTS.md R20.1).

    python scripts/appearance_timing.py [--parent-lib PATH/libflingsim.so] [--episodes 64] [--rounds 5] [--tasks 96] [--actions 3]

1. observe_batch of --episodes episodes of 64 x 64 cloths, 720^2 render -> 400^2 observation, one child process per
   measurement so that two builds of the library can alternate in one call: the parent commit's library (--parent-lib, loaded
   through FLINGSIM_LIB; skipped when absent), this tree's with the flag off (no setter call), and this tree's with a freshly
   drawn appearance per episode before every call (the setter call and the 64 draws are inside the timed window, and timed on
   their own as well).  Every child warms up, then times --calls calls and prints their median; --rounds alternations.
2. The `continuous` evaluation loop (evaluate.run_tasks) of --tasks generated hard tasks, up to --actions actions, with
   randomize_appearance off and "observation", alternating, --rounds rounds."""
import argparse
import json
import os
import random
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def child(mode, episodes, calls):
    import torch

    from flingbot_amd import appearance, sim as fsim
    from scenarios import cloth_params

    sim = fsim.FlingSim(n_envs=episodes, solver=0)
    envs = list(range(episodes))
    for e in envs:
        sim.set_scene(e, cloth_params(64, 64, pos=(0.0, 0.3, 0.0)))
    sim.step(30)                                  # the cloths fall and crumple a little: not one flat square
    for e in envs:
        cp = sim.get_camera_params(e)
        sim.set_camera_params(e, [*cp[2:8], 720, 720])
    times, set_ms, draw_ms = [], [], []
    for k in range(calls + 3):                    # three calls warm up (scratch, work buffers)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if mode == "on":
            t1 = time.perf_counter()
            fresh = [appearance.draw((2, e, k)) for e in envs]
            t2 = time.perf_counter()
            sim.set_appearance(envs, fresh)
            t3 = time.perf_counter()
            draw_ms.append((t2 - t1) * 1e3)
            set_ms.append((t3 - t2) * 1e3)
        sim.observe_batch(envs, 400)              # (ends with the download of the bounding boxes: the device has finished)
        times.append((time.perf_counter() - t0) * 1e3)
    out = dict(mode=mode, ms=float(np.median(times[3:])), min_ms=float(np.min(times[3:])))
    if mode == "on":
        out.update(draw_ms=float(np.median(draw_ms[3:])), set_ms=float(np.median(set_ms[3:])))
    print("RESULT " + json.dumps(out), flush=True)
    sim.close()


def observe_timing(parent_lib, episodes, rounds, calls):
    modes = (["parent"] if parent_lib else []) + ["off", "on"]
    got = {m: [] for m in modes}
    extra = {}
    for r in range(rounds):
        for m in modes:
            env = dict(os.environ)
            env.pop("FLINGSIM_LIB", None)
            if m == "parent":
                env["FLINGSIM_LIB"] = parent_lib
            cmd = [sys.executable, "-W", "ignore", os.path.abspath(__file__), "--child", "off" if m == "parent" else m,
                   "--episodes", str(episodes), "--calls", str(calls)]
            res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            line = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")]
            if res.returncode != 0 or not line:
                print(res.stdout[-2000:], res.stderr[-2000:], flush=True)
                raise SystemExit(f"child {m} failed with status {res.returncode}")     # nothing more is started on the device
            out = json.loads(line[0][7:])
            got[m].append(out["ms"])
            if m == "on":
                extra.setdefault("draw", []).append(out["draw_ms"])
                extra.setdefault("set", []).append(out["set_ms"])
            print(f"  round {r}, {m:<6}: {out['ms']:.3f} ms per observe_batch (min {out['min_ms']:.3f})", flush=True)
    print(f"observe_batch, {episodes} episodes of 64 x 64 cloths, 720^2 -> 400^2, median of {calls} calls per round:")
    for m in modes:
        v = got[m]
        print(f"  {m:<6}: median {np.median(v):.3f} ms  ({', '.join(f'{x:.3f}' for x in v)})  spread {max(v) - min(v):.3f} ms")
    if "parent" in got:
        print(f"  off - parent: {np.median(got['off']) - np.median(got['parent']):+.3f} ms")
    print(f"  on - off: {np.median(got['on']) - np.median(got['off']):+.3f} ms per call, "
          f"{(np.median(got['on']) - np.median(got['off'])) / episodes * 1e3:+.2f} us per observation; inside: "
          f"{episodes} draws {np.median(extra['draw']):.3f} ms, set_appearance {np.median(extra['set']):.3f} ms")


def loop_timing(n_tasks, n_slots, rounds, actions):
    import torch

    from flingbot_amd import nets, sim as fsim, tasks as ftasks
    from flingbot_amd.env import BatchedFlingEnv
    from flingbot_amd.evaluate import run_tasks

    random.seed(1); np.random.seed(1); torch.manual_seed(1)   # noqa: E702
    gen = fsim.FlingSim(n_envs=n_tasks, solver=0)
    tasks = [t for t in ftasks.generate_tasks(gen, [ftasks.draw_task_parameters() for _ in range(n_tasks)]) if t is not None]
    gen.close()
    policy, results = None, {}
    for r in range(rounds + 1):                   # the first round warms up
        for mode in (None, "observation"):
            ctx = fsim.FlingSim(n_envs=n_slots, solver=0)
            env = BatchedFlingEnv(ctx, episode_length=actions, **({} if mode is None else dict(randomize_appearance=mode)))
            if policy is None:
                policy = nets.MaximumValuePolicy(action_primitives=["fling"], num_rotations=12, scale_factors=list(env.scale_factors),
                                                 obs_dim=64, pix_grasp_dist=8, pix_drag_dist=8, pix_place_dist=5, rgb_only=True,
                                                 depth_only=False, action_expl_prob=0.0, action_expl_decay=1.0,
                                                 value_expl_prob=0.0, value_expl_decay=1.0, device="cuda:0")
            t0 = time.perf_counter()
            stats = run_tasks(policy, env, tasks, seed=1)
            dt = time.perf_counter() - t0
            ctx.close()
            flings = int(sum(stats["action_primitive_counts"].values()))
            observations = int(sum(len(rec["actions"]) for rec in stats["records"]))
            if r:
                results.setdefault(mode or "off", []).append((dt, flings, observations))
            print(f"  round {r}{' (warm-up)' if not r else ''}, randomize_appearance {str(mode):<12}: {dt:6.2f} s, {flings} flings "
                  f"({flings / dt:.1f} /s), {stats['simulation_steps']} episode-steps", flush=True)
    print(f"evaluation loop, {len(tasks)} tasks through {n_slots} slots, up to {actions} actions:")
    for mode, v in results.items():
        dts = [x[0] for x in v]
        print(f"  {mode:<12}: median {np.median(dts):.2f} s  ({', '.join(f'{x:.2f}' for x in dts)}), "
              f"{np.median([x[1] / x[0] for x in v]):.1f} flings/s, {v[0][2]} observations with an action")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--child", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--episodes", type=int, default=64)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tasks", type=int, default=96)
    ap.add_argument("--slots", type=int, default=96)
    ap.add_argument("--actions", type=int, default=3)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.episodes, a.calls)
        sys.exit(0)
    if a.parent_lib and not os.path.exists(a.parent_lib):
        raise SystemExit(f"--parent-lib {a.parent_lib}: no such file")
    observe_timing(a.parent_lib, a.episodes, a.rounds, a.calls)
    if a.tasks > 0:
        loop_timing(a.tasks, a.slots, a.rounds, a.actions)
