#!/usr/bin/env python
"""dropin_large_timing.py -- the `pyflex` drop-in at a real task size: bench_dropin.py's `picker` call pattern on a 90 x 90 cloth
(8100 particles: above the 4096 particles of the fused kernels; the size of most of the reference's tasks).

Three configurations, the A/B alternated `--rounds` times in one run:
  1 process, FLINGSIM_SHARED_GPU unset (a lone tenant: AUTO, the streaming kernels);
  16 processes, FLINGSIM_SHARED_GPU=0 (AUTO in every process: streaming);
  16 processes, FLINGSIM_SHARED_GPU=1 (FS_SOLVER_COTENANT: whatever that mode selects for the cloth).
EXPERIMENTS R7.2 used it as the gate of an LDS-resident kernel for such cloths: the co-tenant figure had to reach 2x streaming.
The parent never opens the GPU; at most 16 worker processes run at a time; a configuration whose workers fail ends the run.

    python scripts/dropin_large_timing.py [--steps 150] [--rounds 2]     -> one JSON line (each run also on stderr)
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM = 90


def worker(steps, start_at):
    sys.path.insert(0, os.path.join(ROOT, "flingbot_amd", "pyflex_native"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import pyflex
    import scenarios as sc

    pyflex.init(True, False, 720, 720)
    e_f, e_i = np.zeros(0, np.float32), np.zeros(0, np.int32)
    pyflex.set_scene(0, sc.survey_params(DIM), e_f, e_i, e_i, e_i, e_i, 0)
    pyflex.step()
    pyflex.set_positions(sc.set_to_flatten_positions(DIM, DIM).flatten())
    for c in ((0.04, 0.1, 0.0), (-0.04, 0.1, 0.0)):
        pyflex.add_sphere(0.02, np.array(c), np.array([1., 0., 0., 0.]))
    pyflex.step()
    pyflex.get_positions()
    while time.time() < start_at:
        time.sleep(0.0005)
    t0 = time.time()
    delta = np.array([0.0, 1e-4, 0.0])
    for _ in range(steps):  # bench_dropin.py's picker pattern (Picker._get_pos / _set_pos around pyflex.step)
        picker = np.array(pyflex.get_shape_states()).reshape(-1, 14)
        particles = np.array(pyflex.get_positions()).reshape(-1, 4)
        st = np.array(pyflex.get_shape_states()).reshape(-1, 14)
        st[:, 3:6] = st[:, :3]
        st[:, :3] = picker[:, :3] + delta
        pyflex.set_shape_states(st)
        pyflex.set_positions(particles)
        pyflex.step()
    pyflex.get_positions()
    t1 = time.time()
    print(json.dumps({"steps": steps, "t0": t0, "t1": t1, "backend": pyflex._tenants()[1]}), flush=True)


def run(n_procs, steps, shared_gpu, timeout):
    start_at = time.time() + 8.0 + 0.5 * n_procs
    env = {k: v for k, v in os.environ.items() if k != "FLINGSIM_SHARED_GPU"}
    if shared_gpu is not None:
        env["FLINGSIM_SHARED_GPU"] = shared_gpu
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--steps", str(steps), "--start-at",
                               repr(start_at)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
             for _ in range(n_procs)]
    recs, errs = [], []
    for p in procs:
        try:
            out, err = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            p.kill()
            out, err = p.communicate()
        line = [ln for ln in out.splitlines() if ln.startswith("{")]
        if p.returncode == 0 and line:
            recs.append(json.loads(line[-1]))
        else:
            errs.append((p.returncode, (err or out).strip().splitlines()[-1:]))
    if errs:
        return {"processes": n_procs, "failed": len(errs), "errors": errs[:2]}
    span = max(r["t1"] for r in recs) - min(r["t0"] for r in recs)
    return {"processes": n_procs, "shared_gpu": shared_gpu, "steps_per_s": sum(r["steps"] for r in recs) / span,
            "slowest_process_steps_per_s": min(r["steps"] / (r["t1"] - r["t0"]) for r in recs), "seconds": span,
            "backends": sorted({r["backend"] for r in recs})}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--start-at", type=float, default=0.0)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--timeout", type=float, default=240.0)
    a = ap.parse_args()
    if a.worker:
        worker(a.steps, a.start_at)
        return
    out = []
    for r in range(a.rounds):
        for n, sg in ((1, None), (16, "0"), (16, "1")):
            res = run(n, a.steps, sg, a.timeout)
            res["round"] = r
            out.append(res)
            print(json.dumps(res), file=sys.stderr, flush=True)
            if res.get("failed"):
                print(json.dumps({"error": res}))
                sys.exit(1)
    print(json.dumps({"dim": DIM, "runs": out}))


if __name__ == "__main__":
    main()
