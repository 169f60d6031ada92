"""What the measured reward maps cost (flingbot_amd/probe.py; EXPERIMENTS.md, measured reward maps).

    python scripts/probe_timing.py [--rounds 5] [--slots 192] [--stride 8] [--example DIR]

1. fs_lattice_actions (ActionSelector.lattice) for 48 observations x a 16 x 16 lattice (stride 3 on the interior of D = 64,
   S = 400), one call, against the host loop over the same cells: `_candidate` plus two `_on_cloth` per cell.
2. report.compose_probe (fs_probe_panels) for 48 strips at panel 200.
3. Probe throughput in executed lane-steps per second at --slots slots: generated hard tasks, --slots // 4 episodes, step 0
   probed at --stride; with --example the first map's strip goes to DIR and its statistics are printed."""
import argparse
import os
import random
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

med = lambda v: float(np.median(v[1:]))   # noqa: E731  (the first round warms up)
fmt = lambda v: ", ".join(f"{x:.2f}" for x in v[1:])   # noqa: E731


def lattice_timing(n=48, rounds=5):
    from flingbot_amd.action import ActionSelector
    from flingbot_amd.env import BatchedFlingEnv

    dev = torch.device("cuda:0")
    D, S, g, stride, radius = 64, 400, 8, 3, 1
    rotations = [(2 * i / 11 - 1) * 90 for i in range(12)]
    scales = np.array([1.0, 1.25, 1.5, 1.75, 2.0, 2.25, 2.5, 2.75]) * 0.6
    sel = ActionSelector(["fling"], rotations, D, g, 8, 5, 1.2)
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:S, 0:S]
    depth = np.full((n, S, S), 2.0, np.float32)
    for e in range(n):
        blob = (xx - S * rng.uniform(0.4, 0.6)) ** 2 + (yy - S * rng.uniform(0.4, 0.6)) ** 2 < (S * rng.uniform(0.1, 0.2)) ** 2
        depth[e][blob] = 1.97
    values = torch.randn((n, 1, 96, D, D), device=dev)
    d_depth = torch.tensor(depth, device=dev)
    requests = [(e, 0, int(rng.integers(0, 96)), g, g, stride, 16, 16) for e in range(n)]
    t_dev = []
    for _ in range(rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        valid, on1, on2, value = sel.lattice(values, [scales] * n, d_depth, requests, radius)
        t_dev.append(1e3 * (time.perf_counter() - t0))
    host = types.SimpleNamespace(conservative_grasp_radius=radius)
    t_host = []
    for _ in range(2):      # the host loop takes seconds: one warm-up, one round
        t0 = time.perf_counter()
        for k, (e, _p, t, y0, z0, _s, gy, gz) in enumerate(requests):
            for i in range(gy):
                for j in range(gz):
                    got = sel._candidate("fling", t, y0 + i * stride, z0 + j * stride, scales, depth[e])
                    ok = got is not None
                    if ok:
                        pix = got["pretransform_pixels"]
                        c1 = BatchedFlingEnv._on_cloth(host, depth[e], (pix[0][1], pix[0][0]))
                        c2 = BatchedFlingEnv._on_cloth(host, depth[e], (pix[1][1], pix[1][0]))
                        assert (c1, c2) == (bool(on1[k, i, j]), bool(on2[k, i, j]))
                    assert ok == bool(valid[k, i, j])
        t_host.append(1e3 * (time.perf_counter() - t0))
    print(f"lattice of 16 x 16 cells for {n} observations, D {D}, S {S}, radius {radius} ({int(valid.sum())} of {valid.size} cells valid):")
    print(f"  one fs_lattice_actions call (ActionSelector.lattice, host clock, ends with its download): {med(t_dev):.2f} ms"
          f"  (rounds: {fmt(t_dev)})")
    print(f"  host loop, _candidate + 2 x _on_cloth per valid cell, the same answers: {t_host[-1]:.0f} ms (one round after a warm-up)"
          f" -> {t_host[-1] / med(t_dev):.0f} x")


def compose_timing(n=48, rounds=5, panel=200):
    from flingbot_amd import report

    dev = torch.device("cuda:0")
    D, S = 64, 400
    rng = np.random.default_rng(1)
    items = []
    for _ in range(n):
        measured = np.where(rng.random((13, 13)) < 0.6, rng.standard_normal((13, 13)), np.nan).astype(np.float32)
        items.append(dict(stack=torch.rand((4, D, D), device=dev), value_map=torch.randn((D, D), device=dev),
                          after=torch.rand((3, S, S), device=dev), measured=torch.tensor(measured, device=dev),
                          valid=torch.ones((13, 13), dtype=torch.uint8, device=dev), range=torch.tensor([-2.0, 2.0], device=dev),
                          origin=(8, 8), stride=4, chosen_cell=(6, 6), small=report.action_overlays("fling", np.array([[40, 32], [24, 32]]), 1)))
    t = []
    for _ in range(rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        strips = report.compose_probe(items, panel=panel)
        t.append(1e3 * (time.perf_counter() - t0))
    print(f"compose_probe, {n} strips at panel {panel} ({strips.nbytes / 1e6:.1f} MB, host clock, with the download): {med(t):.2f} ms"
          f"  (rounds: {fmt(t)})")


def loop_timing(slots, stride, example):
    from flingbot_amd import nets, probe, sim as fsim, tasks as ftasks
    from flingbot_amd.env import BatchedFlingEnv

    random.seed(1); np.random.seed(1); torch.manual_seed(1)
    n = max(1, slots // 4)
    gen = fsim.FlingSim(n_envs=n, solver=0)
    tasks = [t for t in ftasks.generate_tasks(gen, [ftasks.draw_task_parameters() for _ in range(n)]) if t is not None]
    gen.close()
    ctx = fsim.FlingSim(n_envs=slots, solver=0)
    env = BatchedFlingEnv(ctx, episode_length=1)
    policy = nets.MaximumValuePolicy(action_primitives=["fling"], num_rotations=12, scale_factors=list(env.scale_factors),
                                     obs_dim=64, pix_grasp_dist=8, pix_drag_dist=8, pix_place_dist=5, rgb_only=True,
                                     depth_only=False, action_expl_prob=0.0, action_expl_decay=1.0, value_expl_prob=0.0,
                                     value_expl_decay=1.0, device="cuda:0")
    drawing = None if example is None else dict(panel=200, tasks=[0], log=None)
    t0 = time.perf_counter()
    stats = probe.run_episodes(policy, env, tasks, stride, steps=(0,), report=drawing)
    dt = time.perf_counter() - t0
    ctx.close()
    block = stats["probe"]
    free = slots - len(tasks)
    print(f"probe, {len(tasks)} generated hard tasks in {slots} slots ({free} free), stride {stride}, step 0: {dt:.1f} s for "
          f"{block['n_executed']} executed cells + {len(tasks)} followed flings = {(block['n_executed'] + len(tasks)) / dt:.1f} lane-steps/s; "
          f"{block['n_executed'] / len(tasks):.1f} cells per map, {-(-block['n_executed'] // free)} passes")
    print("  means:", {k: v for k, v in block.items() if k not in ("maps", "steps_probed")})
    if example is not None:
        from flingbot_amd import report
        os.makedirs(example, exist_ok=True)
        m = block["maps"][0]
        report.write_png(os.path.join(example, "probe_example.png"), stats["probe_panels"][(0, 0)])
        print("  example map (task 0):", {k: m[k] for k in ("transform_index", "chosen_pixel", "origin", "shape", "n_executed")}, m["stats"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--slots", type=int, default=192)
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--example", default=None, metavar="DIR")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_timing: no GPU (a timing taken elsewhere says nothing)")
    lattice_timing(rounds=a.rounds)
    compose_timing(rounds=a.rounds)
    if a.slots > 0:
        loop_timing(a.slots, a.stride, a.example)
