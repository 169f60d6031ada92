"""What the action report costs (flingbot_amd/report.py; EXPERIMENTS.md, action reports).

    python scripts/report_timing.py [--actions 192] [--panel 200] [--tasks 384] [--slots 192] [--repeats 2] [--sample out.png]

1. One `report.compose` call for --actions actions at the defaults (D 64, S 400): the entry point between device events (the
   table upload and fs_k_action_panels; ten calls back to back, per call), the whole call on the host clock (plus the
   download of the strips), and fs_value_range over as many [96, 64, 64] map stacks: ten calls back to back between device
   events, and the `report.value_range` wrapper on the host clock.
2. The evaluation loop at the size of bench.py --full's `continuous` figure (--tasks generated hard tasks through --slots
   slots, up to 3 actions each) with reporting off / on, strips kept in memory / on, strips written as PNG files --
   alternated, --repeats rounds, one task set.  The statistics of all runs must be equal.
--sample writes the first composed strip of part 2 as a PNG (to look at)."""
import argparse
import os
import random
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def compose_timing(n_actions, panel, rounds=5):
    from flingbot_amd import report
    from flingbot_amd.sim import stream_call, work_buffer

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    D, S = 64, 400
    stacks = torch.rand((n_actions, 4, D, D), device=dev, generator=g)
    maps = torch.randn((n_actions, 96, D, D), device=dev, generator=g)
    before = torch.rand((n_actions, 3, S, S), device=dev, generator=g)
    after = torch.rand((n_actions, 3, S, S), device=dev, generator=g)
    small = report.action_overlays("fling", np.array([[24, 30], [40, 30]]), 1)
    large = report.action_overlays("fling", np.array([[150, 190], [250, 190]]), 3)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    range_ms, range_call_ms, launch_ms, call_ms = [], [], [], []
    REPEAT = 10
    range_items = np.zeros(n_actions, report.RANGE_ITEM)
    for k in range(n_actions):
        range_items[k] = (maps[k].data_ptr(), maps[k].numel())
    range_out = torch.empty((n_actions, 2), dtype=torch.float32, device=dev)
    for _ in range(rounds + 1):          # the first round warms up
        # the kernel: REPEAT calls of the entry point queued back to back between two events (the table is built beforehand:
        # with one call between the events the device waits for the host and the figure is the host's)
        start.record()
        for _r in range(REPEAT):
            stream_call("fs_value_range", dev, range_items.ctypes.data, n_actions, range_out)
        stop.record()
        stop.synchronize()
        range_ms.append(start.elapsed_time(stop) / REPEAT)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ranges = report.value_range([maps[k] for k in range(n_actions)])
        torch.cuda.synchronize()
        range_call_ms.append(1e3 * (time.perf_counter() - t0))
        assert (ranges == range_out).all()
        items = [dict(stack=stacks[k], value_map=maps[k, 5], range=ranges[k], before=before[k], after=after[k], small=small,
                      large=large) for k in range(n_actions)]
        t0 = time.perf_counter()
        strips = report.compose(items, panel=panel)
        call_ms.append(1e3 * (time.perf_counter() - t0))
        # the launch alone: compose's own table, uploaded and composed between two events
        table = np.zeros(n_actions, report.PANEL_RECORD)
        for k, it in enumerate(items):
            row = table[k]
            row["stack"], row["value_map"], row["range"] = it["stack"].data_ptr(), it["value_map"].data_ptr(), it["range"].data_ptr()
            row["before"], row["after"] = it["before"].data_ptr(), it["after"].data_ptr()
            row["n_small"], row["n_large"] = len(small), len(large)
            row["small"][:len(small)], row["large"][:len(large)] = small, large
        out = torch.empty((n_actions, panel, 5 * panel, 3), dtype=torch.uint8, device=dev)
        work = work_buffer("fs_action_panels_work_bytes", dev, n_actions)
        start.record()
        for _r in range(REPEAT):     # (every call uploads its table and waits for that: the host's checks are inside the figure)
            stream_call("fs_action_panels", dev, table.ctypes.data, n_actions, D, S, panel, out, work)
        stop.record()
        stop.synchronize()
        launch_ms.append(start.elapsed_time(stop) / REPEAT)
        assert (out.cpu().numpy() == strips).all()
    nbytes = strips.nbytes
    med = lambda v: float(np.median(v[1:]))   # noqa: E731
    print(f"compose, {n_actions} actions, panel {panel}, D {D}, S {S}: {nbytes / 1e6:.1f} MB of strips")
    print(f"  fs_value_range over {n_actions} x [96, 64, 64] (device events, {REPEAT} calls back to back, per call): {med(range_ms):.3f} ms"
          f" -> {maps.numel() * 4 / med(range_ms) / 1e6:.0f} GB/s read  (rounds: {', '.join(f'{v:.3f}' for v in range_ms[1:])})")
    print(f"  report.value_range, host clock, synchronised: {med(range_call_ms):.3f} ms  (rounds: "
          f"{', '.join(f'{v:.3f}' for v in range_call_ms[1:])})")
    print(f"  table upload + fs_k_action_panels (device events, {REPEAT} calls, per call): {med(launch_ms):.3f} ms -> {nbytes / med(launch_ms) / 1e6:.1f} GB/s written"
          f"  (rounds: {', '.join(f'{v:.3f}' for v in launch_ms[1:])})")
    print(f"  report.compose, host clock, with the download: {med(call_ms):.1f} ms  (rounds: {', '.join(f'{v:.1f}' for v in call_ms[1:])})")


def loop_timing(n_tasks, n_slots, repeats, sample):
    from flingbot_amd import nets, report, sim as fsim, tasks as ftasks
    from flingbot_amd.env import BatchedFlingEnv
    from flingbot_amd.evaluate import run_tasks

    random.seed(1); np.random.seed(1); torch.manual_seed(1)
    tasks = []
    for k in range(0, n_tasks, n_slots):
        part = [ftasks.draw_task_parameters() for _ in range(min(n_slots, n_tasks - k))]
        gen = fsim.FlingSim(n_envs=len(part), solver=0)
        tasks += [t for t in ftasks.generate_tasks(gen, part) if t is not None]
        gen.close()
    policy = None
    results, first = {}, None
    stamps = dict(compose=0.0, look=0.0, png=0.0)
    for r in range(repeats):
        for mode in ("off", "memory", "png"):
            root = tempfile.mkdtemp(prefix="report_timing_") if mode == "png" else None
            ctx = fsim.FlingSim(n_envs=n_slots, solver=0)
            env = BatchedFlingEnv(ctx, episode_length=3, **({} if mode == "off" else dict(action_report=True, report_root=root)))
            if policy is None:
                policy = nets.MaximumValuePolicy(action_primitives=["fling"], num_rotations=12, scale_factors=list(env.scale_factors),
                                                 obs_dim=64, pix_grasp_dist=8, pix_drag_dist=8, pix_place_dist=5, rgb_only=True,
                                                 depth_only=False, action_expl_prob=0.0, action_expl_decay=1.0,
                                                 value_expl_prob=0.0, value_expl_decay=1.0, device="cuda:0")
            if mode != "off":        # where the host time of reporting goes
                def timed(fn, name):
                    def wrapper(*a, **kw):
                        t0 = time.perf_counter()
                        out = fn(*a, **kw)       # (both services end with a download: the host clock sees the device's part)
                        stamps[name] += time.perf_counter() - t0
                        return out
                    return wrapper
                env.compose_reports = timed(env.compose_reports, "compose")
                env.look_batch = timed(env.look_batch, "look")
                if env._report_log.root is not None:
                    env._report_log.write = timed(env._report_log.write, "png")
                for k in stamps:
                    stamps[k] = 0.0
            t0 = time.perf_counter()
            stats = run_tasks(policy, env, tasks)
            dt = time.perf_counter() - t0
            ctx.close()
            flings = int(sum(stats["action_primitive_counts"].values()))
            key = (stats["simulation_steps"], flings, tuple(np.round(stats["final_coverage"], 12)))
            first = key if first is None else first
            assert key == first, "reporting changed the run"
            extra = ""
            if mode != "off":
                extra = "  [inside: " + ", ".join(f"{k} {v:.2f} s" for k, v in stamps.items() if v) + "]"
            if mode == "memory" and sample and r == 0:
                strip = next(p for rec in stats["records"] for p in rec.get("panels", []) if p is not None)
                report.write_png(sample, strip)
            if root is not None:
                shutil.rmtree(root, ignore_errors=True)
            results.setdefault(mode, []).append(dt)
            print(f"  round {r}, reporting {mode:<6}: {dt:6.2f} s, {flings} flings ({flings / dt:.1f} /s), "
                  f"{stats['simulation_steps']} episode-steps{extra}", flush=True)
    print(f"evaluation loop, {len(tasks)} tasks through {n_slots} slots, up to 3 actions:")
    for mode, v in results.items():
        print(f"  reporting {mode:<6}: median {np.median(v):.2f} s  ({', '.join(f'{x:.2f}' for x in v)})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--actions", type=int, default=192)
    ap.add_argument("--panel", type=int, default=200)
    ap.add_argument("--tasks", type=int, default=384)
    ap.add_argument("--slots", type=int, default=192)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--sample", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("report_timing: no GPU (a timing taken elsewhere says nothing)")
    compose_timing(a.actions, a.panel)
    if a.tasks > 0:
        loop_timing(a.tasks, a.slots, a.repeats, a.sample)
