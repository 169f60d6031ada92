"""What the lane report and training on lanes cost (flingbot_amd/report.py compose_lanes, lookahead.py, train.py;
EXPERIMENTS.md, lane report and lane training).

    python scripts/lane_timing.py [--records 48] [--k 4] [--panel 200] [--repeats 5] [--tasks 48] [--slots 192] [--actions 3]
                                  [--train-tasks 48] [--parent DIR]

1. fs_lane_panels for --records records of --k lanes at S = 400: the device window (the table's upload and the launch, torch
   events around the call, the output allocated outside) and report.compose_lanes as a whole, download included (host clock).
2. A look-ahead evaluation (lookahead.run_waves, follow = policy) of --tasks generated hard tasks at --slots slots with the
   lane report off and on, alternately, --repeats times each; the report goes to a temporary directory.
3. One train.run round of --train-tasks tasks with lookahead = --k against one without, on the same tasks, from scratch each.
4. --parent DIR: a built checkout of the parent commit.  The evaluation of 2 with the report off is run alternately from this
   tree and from DIR, one fresh process per run (--one-evaluation is that process), and the two spreads are printed side by
   side: the report-off path gains no launch, so the two must overlap.
Every figure is printed as min .. max over the repeats after one warm-up run."""
import argparse
import json
import os
import random
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def span(values, unit="ms", digits=2):
    return f"{min(values):.{digits}f} .. {max(values):.{digits}f} {unit} (median {float(np.median(values)):.{digits}f}, n = {len(values)})"


def make_policy(env):
    from flingbot_amd import nets
    torch.manual_seed(1)
    return nets.MaximumValuePolicy(action_primitives=["fling"], num_rotations=12, scale_factors=list(env.scale_factors), obs_dim=64,
                                   pix_grasp_dist=8, pix_drag_dist=8, pix_place_dist=5, rgb_only=True, depth_only=False,
                                   action_expl_prob=0.0, action_expl_decay=1.0, value_expl_prob=0.0, value_expl_decay=1.0,
                                   device="cuda:0")


def make_tasks(n):
    from flingbot_amd import sim as fsim, tasks as ftasks
    random.seed(1); np.random.seed(1); torch.manual_seed(1)
    gen = fsim.FlingSim(n_envs=n, solver=0)
    tasks = [t for t in ftasks.generate_tasks(gen, [ftasks.draw_task_parameters() for _ in range(n)]) if t is not None]
    gen.close()
    return tasks


def panels_timing(records, k, panel, repeats, S=400):
    from flingbot_amd import report
    from flingbot_amd.sim import stream_call, work_buffer

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    items = []
    for _ in range(records):
        lanes = []
        for _j in range(k):
            pix = rng.integers(S // 8, S - S // 8, (2, 2))
            lanes.append(dict(after=torch.rand((3, S, S), device=dev), prims=report.action_overlays("fling", pix, thickness=3)))
        items.append(dict(before=torch.rand((3, S, S), device=dev), lanes=lanes, followed=int(rng.integers(0, k))))
    table = np.zeros(records, report.LANE_RECORD)
    for n, it in enumerate(items):
        row = table[n]
        row["before"], row["n_lanes"], row["followed"] = it["before"].data_ptr(), k, it["followed"]
        for j, lane in enumerate(it["lanes"]):
            row["after"][j], row["n_prims"][j] = lane["after"].data_ptr(), len(lane["prims"])
            row["prims"][j, :len(lane["prims"])] = lane["prims"]
    out = torch.empty((records, panel, (1 + k) * panel, 3), dtype=torch.uint8, device=dev)
    work = work_buffer("fs_lane_panels_work_bytes", dev, records)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    window, whole = [], []
    for r in range(repeats + 1):           # the first round warms up
        torch.cuda.synchronize()
        start.record()
        stream_call("fs_lane_panels", dev, table.ctypes.data, records, k, S, panel, out, work)
        stop.record()
        stop.synchronize()
        window.append(start.elapsed_time(stop))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        strips = report.compose_lanes(items, k, panel=panel)
        whole.append(1e3 * (time.perf_counter() - t0))
    assert (strips == out.cpu().numpy()).all()
    written = out.numel()
    print(f"fs_lane_panels, {records} records x {k} lanes, S {S}, panel {panel}: {written / 1e6:.1f} MB of strips")
    print(f"  upload of the table + launch (device events): {span(window[1:], digits=3)} -> {written / min(window[1:]) / 1e6:.0f} GB/s written at best")
    print(f"  report.compose_lanes, download included (host clock): {span(whole[1:])}", flush=True)


def one_evaluation(tasks, slots, k, actions, report_root=None, panel=200):
    """Seconds of one lookahead.run_waves over `tasks` on a fresh context, and its statistics."""
    from flingbot_amd import lookahead, sim as fsim
    from flingbot_amd.env import BatchedFlingEnv

    ctx = fsim.FlingSim(n_envs=slots, solver=0)
    kwargs = {} if report_root is None else dict(action_report=True, report_root=report_root, report_panel=panel)
    env = BatchedFlingEnv(ctx, episode_length=actions, **kwargs)
    policy = make_policy(env)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stats = lookahead.run_waves(policy, env, tasks, k, follow="policy")
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ctx.close()
    return dt, stats


def evaluation_timing(tasks, slots, k, actions, repeats, panel):
    off, on, strips = [], [], 0
    for r in range(repeats + 1):           # the first pair warms up
        dt, plain = one_evaluation(tasks, slots, k, actions)
        off.append(dt)
        with tempfile.TemporaryDirectory() as root:
            dt, drawn = one_evaluation(tasks, slots, k, actions, report_root=root, panel=panel)
            strips = sum(f.endswith(".png") for _, _, files in os.walk(root) for f in files)
        on.append(dt)
        assert np.array_equal(plain["coverage_steps"], drawn["coverage_steps"])
    look = plain["lookahead"]
    print(f"look-ahead evaluation, {len(tasks)} hard tasks, {slots} slots, k = {k}, up to {actions} actions: {look['n_steps']} steps, "
          f"{look['n_lane_steps']} lane-steps, {strips} strips of panel {panel}")
    print(f"  report off: {span(off[1:], 's')}")
    print(f"  report on:  {span(on[1:], 's')}", flush=True)


def train_timing(tasks, slots, k, actions, repeats):
    from flingbot_amd import sim as fsim, train
    from flingbot_amd.env import BatchedFlingEnv

    rows = {None: [], k: []}
    entries = {}
    for r in range(repeats + 1):
        for lanes in (None, k):
            ctx = fsim.FlingSim(n_envs=slots if lanes is not None else min(slots, len(tasks)), solver=0)
            env = BatchedFlingEnv(ctx, episode_length=actions, record_experience=True)
            policy = make_policy(env)
            opt = train.make_optimizer(policy, hip=True)
            with tempfile.TemporaryDirectory() as log_dir:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = train.run(policy, opt, env, tasks, log_dir, rounds=1, tasks_per_round=len(tasks), seed=0, batch_size=32, warmup=32,
                                hip_step=True, lookahead=lanes)
                torch.cuda.synchronize()
                rows[lanes].append(time.perf_counter() - t0)
            entries[lanes] = (out["rounds"][0]["new_entries"], out["rounds"][0]["updates"])
            ctx.close()
    print(f"one train.run round, {len(tasks)} hard tasks, up to {actions} actions, batch 32, warm-up 32, hip_step:")
    print(f"  without lanes:  {span(rows[None][1:], 's')}, {entries[None][0]} entries, {entries[None][1]} updates")
    print(f"  lookahead = {k}:  {span(rows[k][1:], 's')}, {entries[k][0]} entries, {entries[k][1]} updates", flush=True)


def parent_comparison(parent, a):
    """The report-off evaluation alternately from this tree and from the parent's, one fresh process each."""
    times = {"this tree": [], "parent": []}
    for r in range(a.repeats + 1):
        for name, tree in (("this tree", ROOT), ("parent", os.path.abspath(parent))):
            cmd = [sys.executable, os.path.abspath(__file__), "--one-evaluation", "--tree", tree, "--tasks", str(a.tasks), "--slots", str(a.slots),
                   "--k", str(a.k), "--actions", str(a.actions)]
            got = subprocess.run(cmd, check=True, capture_output=True, text=True, cwd=tree).stdout.strip().splitlines()[-1]
            times[name].append(json.loads(got)["seconds"])
            print(f"  run {r}, {name}: {got}", flush=True)
    print(f"look-ahead evaluation with the report off, {a.tasks} tasks, {a.slots} slots, k = {a.k}, one process per run, alternately:")
    for name, v in times.items():
        print(f"  {name:<10} {span(v[1:], 's')}  (runs: {', '.join(f'{x:.2f}' for x in v[1:])})", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--records", type=int, default=48)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--panel", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tasks", type=int, default=48)
    ap.add_argument("--slots", type=int, default=192)
    ap.add_argument("--actions", type=int, default=3)
    ap.add_argument("--train-tasks", type=int, default=48)
    ap.add_argument("--parent", default=None, metavar="DIR")
    ap.add_argument("--skip", nargs="*", default=[], choices=["panels", "evaluation", "train"])
    ap.add_argument("--one-evaluation", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    sys.path.insert(0, a.tree)
    if not torch.cuda.is_available():
        raise SystemExit("lane_timing: no GPU (a timing taken elsewhere says nothing)")
    if a.one_evaluation:
        seconds, stats = one_evaluation(make_tasks(a.tasks), a.slots, a.k, a.actions)
        print(json.dumps(dict(seconds=seconds, n_lane_steps=stats["lookahead"]["n_lane_steps"],
                              final_coverage=stats["mean"]["final_coverage"])))
        raise SystemExit(0)
    if "panels" not in a.skip:
        panels_timing(a.records, a.k, a.panel, a.repeats)
    if "evaluation" not in a.skip:
        evaluation_timing(make_tasks(a.tasks), a.slots, a.k, a.actions, a.repeats, a.panel)
    if "train" not in a.skip:
        train_timing(make_tasks(a.train_tasks), a.slots, a.k, a.actions, a.repeats)
    if a.parent:
        parent_comparison(a.parent, a)
