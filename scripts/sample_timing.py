"""What sampled look-ahead lanes cost (flingbot_amd/action.py `sampled`, fs_sample_actions; EXPERIMENTS.md, sampled lanes).

    python scripts/sample_timing.py [--rounds 5] [--tasks 8] [--slots 32] [--actions 3] [--parent DIR [--parent-rounds 5]]
                                    [--skip-selector] [--skip-loop] [--out FILE]

Every time is a host clock around work that ends with the call's own download (a device synchronise); the first round of every
shape warms up and is dropped, the rest are listed so that the spread can be seen.  Nothing here says anything about what
sampled lanes do to a trained policy.

1. ActionSelector.sampled against ActionSelector.candidates, and the entry point fs_sample_actions (ActionSelector.sample)
   alone, at 96 transforms, D = 64, S = 400, n in {1, 48, 192} observations and k in {1, 4, 8}.
2. One look-ahead evaluation with k = 4 on generated tasks, lanes="sampled" against lanes="winners", alternating, in one
   process.
3. With --parent DIR (a built checkout of the commit before sampled lanes): `python -m flingbot_amd.evaluate --lookahead 4`
   with no new flag, alternately from DIR and from this tree, --parent-rounds times each, on one task file and one file of
   weights.  The JSON lines must be byte-identical, and this tree's median time must not exceed the parent's slowest run (a
   whole-process wall time carries the start of the interpreter and the import of torch, a tenth of a second of jitter: single
   runs are listed, the median is what is compared; faster than the parent's fastest run is no failure).  The script exits
   with status 1 if either fails."""
import argparse
import os
import random
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def selector_timing(rounds, say):
    from flingbot_amd.action import ActionSelector, gumbel_table

    dev = torch.device("cuda:0")
    D, S, g = 64, 400, 8
    rotations = [(2 * i / 11 - 1) * 90 for i in range(12)]
    scales = np.array([1.0, 1.25, 1.5, 1.75, 2.0, 2.25, 2.5, 2.75]) * 0.6
    sel = ActionSelector(["fling"], rotations, D, g, 8, 5, 1.2)
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:S, 0:S]
    n_max = 192
    depth = np.full((n_max, S, S), 2.0, np.float32)
    for e in range(n_max):
        blob = (xx - S * rng.uniform(0.4, 0.6)) ** 2 + (yy - S * rng.uniform(0.4, 0.6)) ** 2 < (S * rng.uniform(0.1, 0.2)) ** 2
        depth[e][blob] = 1.97
    values_all = torch.randn((n_max, 1, 96, D, D), device=dev) * 0.05
    depth_all = torch.tensor(depth, device=dev)
    noise = gumbel_table(dev)
    med = lambda v: float(np.median(v[1:]))   # noqa: E731
    fmt = lambda v: ", ".join(f"{x:.2f}" for x in v[1:])   # noqa: E731
    say(f"action selection over 96 maps, D {D}, S {S}, temperature 0.05, on-cloth radius 1 (host clock; every call ends with its "
        f"download; ms, median of {rounds} rounds after one warm-up)")
    for n in (1, 48, 192):
        values, d_depth = values_all[:n], depth_all[:n]
        keys = np.arange(2 * n, dtype=np.uint32).reshape(n, 2)
        host_depth, dev_depth = list(depth[:n]), list(d_depth)
        for k in (1, 4, 8):
            t_entry, t_sampled, t_cands = [], [], []
            for _ in range(rounds + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sel.sample(values, [scales] * n, d_depth, min(16, k + 4), keys, 20.0, noise, radius=1)
                t_entry.append(1e3 * (time.perf_counter() - t0))
                t0 = time.perf_counter()
                drawn = sel.sampled(values, [scales] * n, host_depth, k, keys, 0.05, depth_device=dev_depth, radius=1)
                t_sampled.append(1e3 * (time.perf_counter() - t0))
                t0 = time.perf_counter()
                best = sel.candidates(values, [scales] * n, host_depth, k, depth_device=dev_depth)
                t_cands.append(1e3 * (time.perf_counter() - t0))
            assert all(a[0][1]["flat_index"] == b[0][1]["flat_index"] for a, b in zip(drawn, best) if a and b)
            say(f"  n {n:3d} k {k}: fs_sample_actions ({min(16, k + 4)} picks) {med(t_entry):7.2f} | sampled {med(t_sampled):7.2f} | "
                f"candidates {med(t_cands):7.2f} | sampled / candidates {med(t_sampled) / med(t_cands):.2f}   "
                f"(rounds: {fmt(t_entry)} | {fmt(t_sampled)} | {fmt(t_cands)}); found {sum(len(c) for c in drawn)} / "
                f"{sum(len(c) for c in best)} of {n * k}")


def make_tasks(n, slots):
    from flingbot_amd import sim as fsim, tasks as ftasks

    random.seed(1); np.random.seed(1); torch.manual_seed(1)   # noqa: E702
    gen = fsim.FlingSim(n_envs=slots, solver=0)
    tasks = [t for t in ftasks.generate_tasks(gen, [ftasks.draw_task_parameters() for _ in range(n)]) if t is not None]
    gen.close()
    return tasks


def loop_timing(tasks, slots, actions, rounds, say):
    from flingbot_amd import lookahead, nets, sim as fsim
    from flingbot_amd.env import BatchedFlingEnv

    policy, times = None, {"winners": [], "sampled": []}
    say(f"look-ahead evaluation, {len(tasks)} generated tasks, k = 4, {slots} slots, up to {actions} actions, seed 1 (s, whole call):")
    for _ in range(rounds + 1):
        for lanes in ("winners", "sampled"):
            ctx = fsim.FlingSim(n_envs=slots, solver=0)
            env = BatchedFlingEnv(ctx, episode_length=actions)
            if policy is None:
                policy = nets.MaximumValuePolicy(action_primitives=["fling"], num_rotations=12, scale_factors=list(env.scale_factors),
                                                 obs_dim=64, pix_grasp_dist=8, pix_drag_dist=8, pix_place_dist=5, rgb_only=True,
                                                 depth_only=False, action_expl_prob=0.0, action_expl_decay=1.0,
                                                 value_expl_prob=0.0, value_expl_decay=1.0, device="cuda:0")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stats = lookahead.run_waves(policy, env, tasks, 4, follow="policy", seed=1, lanes=lanes, lane_temperature=0.05)
            torch.cuda.synchronize()
            times[lanes].append(time.perf_counter() - t0)
            ctx.close()
            look = stats["lookahead"]
            last = (f"{look['n_lane_steps']} lane-steps, regret {look['regret']:.4f}, mean reward per rank "
                    + " / ".join("-" if v is None else f"{v:+.4f}" for v in look["mean_reward_per_rank"])
                    + (f", refused {look['refused']}" if lanes == "sampled" else ""))
            times[lanes + " last"] = last
    for lanes in ("winners", "sampled"):
        t = times[lanes][1:]
        say(f"  lanes={lanes:<8} median {np.median(t):6.2f}  (rounds: {', '.join(f'{x:.2f}' for x in t)}); {times[lanes + ' last']}")
    say(f"  sampled / winners: {np.median(times['sampled'][1:]) / np.median(times['winners'][1:]):.3f}")


def parent_comparison(parent, tasks, slots, actions, rounds, out_dir, say):
    """The unchanged command line from the parent's tree and from this one, alternating.  True when the JSON lines are
    byte-identical and this tree's median time does not exceed the parent's slowest run."""
    from flingbot_amd import nets, taskio

    path, weights = os.path.join(out_dir, "sample_timing_tasks.npz"), os.path.join(out_dir, "sample_timing_weights.pth")
    taskio.save_tasks(path, tasks)
    torch.manual_seed(1)   # one set of (untrained) weights for every process: fresh ones would execute different flings
    policy = nets.MaximumValuePolicy(action_primitives=["fling"], num_rotations=12, scale_factors=[1.0], obs_dim=64,
                                     pix_grasp_dist=8, pix_drag_dist=8, pix_place_dist=5, rgb_only=True, depth_only=False,
                                     action_expl_prob=0.0, action_expl_decay=1.0, value_expl_prob=0.0, value_expl_decay=1.0,
                                     device="cuda:0")
    torch.save(policy.state_dict(), weights)
    cmd = [sys.executable, "-m", "flingbot_amd.evaluate", "--tasks", path, "--weights", weights, "--lookahead", "4", "--slots",
           str(slots), "--episode-length", str(actions), "--seed", "1"]
    lines, times = {"parent": [], "this": []}, {"parent": [], "this": []}
    for _ in range(rounds):
        for name, cwd in (("parent", parent), ("this", ROOT)):
            env = dict(os.environ, PYTHONPATH=cwd)
            t0 = time.perf_counter()
            done = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
            times[name].append(time.perf_counter() - t0)
            if done.returncode != 0:
                say(f"  {name}: exit status {done.returncode}\n{done.stderr[-2000:]}")
                return False
            lines[name].append([ln for ln in done.stdout.splitlines() if ln.startswith("{")][-1])
    same = len(set(lines["parent"] + lines["this"])) == 1
    lo, hi = min(times["parent"]), max(times["parent"])
    inside = float(np.median(times["this"])) <= hi
    say(f"`evaluate --weights W --lookahead 4 --slots {slots} --episode-length {actions} --seed 1`, no new flag, whole command (s):")
    say(f"  parent: {', '.join(f'{t:.2f}' for t in times['parent'])}   this tree: {', '.join(f'{t:.2f}' for t in times['this'])}")
    say(f"  JSON lines byte-identical: {same} ({len(lines['this'][0])} bytes); medians {np.median(times['parent']):.2f} / "
        f"{np.median(times['this']):.2f}; this tree's median within the parent's spread [{lo:.2f}, {hi:.2f}]: {inside}")
    if not same:
        say("  parent: " + lines["parent"][0][:600])
        say("  this:   " + lines["this"][0][:600])
    return same and inside


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tasks", type=int, default=8)
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--actions", type=int, default=3)
    ap.add_argument("--parent", default=None, metavar="DIR", help="a built checkout of the parent commit")
    ap.add_argument("--parent-rounds", type=int, default=5)
    ap.add_argument("--skip-selector", action="store_true", help="leave part 1 out")
    ap.add_argument("--skip-loop", action="store_true", help="leave part 2 out")
    ap.add_argument("--out", default=None, metavar="FILE", help="also append every line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_timing: no GPU (a timing taken elsewhere says nothing)")

    def say(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(line + "\n")

    if not a.skip_selector:
        selector_timing(a.rounds, say)
    ok = True
    if a.tasks > 0:
        made = make_tasks(a.tasks, a.slots)
        if not a.skip_loop:
            loop_timing(made, a.slots, a.actions, min(a.rounds, 2), say)
        if a.parent:
            ok = parent_comparison(os.path.abspath(a.parent), made, a.slots, a.actions, a.parent_rounds,
                                   os.path.dirname(os.path.abspath(a.out)) if a.out else os.getcwd(), say)
    sys.exit(0 if ok else 1)
