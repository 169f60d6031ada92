"""What the look-ahead rollouts cost (flingbot_amd/lookahead.py; EXPERIMENTS.md, look-ahead rollouts).

    python scripts/lookahead_timing.py [--trunks 48] [--lanes 3] [--rounds 5] [--slots 192] [--k 4] [--actions 3]

1. The fork launch: --trunks crumpled grid cloths (64 x 64, then 104 x 104, two pickers each) forked into --lanes fresh
   slots each by ONE fs_fork call.  The device window is taken with the context's HIP events while the device is kept busy
   in front of the call (one small episode stepped for many frames by the fused back-end, ONE launch: on an idle device the
   start event completes at once and the window would hold the call's host work as well); the call's host time is taken too.  Next to
   it a `torch` device-to-device copy of as many bytes as the fork WRITES, timed in the same process with torch's events,
   ten copies back to back.
2. fs_transform_winners for 48 observations x 96 maps at D = 64 (one call) against 48 fs_select_action calls (the parent's
   path, one call per observation), entry points alone and with the host validation of `select` / `candidates`.
3. Look-ahead flings per second at --slots slots with k = --k, next to the plain lock-step evaluate.run_episodes at --slots
   slots, on generated hard tasks, up to --actions actions."""
import argparse
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

PER_PARTICLE = 16 + 16 + 4 + 4      # position, velocity, phase, saved inverse mass


def fork_timing(dim, trunks, lanes, rounds):
    from flingbot_amd import sim as fsim
    from scenarios import cloth_params

    n_dst = trunks * lanes
    blocker = trunks + n_dst * (rounds + 1)          # one more slot: the episode that keeps the device busy
    sim = fsim.FlingSim(n_envs=blocker + 1, solver=0)
    src = list(range(trunks))
    for e in src:
        sim.set_scene(e, cloth_params(dim, dim))
        for c in ([0.5, 0.5, -0.5], [-0.5, 0.5, -0.5]):
            sim.add_sphere(e, 0.02, c, [1, 0, 0, 0])
        sim.picker_reset(e, 0.005, 0.00625, picker_radius=0.02)
    sim.step_list(src, 5)
    # A launch sequence of the streaming back-end is ~130 launches per frame and the device finishes them as fast as the host
    # queues them: it cannot keep the stream busy.  The fused back-end runs ALL frames of a call in one launch, so one small
    # episode stepped for many frames by it blocks the context's stream for as long as the host needs.
    sim.set_scene(blocker, cloth_params(32, 32))
    sim.set_solver(fsim.FS_SOLVER_FUSED)
    sim.timer_start()
    sim.step_list([blocker], 20)
    frame_ms = sim.timer_stop() / 20
    sim.set_solver(fsim.FS_SOLVER_AUTO)
    n = sim.n_particles(0)
    written = n_dst * n * PER_PARTICLE
    moved = written + trunks * n * PER_PARTICLE
    window_ms, host_ms = [], []
    busy = 20
    for r in range(rounds + 1):            # the first round warms up (tables, and it measures the call's host time)
        dst = [trunks + r * n_dst + k for k in range(n_dst)]
        pairs_src = [s for s in src for _ in range(lanes)]
        sim.sync()
        sim.set_solver(fsim.FS_SOLVER_FUSED)
        sim.step_list([blocker], busy)     # one launch: the device is busy while the host prepares and queues the fork
        sim.set_solver(fsim.FS_SOLVER_AUTO)
        sim.timer_start()
        t0 = time.perf_counter()
        sim.fork(pairs_src, dst)
        host_ms.append(1e3 * (time.perf_counter() - t0))
        window_ms.append(sim.timer_stop())
        busy = max(20, int(np.ceil(2.0 * host_ms[-1] / frame_ms)))
    for s, d in zip(pairs_src[::lanes], dst[::lanes]):   # the copies are copies
        assert np.array_equal(sim.get_positions(s).view(np.uint32), sim.get_positions(d).view(np.uint32))
    sim.close()
    # the same bytes written by torch: ten copies back to back between two events
    dev = torch.device("cuda:0")
    a = torch.empty(written, dtype=torch.uint8, device=dev).random_(0, 255)
    b = torch.empty_like(a)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    copy_ms = []
    for _ in range(rounds + 1):
        start.record()
        for _r in range(10):
            b.copy_(a)
        stop.record()
        stop.synchronize()
        copy_ms.append(start.elapsed_time(stop) / 10)
    med = lambda v: float(np.median(v[1:]))   # noqa: E731
    fmt = lambda v: ", ".join(f"{x:.3f}" for x in v[1:])   # noqa: E731
    f_ms, c_ms = med(window_ms), med(copy_ms)
    print(f"fs_fork, {trunks} trunks of {dim} x {dim} -> {lanes} lanes each: {written / 1e6:.1f} MB written, {moved / 1e6:.1f} MB moved")
    print(f"  device window (upload of the tables + fs_k_fork): {f_ms:.3f} ms -> {moved / f_ms / 1e6:.0f} GB/s moved, "
          f"{written / f_ms / 1e6:.0f} GB/s written  (rounds: {fmt(window_ms)})")
    print(f"  torch copy of {written / 1e6:.1f} MB, device events, per copy: {c_ms:.3f} ms -> {2 * written / c_ms / 1e6:.0f} GB/s moved, "
          f"{written / c_ms / 1e6:.0f} GB/s written  (rounds: {fmt(copy_ms)})")
    print(f"  bytes moved per second, fork / torch copy: {(moved / f_ms) / (2 * written / c_ms):.2f}; bytes written per second: "
          f"{c_ms / f_ms:.2f}")
    print(f"  the call on the host clock, until it returns (the device busy behind it: {busy} frames of {frame_ms:.2f} ms in one launch): "
          f"{med(host_ms):.1f} ms = {1e3 * med(host_ms) / n_dst:.0f} us per destination  (rounds: {fmt(host_ms)})")


def winners_timing(n=48, rounds=5):
    import ctypes as C

    from flingbot_amd.action import CAMERA_FOV_DEG, KINDS, ActionSelector, compute_intrinsics
    from flingbot_amd.sim import stream_call, work_buffer

    dev = torch.device("cuda:0")
    D, S, g = 64, 400, 8
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
    mats = sel._transform_mats(S, D, scales)
    kinds = np.array([KINDS["fling"]], np.int32)
    fx = float(compute_intrinsics(CAMERA_FOV_DEG, S)[0, 0])
    dp = C.POINTER(C.c_double)
    pose = np.ascontiguousarray(sel.pose)
    work = work_buffer("fs_select_action_work_bytes", dev, 96)
    t_entry, t_select, t_winners, t_cands = [], [], [], []
    for _ in range(rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        singles = []
        for e in range(n):
            best, bval = C.c_longlong(-1), C.c_float(0.0)
            stream_call("fs_select_action", dev, values[e], 1, kinds.ctypes.data_as(C.POINTER(C.c_int)), 96, D, g, 8, 5,
                        mats.ctypes.data_as(dp), d_depth[e], S, fx, pose.ctypes.data_as(dp), sel.left_arm_base.ctypes.data_as(dp),
                        sel.right_arm_base.ctypes.data_as(dp), 1.2, 0.3, 0.02, C.byref(best), C.byref(bval), work)
            singles.append(int(best.value))
        t_entry.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        chosen = [sel.select(values[e], scales, depth[e], depth_device=d_depth[e]) for e in range(n)]
        t_select.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        index, value = sel.winners(values, [scales] * n, d_depth)
        t_winners.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        cands = sel.candidates(values, [scales] * n, list(depth), 4, depth_device=list(d_depth))
        t_cands.append(1e3 * (time.perf_counter() - t0))
        for e in range(n):      # the best winner of an observation is fs_select_action's answer
            live = [i for i in range(96) if index[e, 0, i] >= 0]
            best = min(live, key=lambda i: (-float(value[e, 0, i]), int(index[e, 0, i]))) if live else None
            assert singles[e] == (-1 if best is None else int(index[e, 0, best]))
            assert (chosen[e][1] or {}).get("flat_index", -1) == singles[e] == (cands[e][0][1]["flat_index"] if cands[e] else -1)
    med = lambda v: float(np.median(v[1:]))   # noqa: E731
    fmt = lambda v: ", ".join(f"{x:.2f}" for x in v[1:])   # noqa: E731
    print(f"action selection for {n} observations x 96 maps, D {D}, S {S} (host clock, synchronised; every call ends with its download):")
    print(f"  {n} fs_select_action calls: {med(t_entry):.2f} ms  (rounds: {fmt(t_entry)})")
    print(f"  one fs_transform_winners call (ActionSelector.winners): {med(t_winners):.2f} ms  (rounds: {fmt(t_winners)})"
          f" -> {med(t_entry) / med(t_winners):.1f} x")
    print(f"  {n} ActionSelector.select calls (with the winner's host validation): {med(t_select):.2f} ms  (rounds: {fmt(t_select)})")
    print(f"  one ActionSelector.candidates call, k = 4 (with up to 4 host validations per observation): {med(t_cands):.2f} ms"
          f"  (rounds: {fmt(t_cands)}); candidates found: {sum(len(c) for c in cands)} of {4 * n}")


def loop_timing(slots, k, actions):
    from flingbot_amd import evaluate, lookahead, nets, sim as fsim, tasks as ftasks
    from flingbot_amd.env import BatchedFlingEnv

    random.seed(1); np.random.seed(1); torch.manual_seed(1)
    gen = fsim.FlingSim(n_envs=slots, solver=0)
    tasks = [t for t in ftasks.generate_tasks(gen, [ftasks.draw_task_parameters() for _ in range(slots)]) if t is not None]
    gen.close()
    policy = None
    for mode in ("run_episodes", "lookahead policy", "lookahead best"):
        ctx = fsim.FlingSim(n_envs=slots, solver=0)
        env = BatchedFlingEnv(ctx, episode_length=actions)
        if policy is None:
            policy = nets.MaximumValuePolicy(action_primitives=["fling"], num_rotations=12, scale_factors=list(env.scale_factors),
                                             obs_dim=64, pix_grasp_dist=8, pix_drag_dist=8, pix_place_dist=5, rgb_only=True,
                                             depth_only=False, action_expl_prob=0.0, action_expl_decay=1.0, value_expl_prob=0.0,
                                             value_expl_decay=1.0, device="cuda:0")
        t0 = time.perf_counter()
        if mode == "run_episodes":
            stats = evaluate.run_episodes(policy, env, tasks)
            flings = int(sum(stats["action_primitive_counts"].values()))
            extra = ""
        else:
            stats = lookahead.run_episodes(policy, env, tasks[:slots // k], k, follow=mode.split()[1])
            look = stats["lookahead"]
            flings = look["n_lane_steps"]
            extra = (f", regret {look['regret']:.4f}, rank 0 best in {look['rank0_best_frac']:.2f} of the steps, mean reward per rank "
                     + " / ".join("-" if v is None else f"{v:+.4f}" for v in look["mean_reward_per_rank"])
                     + f", coverage {stats['mean']['init_coverage']:.3f} -> {stats['mean']['final_coverage']:.3f}")
        dt = time.perf_counter() - t0
        ctx.close()
        print(f"  {mode:<17} {slots} slots: {dt:6.2f} s, {flings} flings executed ({flings / dt:.1f} /s), "
              f"{stats['simulation_steps']} episode-steps ({stats['simulation_steps'] / dt:.0f} /s){extra}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--trunks", type=int, default=48)
    ap.add_argument("--lanes", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--slots", type=int, default=192)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--actions", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lookahead_timing: no GPU (a timing taken elsewhere says nothing)")
    for dim in (64, 104):
        fork_timing(dim, a.trunks, a.lanes, a.rounds)
    winners_timing()
    if a.slots > 0:
        print(f"evaluation, generated hard tasks, up to {a.actions} actions, k = {a.k}:")
        loop_timing(a.slots, a.k, a.actions)
