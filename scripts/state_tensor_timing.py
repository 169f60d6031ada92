"""What the particle state costs as device tensors, against the per-episode path (EXPERIMENTS.md R34.1).

    python scripts/state_tensor_timing.py [--rounds 7] [--calls 5] [--shapes uniform mixed]

Four measurements per shape, all in one context (the per-episode accessors are unchanged by fs_state_gather / fs_state_scatter,
so they ARE the parent commit's path):
  gather,  batched      FlingSim.state_tensors(envs)                      -> pos4, vel4 CUDA [n, n_max, 4]
  gather,  per episode  get_positions + get_velocities per episode, packed into the same padded arrays, ONE upload each
  scatter, batched      FlingSim.set_state_tensors(envs, pos4, vel4)
  scatter, per episode  ONE download of the two tensors, then set_positions + set_velocities per episode
Shapes: `uniform` 256 episodes of 64 x 64; `mixed` 192 episodes with both sides drawn from 64 .. 103, the sizes the
evaluation loop holds.  Every measurement is a host clock around calls that end in a device synchronise; two warm-up calls,
then the median of --calls calls; --rounds rounds, the order of the four reversed in every other round.  Before anything is
timed the two gathers are compared bit for bit at the timed size, and the two scatters by gathering what they wrote."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def shape_sides(name):
    if name == "uniform":
        return [(64, 64)] * 256
    rng = np.random.RandomState(0)
    return [tuple(int(s) for s in rng.randint(64, 104, 2)) for _ in range(192)]


def gather_loop(sim, envs, n_max, dev):
    import torch

    pos = np.zeros((len(envs), n_max, 4), np.float32)
    vel = np.zeros((len(envs), n_max, 4), np.float32)
    for k, e in enumerate(envs):
        p = sim.get_positions(e).reshape(-1, 4)
        pos[k, :p.shape[0]] = p
        vel[k, :p.shape[0], :3] = sim.get_velocities(e).reshape(-1, 3)
    pos4, vel4 = torch.from_numpy(pos).to(dev), torch.from_numpy(vel).to(dev)
    torch.cuda.synchronize()
    return pos4, vel4


def scatter_loop(sim, envs, counts, pos4, vel4):
    pos, vel = pos4.cpu().numpy(), vel4.cpu().numpy()
    for k, e in enumerate(envs):
        sim.set_positions(e, pos[k, :counts[k]])
        sim.set_velocities(e, vel[k, :counts[k], :3])


def measure(name, rounds, calls, ways):
    import torch

    from flingbot_amd import sim as fsim
    from scenarios import cloth_params

    sides = shape_sides(name)
    n = len(sides)
    sim = fsim.FlingSim(n_envs=n, solver=0)
    envs = list(range(n))
    for e, (w, h) in zip(envs, sides):
        sim.set_scene(e, cloth_params(w, h, pos=(0.0, 0.3, 0.0)))
    sim.step(5)   # falling: non-zero velocities
    dev = torch.device("cuda", sim.device)
    st = sim.state_tensors(envs)
    counts, n_max = st.counts, st.n_max
    # ---- the same job, bit for bit, at the timed size
    lp, lv = gather_loop(sim, envs, n_max, dev)
    assert torch.equal(st.pos4.view(torch.int32), lp.view(torch.int32))
    assert torch.equal(st.vel4[..., :3].contiguous().view(torch.int32), lv[..., :3].contiguous().view(torch.int32))
    new_p, new_v = st.pos4.clone(), st.vel4.clone()
    new_p[..., 1] += 1e-3
    new_v[..., :3] *= 0.5
    new_v[..., 3] = 0.0
    sim.set_state_tensors(envs, pos4=new_p, vel4=new_v)
    a = sim.state_tensors(envs)
    sim.set_state_tensors(envs, pos4=st.pos4, vel4=st.vel4)
    scatter_loop(sim, envs, counts, new_p, new_v)
    b = sim.state_tensors(envs)
    assert torch.equal(a.pos4.view(torch.int32), b.pos4.view(torch.int32)) and torch.equal(a.vel4.view(torch.int32), b.vel4.view(torch.int32))
    m = a.mask
    assert torch.equal(a.pos4[m].view(torch.int32), new_p[m].view(torch.int32))

    out = torch.empty_like(st.pos4), torch.empty_like(st.vel4), None
    jobs = {
        "gather, batched": lambda: sim.state_tensors(envs, n_max=n_max, out=out),
        "gather, per episode": lambda: gather_loop(sim, envs, n_max, dev),
        "scatter, batched": lambda: sim.set_state_tensors(envs, pos4=new_p, vel4=new_v),
        "scatter, per episode": lambda: scatter_loop(sim, envs, counts, new_p, new_v),
    }
    jobs = {k: v for k, v in jobs.items() if k.split(",")[0] in ways}
    got = {k: [] for k in jobs}
    for r in range(rounds):
        order = list(jobs) if r % 2 == 0 else list(jobs)[::-1]
        for k in order:
            ts = []
            for c in range(calls + 2):   # two warm-up calls
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                jobs[k]()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            got[k].append(float(np.median(ts[2:])))
    sim.close()
    particles = int(counts.sum())
    print(f"{name}: {n} episodes, {particles} particles, n_max {n_max} ({particles / (n * n_max):.0%} of the padded batch), "
          f"median of {calls} calls per round, {rounds} rounds, order reversed every other round")
    res = dict(shape=name, episodes=n, particles=particles, n_max=int(n_max))
    for k, v in got.items():
        print(f"  {k:<22}: median {np.median(v):9.3f} ms   min {min(v):9.3f}   max {max(v):9.3f}")
        res[k] = dict(median_ms=float(np.median(v)), min_ms=min(v), max_ms=max(v))
    for way in ways:
        fast, slow = np.median(got[f"{way}, batched"]), np.median(got[f"{way}, per episode"])
        worst = max(got[f"{way}, batched"]) < min(got[f"{way}, per episode"])
        print(f"  {way}: batched is {slow / fast:.1f}x the per-episode path's speed; slowest batched round below the fastest "
              f"per-episode round: {worst}")
        res[f"{way}_speedup"] = float(slow / fast)
        res[f"{way}_batched_faster"] = bool(fast < slow)
    print("RESULT " + json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=["uniform", "mixed"], choices=["uniform", "mixed"])
    ap.add_argument("--ways", nargs="+", default=["gather", "scatter"], choices=["gather", "scatter"])
    a = ap.parse_args()
    results = [measure(s, a.rounds, a.calls, a.ways) for s in a.shapes]
    ok = all(r[f"{way}_batched_faster"] for r in results for way in a.ways)
    print(f"the batched call is faster than the per-episode path at every shape, in both directions: {ok}")
