"""Time one training batch out of the device-resident replay buffer against the host path.

    python scripts/replay_sample_timing.py [--samples 10240] [--batch 128] [--repeats 5] [--iters 200] [--host-iters 3]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/replay_sample_timing.py --kernel-only     (the kernel alone)

Legs, alternating within every repeat, after a warm-up, on the same set (rgb_only with jitter) and the same seeds:
  device   ExperienceSet.sample(batch) end to end, synchronised: host draws, table upload, ONE launch (fs_replay_sample)
  host     ExperienceSet.item_host (color_jitter_host: the numpy form of the Pillow chain) + upload of the three arrays
--kernel-only runs the device leg alone, for a kernel trace of its own.  Prints one JSON line; the bytes per batch are
computed from the shapes.  At this size a batch is launch-bound: the figure is the time per batch and the gap to the host."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10240)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()

    import torch

    from flingbot_amd import replay

    rng = np.random.default_rng(0)
    obs = rng.random((a.samples, 4, 64, 64), dtype=np.float32)
    masks = np.zeros((a.samples, 64, 64), bool)
    masks[np.arange(a.samples), rng.integers(64, size=a.samples), rng.integers(64, size=a.samples)] = True
    data = replay.ExperienceSet.from_arrays(obs, masks, rng.random(a.samples, dtype=np.float32)).to_device("cuda:0")
    B = a.batch

    def device_leg(seed, iters):
        r = np.random.default_rng(seed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            out = data.sample(B, r)
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e3, out

    def host_leg(seed, iters):
        r = np.random.default_rng(seed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            idx, params = data.draw(B, r)
            o, m, l = data.item_host(idx, params)
            out = (torch.from_numpy(o).to("cuda:0"), torch.from_numpy(m).to("cuda:0"), torch.from_numpy(l).to("cuda:0"))
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e3, out

    device_leg(99, 20)                                      # warm-up
    if a.kernel_only:
        ms, _ = device_leg(1, a.iters)
        print(json.dumps({"kernel_only": True, "device_ms_per_batch": ms, "launches": a.iters + 20}))
        return
    host_leg(99, 1)
    dev, host = [], []
    for rep in range(a.repeats):
        d_ms, d_out = device_leg(rep, a.iters)
        h_ms, h_out = host_leg(rep, a.host_iters)
        dev.append(d_ms)
        host.append(h_ms)
    # (same seeds: the last batches of both legs are the same batch -- and must be the same bits)
    d_last, _ = device_leg(7, 1)[1], None
    h_last = host_leg(7, 1)[1]
    same = all(torch.equal(x, y) for x, y in zip(d_last, h_last))
    per_sample = 3 * 64 * 64 * 4 + 64 * 64 + 4              # colour planes + mask + label, read once and written once
    nbytes = B * (2 * per_sample + 9 * 4)
    print(json.dumps({
        "samples": a.samples, "batch": B, "repeats": a.repeats, "iters": a.iters, "host_iters": a.host_iters,
        "bytes_per_batch": nbytes, "device_ms_per_batch": {"median": float(np.median(dev)), "min": min(dev), "max": max(dev)},
        "host_ms_per_batch": {"median": float(np.median(host)), "min": min(host), "max": max(host)},
        "host_over_device": float(np.median(host) / np.median(dev)), "device_equals_host_bits": bool(same),
        "device_effective_GBps": nbytes / (float(np.median(dev)) * 1e-3) / 1e9}))


if __name__ == "__main__":
    main()
