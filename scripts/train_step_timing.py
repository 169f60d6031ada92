"""One full value-net train step (forward, loss, backward, Adam) at B = 128 on the rgb net: the hand-written 16 -> 16
convolution passes (nets._TRAIN_CONV_HIP = True) against the stock PyTorch / MIOpen step (False), in ONE process,
alternating between the two.

    python scripts/train_step_timing.py [--batch 128] [--steps 200] [--repeats 5] [--json out.json]
    python scripts/train_step_timing.py --kernels-only hip --steps 50  # a short run for a kernel trace of its own
    python scripts/train_step_timing.py --deterministic                # as train.run() runs its updates

Each timed window is `--steps` steps between two device synchronisations; the windows of the two paths alternate
(hip, stock, hip, stock, ...), `--repeats` of each after a warm-up of both.  Reported: the median window per path in ms
per step, the spread between repeats (max - min), and whether the difference of the medians exceeds the larger spread.
Bytes and FLOPs of the three kernels per step follow from the shapes and are printed for the kernel-trace comparison:
per 16 -> 16 layer forward and data gradient read and write B x 16 x 64 x 64 floats each and do 2 x 144 x 16 FLOPs per
output pixel; the weight gradient reads both tensors and does the same arithmetic.  `--deterministic` wraps every window
in `train.deterministic_library_convs()`, which is how `train.run` runs its updates (it reaches only the
library convolutions left in the step: the first and the last layer, and all of them on the stock path)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--kernels-only", choices=["hip", "stock"], default=None, help="run `--steps` steps of one path and stop")
    ap.add_argument("--deterministic", action="store_true", help="time the steps inside train.deterministic_library_convs(), as train.run runs them")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    from flingbot_amd import nets, train

    dev = "cuda:0"
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    B = a.batch
    obs = torch.rand(B, 3, 64, 64, device=dev)
    mask = torch.zeros(B, 64, 64, dtype=torch.bool)
    for k in range(B):
        mask[k, int(rng.integers(8, 56)), int(rng.integers(8, 56))] = True
    mask = mask.to(dev)
    label = torch.from_numpy(rng.uniform(-0.1, 0.2, B).astype(np.float32)).to(dev)

    def make():
        torch.manual_seed(1)
        net = nets.SpatialValueNet(rgb_only=True, device=dev).to(dev).train()
        return net, torch.optim.Adam(net.parameters(), lr=1e-3, weight_decay=1e-6)

    paths = {"hip": (True,) + make(), "stock": (False,) + make()}

    def window(name, steps):
        flag, net, opt = paths[name]
        nets._TRAIN_CONV_HIP = flag
        with train.deterministic_library_convs(a.deterministic):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                pred = torch.masked_select(net(obs).squeeze(), mask)
                loss = torch.nn.functional.mse_loss(pred, label)
                opt.zero_grad()
                loss.backward()
                opt.step()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        nets._TRAIN_CONV_HIP = True
        return 1e3 * dt / steps

    if a.kernels_only:
        window(a.kernels_only, a.warmup)
        print(json.dumps({"path": a.kernels_only, "ms_per_step": window(a.kernels_only, a.steps), "steps": a.steps, "batch": B}))
        return
    for name in paths:
        window(name, a.warmup)
    times = {name: [] for name in paths}
    for _ in range(a.repeats):
        for name in paths:
            times[name].append(window(name, a.steps))
    act = B * 16 * 64 * 64 * 4
    flops = 2.0 * 144 * 16 * B * 64 * 64
    out = {"batch": B, "steps_per_window": a.steps, "repeats": a.repeats, "deterministic": a.deterministic,
           "per_layer_pass": {"conv_bytes": 2 * act, "wgrad_bytes": 2 * act + 2 * B * 8 * 2304 * 4, "flops": flops}}
    for name, v in times.items():
        out[name] = {"median_ms": float(np.median(v)), "spread_ms": float(max(v) - min(v)), "windows_ms": [round(x, 4) for x in v]}
    gain = out["stock"]["median_ms"] - out["hip"]["median_ms"]
    spread = max(out["hip"]["spread_ms"], out["stock"]["spread_ms"])
    out["gain_ms"] = gain
    out["gate"] = "pass" if gain > spread else "fail"
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
