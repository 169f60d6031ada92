"""What the temperature sweep of the listwise map term costs (EXPERIMENTS R32.1).  One MI355X, HIP events around windows of
calls, warm-up first, alternating pairs of windows per comparison, medians with their ranges; one JSON line:

    python scripts/map_sweep_timing.py

Per shape (32 x 144, 1000 x 144 and 1 x 4096 labels) and per number of temperatures S (33 and 64, spread over 1e-3 .. 1e2, label
temperature 0.1, label mean): one fs_map_list_sweep call (both launches, through trainops.MapListSweep._launch) against
(a) S calls of trainops.MapListFunction._launch, one per temperature -- what a sweep cost before -- and
(b) trainops.map_list_sweep_torch on the device, in float64 as the kernel computes.
The one condition is that the sweep is faster than (a) in every pair at every shape.  And one whole trainops.fit_temperature
call (six sweeps and six downloads of a [33, 8] curve) at each shape.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=5)
a = ap.parse_args()
sys.path.insert(0, HERE)

import torch  # noqa: E402
from flingbot_amd import trainops  # noqa: E402

DEV = "cuda:0"
TY = 0.1
stat = lambda v: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}   # noqa: E731


def window(fn, calls):
    """ms per call of `calls` calls between two HIP events."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def alternate(first, second, calls_first, calls_second):
    """`pairs` alternating pairs of windows, in ms per call; a quarter window of each as warm-up."""
    window(first, max(calls_first // 4, 3)), window(second, max(calls_second // 4, 3))
    x, y = [], []
    for _ in range(a.pairs):
        x.append(window(first, calls_first))
        y.append(window(second, calls_second))
    return x, y


def batch(images, labels_per_image):
    rng = np.random.default_rng(images * 10000 + labels_per_image)
    n = images * labels_per_image
    label = (np.round(rng.uniform(-0.11, 0.21, n) / 0.01) * 0.01).astype(np.float32)
    pred = (label + rng.standard_normal(n) * 0.1).astype(np.float32)
    return torch.from_numpy(pred).to(DEV), torch.from_numpy(label).to(DEV), np.arange(images + 1, dtype=np.int64) * labels_per_image


def shape(images, labels_per_image, calls_sweep, calls_chain, calls_torch):
    pred, label, offsets = batch(images, labels_per_image)
    off = torch.from_numpy(offsets.astype(np.int32)).to(DEV)
    pred64, label64 = pred.double(), label.double()
    out = {"images": images, "labels": images * labels_per_image}
    for S in (33, 64):
        temps = np.exp(np.linspace(np.log(1e-3), np.log(1e2), S))
        sweep = lambda: trainops.MapListSweep._launch(pred, label, off, temps, TY, False)   # noqa: E731, B023

        def chain():
            for t in temps:   # noqa: B023
                trainops.MapListFunction._launch(pred, label, off, 1.0, float(t), TY, False)

        stated = lambda: trainops.map_list_sweep_torch(pred64, label64, offsets, temps, TY, False)   # noqa: E731, B023
        k, c = alternate(sweep, chain, calls_sweep, calls_chain)
        k2, t = alternate(sweep, stated, calls_sweep, calls_torch)
        out[f"S{S}"] = {"fs_map_list_sweep_ms": stat(k), "one_list_loss_per_temperature_ms": stat(c),
                        "chain_over_sweep": stat([y / x for x, y in zip(k, c)]),
                        "sweep_is_faster_in_every_pair": bool(all(x < y for x, y in zip(k, c))),
                        "fs_map_list_sweep_again_ms": stat(k2), "map_list_sweep_torch_ms": stat(t),
                        "torch_over_sweep": stat([y / x for x, y in zip(k2, t)])}
    fit = lambda: trainops.fit_temperature(pred, label, offsets, TY)   # noqa: E731
    sweeps = fit()["sweeps"]
    window(fit, 3)
    out["fit_temperature"] = {"sweeps": sweeps, "ms": stat([window(fit, 10) for _ in range(a.pairs)])}
    return out


print(json.dumps({"32x144": shape(32, 144, 300, 10, 20), "1000x144": shape(1000, 144, 100, 10, 5), "1x4096": shape(1, 4096, 300, 10, 20)}))
