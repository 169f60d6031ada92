"""What the map loss costs (EXPERIMENTS R26.1).  One MI355X, one process, a host clock around windows that end in a device
synchronise, warm-up first, five alternating pairs of windows per comparison; one JSON line:

    python scripts/map_loss_timing.py

(a) fs_map_loss against fs_group_loss on identical inputs (label mean, weight 0.5, temperature 0.1), the raw launches back to
    back: one image of 4096 labels -- the shape splitting a long image is for: the one condition is that fs_map_loss is faster
    in every pair -- and 28 images x 144 labels = 4032, the largest whole-map batch fs_group_loss takes.
(b) fs_map_loss at 32 x 144 and 64 x 144 labels against trainops.map_loss_torch on the GPU, forward + backward of the loss alone
    through autograd (MapLossFunction against the torch statement).
(c) one train.optimize_maps(hip_step=True) step at 32 images x 144 labels with map_loss=True, rank_weight=0.5 against the same
    step with rank_weight=0 and no map loss (torch's mse_loss).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--steps", type=int, default=40, help="(c): steps per window")
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
from flingbot_amd import nets, replay, train, trainops  # noqa: E402

DEV = "cuda:0"
K = 144
W, TAU = 0.5, 0.1
LATTICE = np.array([y * 64 + x for y in range(8, 56, 4) for x in range(8, 56, 4)], np.int32)
stat = lambda v: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}   # noqa: E731


def window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / calls


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
    pred = torch.from_numpy((rng.standard_normal(n) * 0.3).astype(np.float32)).to(DEV)
    label = torch.from_numpy((np.round(rng.standard_normal(n) * 0.1 / 0.05) * 0.05).astype(np.float32)).to(DEV)
    return pred, label, np.arange(images + 1, dtype=np.int64) * labels_per_image


def raw_launches(images, labels_per_image, calls_new, calls_old):
    pred, label, offsets = batch(images, labels_per_image)
    off = torch.from_numpy(offsets.astype(np.int32)).to(DEV)
    bounds = torch.from_numpy(np.repeat(np.stack([offsets[:-1], offsets[1:]], 1), np.diff(offsets), 0).astype(np.int32)).to(DEV)
    new = lambda: trainops.MapLossFunction._launch(pred, label, off, W, TAU, 0.0, False)          # noqa: E731
    old = lambda: trainops.GroupLossFunction._launch(pred, label, bounds, W, TAU, 0.0)            # noqa: E731
    (_, stats, _), (_, old_stats) = new(), old()
    assert stats[3].item() == old_stats[3].item() > 0                                             # the same pairs
    m, g = alternate(new, old, calls_new, calls_old)
    return {"labels": images * labels_per_image, "pairs": int(stats[3].item()), "fs_map_loss_ms": stat(m), "fs_group_loss_ms": stat(g),
            "group_over_map": stat([y / x for x, y in zip(m, g)]), "map_loss_is_faster_in_every_pair": bool(all(x < y for x, y in zip(m, g)))}


def against_torch(images, calls_kernel, calls_torch):
    pred0, label, offsets = batch(images, K)

    def kernel():
        p = pred0.clone().requires_grad_(True)
        trainops.MapLossFunction.apply(p, label, offsets, W, TAU, 0.0, False)[0].backward()

    def stated():
        p = pred0.clone().requires_grad_(True)
        trainops.map_loss_torch(p, label, offsets, W, TAU, 0.0, False)[0].backward()

    m, t = alternate(kernel, stated, calls_kernel, calls_torch)
    return {"labels": images * K, "map_loss_function_ms": stat(m), "map_loss_torch_ms": stat(t), "torch_over_kernel": stat([y / x for x, y in zip(m, t)])}


def steps():
    rng = np.random.default_rng(0)
    m = 32
    maps = replay.MapSet.from_arrays(rng.random((m, 4, 64, 64), dtype=np.float32), np.arange(m + 1) * K, np.tile(LATTICE, m),
                                     (np.round(rng.uniform(-0.1, 0.2, m * K) / 0.01) * 0.01).astype(np.float32)).to_device(DEV)
    draw = np.random.default_rng(5)

    def side(**kw):
        torch.manual_seed(1)
        net = nets.SpatialValueNet(rgb_only=True, device=DEV).to(DEV).train()
        opt = train.HipAdam(net.parameters(), lr=1e-3, weight_decay=1e-6)

        def run():
            losses = train.optimize_maps("fling", net, opt, maps, a.steps, m, draw, hip_step=True, **kw)
            assert len(losses) == a.steps and np.isfinite(losses).all()
        return run

    ranked, plain = side(map_loss=True, rank_weight=W), side()
    ranked(), plain()   # (a window is one call of a.steps steps)
    r, p = [], []
    for _ in range(a.pairs):
        r.append(window(ranked, 1))
        p.append(window(plain, 1))
    return {"images": m, "labels": m * K, "map_loss_rank_weight_0.5_step_ms": stat([x / a.steps for x in r]),
            "mse_loss_step_ms": stat([x / a.steps for x in p]), "ranked_over_plain": stat([x / y for x, y in zip(r, p)])}


print(json.dumps({"a_1x4096": raw_launches(1, 4096, 200, 20), "a_28x144": raw_launches(28, K, 2000, 2000),
                  "b_32x144": against_torch(32, 1000, 100), "b_64x144": against_torch(64, 1000, 50), "c_step_32x144": steps()}))
