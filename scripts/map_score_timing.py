"""What scoring recorded maps costs (EXPERIMENTS R27.1).  One MI355X, one process, a host clock around windows that end in a
device synchronise, warm-up first, `--pairs` alternating pairs of windows per comparison; one JSON line:

    python scripts/map_score_timing.py

(a) fs_map_score (trainops.map_score on dense maps that are already on the device, rows left there) at 64 x 144, 1000 x 144 and
    1 x 4096 labels, next to the host loop over probe.map_stats on the same maps (predictions and labels already on the host: the
    read-back it would need is not counted).  The one condition: the kernel path is cheaper than the host loop in every pair, at
    every shape.
(b) a whole train.score_maps pass over 1000 images x 144 labels (take_maps, the folded HIP forward, fs_map_score, one read-back,
    the summary), next to ONE train.optimize_maps(hip_step=True, map_loss=True, rank_weight=0.5) update at 32 x 144.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--steps", type=int, default=40, help="(b): updates per window")
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
from flingbot_amd import nets, probe, replay, train, trainops  # noqa: E402

DEV = "cuda:0"
K = 144
LATTICE = np.array([y * 64 + x for y in range(8, 56, 4) for x in range(8, 56, 4)], np.int32)
stat = lambda v: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}   # noqa: E731


def window(fn, calls, device=True):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    if device:
        torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / calls


def kernel_and_host(images, labels_per_image, calls_kernel, calls_host):
    rng = np.random.default_rng(images * 10000 + labels_per_image)
    value = (rng.standard_normal((images, 4096)) * 0.3).astype(np.float32)
    pixels = LATTICE if labels_per_image == K else np.arange(labels_per_image, dtype=np.int32)
    pix = np.tile(pixels, images)
    label = (np.round(rng.standard_normal(images * labels_per_image) * 0.1 / 0.01) * 0.01).astype(np.float32)
    offsets = np.arange(images + 1, dtype=np.int64) * labels_per_image
    d_value, d_pix, d_label = (torch.from_numpy(v).to(DEV) for v in (value, pix, label))
    kernel = lambda: trainops.map_score(d_value, offsets, d_pix, d_label)   # noqa: E731
    pred = value[:, pixels]

    def host():
        return [probe.map_stats(pred[b], label[b * labels_per_image:(b + 1) * labels_per_image], None, 1.0) for b in range(images)]

    rows, stats = kernel().cpu().numpy(), host()
    assert [int(r[4]) for r in rows] == [s["pairs"] for s in stats] and [int(r[5]) for r in rows] == [s["concordant"] for s in stats]
    window(kernel, max(calls_kernel // 4, 3)), window(host, 1, device=False)
    k, h = [], []
    for _ in range(a.pairs):
        k.append(window(kernel, calls_kernel))
        h.append(window(host, calls_host, device=False))
    return {"images": images, "labels": images * labels_per_image, "fs_map_score_ms": stat(k), "host_map_stats_loop_ms": stat(h),
            "host_over_kernel": stat([y / x for x, y in zip(k, h)]), "kernel_is_cheaper_in_every_pair": bool(all(x < y for x, y in zip(k, h)))}


def pass_and_update():
    rng = np.random.default_rng(0)
    m = 1000
    maps = replay.MapSet.from_arrays(rng.random((m, 4, 64, 64), dtype=np.float32), np.arange(m + 1) * K, np.tile(LATTICE, m),
                                     (np.round(rng.uniform(-0.1, 0.2, m * K) / 0.01) * 0.01).astype(np.float32)).to_device(DEV)
    torch.manual_seed(1)
    policy = nets.MaximumValuePolicy(action_primitives=["fling"], num_rotations=12, scale_factors=[1.0], obs_dim=64, pix_grasp_dist=8,
                                     pix_drag_dist=8, pix_place_dist=5, rgb_only=True, depth_only=False, action_expl_prob=0.0,
                                     action_expl_decay=1.0, value_expl_prob=0.0, value_expl_decay=1.0, device=DEV)
    net = policy.value_nets["fling"]
    opt = train.HipAdam(policy.parameters(), lr=1e-3, weight_decay=1e-6)
    draw = np.random.default_rng(5)

    def score():
        out = train.score_maps(policy, {"fling": maps}, images_per_batch=64)["fling"]
        assert out["n_maps"] == m and out["pairs"] > 0

    def updates():
        policy.train()
        losses = train.optimize_maps("fling", net, opt, maps, a.steps, 32, draw, hip_step=True, map_loss=True, rank_weight=0.5)
        policy.eval()
        assert len(losses) == a.steps and np.isfinite(losses).all()

    score(), updates()
    s, u = [], []
    for _ in range(a.pairs):
        s.append(window(score, 1))    # (the first pass after updates also renews the fold: part of what a validation costs)
        u.append(window(updates, 1))
    return {"images": m, "labels": m * K, "score_maps_pass_ms": stat(s), "update_32x144_ms": stat([x / a.steps for x in u]),
            "pass_in_updates": stat([x / (y / a.steps) for x, y in zip(s, u)])}


print(json.dumps({"a_64x144": kernel_and_host(64, K, 2000, 1), "a_1000x144": kernel_and_host(1000, K, 500, 1),
                  "a_1x4096": kernel_and_host(1, 4096, 100, 2), "b_pass_1000x144": pass_and_update()}))
