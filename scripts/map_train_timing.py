"""What a dense map update costs against the per-entry updates that carry the same labels (EXPERIMENTS R25.1).  A synthetic set of
144-label images (a stride-4 lattice of 12 x 12 cells on [8, 55], as `evaluate --probe-stride 4` records them), hip_step=True:

    python scripts/map_train_timing.py                   # (a) step times and (b) resident bytes, one JSON line
    python scripts/map_train_timing.py --kernels-only    # a few dense steps and nothing else: the run to put under
                                                         # `rocprofv3 --kernel-trace --stats -d <dir> -- python ...` for (c)

(a) one `train.optimize_maps` step at 32 images x 144 labels against the 36 `train.optimize` steps of B = 128 that carry the same
    4608 labels through the per-entry path, in alternating windows in ONE process, host clock around work that ends in a device
    synchronise; the per-entry step alone is printed too (EXPERIMENTS R13: 3.81 ms).
(b) the bytes each set holds on the device for the same --images images: MapSet (one copy per image) and ExperienceSet (one copy
    per label).
(c) prints the bytes the two head kernels must move at the step's shape, to set their kernel times against: dh written once
    (32 x 16 x 64 x 64 x 4 bytes), h read at the taps (at most 144 x 4 bytes per label, forward and weight gradient each).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=32, help="images in the set (the per-entry set holds 144 x this many entries)")
ap.add_argument("--images-per-batch", type=int, default=32)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--steps", type=int, default=40, help="dense steps per window; the per-entry window runs 36 x this many / 4")
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--kernels-only", action="store_true")
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
from flingbot_amd import nets, replay, train  # noqa: E402

DEV = "cuda:0"
K = 144
B_ENTRY = 128
LATTICE = np.array([y * 64 + x for y in range(8, 56, 4) for x in range(8, 56, 4)], np.int32)
assert LATTICE.size == K and a.images_per_batch * K % B_ENTRY == 0
ENTRY_STEPS = a.images_per_batch * K // B_ENTRY          # 36 per-entry steps carry one dense step's labels


def make_sets():
    rng = np.random.default_rng(0)
    m = a.images
    images = rng.random((m, 4, 64, 64), dtype=np.float32)
    labels = rng.uniform(-0.1, 0.2, m * K).astype(np.float32)
    maps = replay.MapSet.from_arrays(images, np.arange(m + 1) * K, np.tile(LATTICE, m), labels).to_device(DEV)
    if a.kernels_only:
        return maps, None
    masks = np.zeros((m * K, 64, 64), bool)
    masks[np.arange(m * K), np.tile(LATTICE, m) // 64, np.tile(LATTICE, m) % 64] = True
    entries = replay.ExperienceSet.from_arrays(np.repeat(images, K, axis=0), masks, labels, groups=np.repeat(np.arange(m), K))
    return maps, entries.to_device(DEV)


def fresh():
    torch.manual_seed(1)
    net = nets.SpatialValueNet(rgb_only=True, device=DEV).to(DEV).train()
    return net, train.HipAdam(net.parameters(), lr=1e-3, weight_decay=1e-6)


def main():
    maps, entries = make_sets()
    net_d, opt_d = fresh()
    rng = np.random.default_rng(5)

    def dense(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        losses = train.optimize_maps("fling", net_d, opt_d, maps, steps, a.images_per_batch, rng, hip_step=True)
        torch.cuda.synchronize()
        assert len(losses) == steps and np.isfinite(losses).all()
        return 1e3 * (time.perf_counter() - t0) / steps

    if a.kernels_only:
        dense(a.warmup)
        print(json.dumps({"kernels_only": True, "dense_steps": a.warmup}))
        return
    net_e, opt_e = fresh()

    def per_entry(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        losses = train.optimize("fling", net_e, opt_e, entries, steps, B_ENTRY, rng, hip_step=True)
        torch.cuda.synchronize()
        assert len(losses) == steps and np.isfinite(losses).all()
        return 1e3 * (time.perf_counter() - t0) / steps

    dense(a.warmup)
    per_entry(a.warmup)
    d, e = [], []
    for _ in range(a.windows):          # alternating windows in one process
        d.append(dense(a.steps))
        e.append(per_entry(max(ENTRY_STEPS * a.steps // 4, 1)))
    ratios = [ENTRY_STEPS * y / x for x, y in zip(d, e)]
    stat = lambda v: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}   # noqa: E731
    entry_bytes = sum(int(t.numel()) * t.element_size() for k, t in entries._dev.items() if k != "device")
    labels = a.images_per_batch * K
    print(json.dumps({
        "shape": {"images_per_batch": a.images_per_batch, "labels_per_image": K, "labels": labels, "per_entry_batch": B_ENTRY,
                  "per_entry_steps_for_the_same_labels": ENTRY_STEPS},
        "dense_step_ms": stat(d), "per_entry_step_ms": stat(e),
        "per_entry_steps_for_the_same_labels_ms": stat([ENTRY_STEPS * y for y in e]),
        "per_entry_over_dense": stat(ratios), "dense_is_faster_in_every_window": bool(min(ratios) > 1.0),
        "resident_bytes": {"images": a.images, "labels": a.images * K, "map_set": maps.resident_bytes(), "experience_set": entry_bytes,
                           "ratio": entry_bytes / maps.resident_bytes()},
        "head_kernels_bytes": {"dh_written": a.images_per_batch * 16 * 64 * 64 * 4, "h_read_at_the_taps_at_most": labels * 144 * 4},
    }))


main()
