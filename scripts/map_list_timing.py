"""What the listwise map term costs (EXPERIMENTS R31.1).  One MI355X, HIP events around windows of calls, warm-up first, alternating
pairs of windows per comparison, medians with their ranges; one JSON line:

    python scripts/map_list_timing.py [--parent DIR]

(a) fs_map_list_loss at 1 x 4096, 32 x 144 and 1000 x 144 labels (label mean, weight 0.5, both temperatures 0.1): forward +
    backward of the term alone through autograd, MapListFunction against trainops.map_list_torch on the device -- the one
    condition is that the kernel path is faster in every pair at every shape -- and the raw launches against fs_map_loss' with
    weight 0.5 on the same inputs.
(b) one train.optimize_maps(hip_step=True, map_loss=True, rank_weight=0.5) update at 32 images x 144 labels with list_weight 0
    and 0.5.
(c) with --parent DIR (a built checkout of the parent commit): the flags-absent update of (b) under this tree's code and under
    the parent's, each in a fresh process (`--step-only --root DIR`), alternating; the condition is that this tree's median lies
    inside the range of the parent's own runs.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--steps", type=int, default=40, help="(b), (c): updates per window")
ap.add_argument("--parent", type=str, default=None, help="(c): a built checkout of the parent commit")
ap.add_argument("--runs", type=int, default=4, help="(c): processes per side")
ap.add_argument("--step-only", action="store_true", help="(c)'s child: time the flags-absent update under --root's package")
ap.add_argument("--root", type=str, default=HERE)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))

import torch  # noqa: E402
from flingbot_amd import nets, replay, train, trainops  # noqa: E402

DEV = "cuda:0"
K = 144
W, T = 0.5, 0.1
LATTICE = np.array([y * 64 + x for y in range(8, 56, 4) for x in range(8, 56, 4)], np.int32)
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


def shape(images, labels_per_image, calls_kernel, calls_torch, calls_pairwise):
    pred0, label, offsets = batch(images, labels_per_image)
    off = torch.from_numpy(offsets.astype(np.int32)).to(DEV)

    def kernel():
        p = pred0.clone().requires_grad_(True)
        trainops.MapListFunction.apply(p, label, offsets, W, T, None, False)[0].backward()

    def stated():
        p = pred0.clone().requires_grad_(True)
        trainops.map_list_torch(p, label, offsets, W, T, None, False)[0].backward()

    raw = lambda: trainops.MapListFunction._launch(pred0, label, off, W, T, T, False)             # noqa: E731
    pairwise = lambda: trainops.MapLossFunction._launch(pred0, label, off, W, T, 0.0, False)      # noqa: E731
    k, t = alternate(kernel, stated, calls_kernel, calls_torch)
    r, m = alternate(raw, pairwise, calls_kernel, calls_pairwise)
    return {"images": images, "labels": images * labels_per_image, "map_list_function_ms": stat(k), "map_list_torch_ms": stat(t),
            "torch_over_kernel": stat([y / x for x, y in zip(k, t)]), "kernel_is_faster_in_every_pair": bool(all(x < y for x, y in zip(k, t))),
            "fs_map_list_loss_ms": stat(r), "fs_map_loss_ms": stat(m), "pairwise_over_listwise": stat([y / x for x, y in zip(r, m)])}


def update(**kw):
    """A closure that runs a.steps optimize_maps updates at 32 x 144 on a fresh net."""
    rng = np.random.default_rng(0)
    m = 32
    maps = replay.MapSet.from_arrays(rng.random((m, 4, 64, 64), dtype=np.float32), np.arange(m + 1) * K, np.tile(LATTICE, m),
                                     (np.round(rng.uniform(-0.1, 0.2, m * K) / 0.01) * 0.01).astype(np.float32)).to_device(DEV)
    draw = np.random.default_rng(5)
    torch.manual_seed(1)
    net = nets.SpatialValueNet(rgb_only=True, device=DEV).to(DEV).train()
    opt = train.HipAdam(net.parameters(), lr=1e-3, weight_decay=1e-6)

    def run():
        losses = train.optimize_maps("fling", net, opt, maps, a.steps, m, draw, hip_step=True, map_loss=True, rank_weight=W, **kw)
        assert len(losses) == a.steps and np.isfinite(losses).all()
    return run


def steps():
    plain, listed = update(), update(list_weight=0.5)
    plain(), listed()   # (a window is one call of a.steps updates)
    p, q = [], []
    for _ in range(a.pairs):
        p.append(window(plain, 1) / a.steps)
        q.append(window(listed, 1) / a.steps)
    return {"images": 32, "labels": 32 * K, "list_weight_0_update_ms": stat(p), "list_weight_0.5_update_ms": stat(q),
            "listed_over_plain": stat([y / x for x, y in zip(p, q)])}


def step_only():
    plain = update()
    plain()
    return [window(plain, 1) / a.steps for _ in range(a.pairs)]


def against_parent():
    """The flags-absent update, a.runs fresh processes per side, parent and this tree alternating; every process's median."""
    sides = {"parent": [], "this_tree": []}
    for _ in range(a.runs):
        for name, root in (("parent", a.parent), ("this_tree", HERE)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--step-only", "--root", root, "--pairs", str(a.pairs),
                                  "--steps", str(a.steps)], check=True, capture_output=True, text=True, timeout=600).stdout
            sides[name].append(float(np.median(json.loads(out.strip().splitlines()[-1]))))
    lo, hi = min(sides["parent"]), max(sides["parent"])
    mine = float(np.median(sides["this_tree"]))
    return {"parent_update_ms": stat(sides["parent"]), "this_tree_update_ms": stat(sides["this_tree"]), "parent_runs": sides["parent"],
            "this_tree_runs": sides["this_tree"], "this_tree_median_inside_parent_range": bool(lo <= mine <= hi)}


if a.step_only:
    print(json.dumps(step_only()))
else:
    out = {}
    if a.parent:   # (first: this process has not opened the device yet, so one process at a time holds it)
        out["c_flags_absent_against_parent"] = against_parent()
    out.update({"a_1x4096": shape(1, 4096, 500, 50, 50), "a_32x144": shape(32, K, 500, 50, 500),
                "a_1000x144": shape(1000, K, 200, 20, 50), "b_update_32x144": steps()})
    print(json.dumps(out))
