"""What the ranking term costs (EXPERIMENTS R23.1).  One process = one tree and one configuration: `train.optimize(hip_step=True)`
at B = 128 on a device-resident set of 512 entries in 128 groups of 4 (a batch is 32 groups of 4); prints one JSON line with the
window times in ms per update.  Run the configurations as separate processes, alternating, and compare their medians against the
spread between processes:

    python scripts/rank_loss_timing.py --tree ../parent-checkout            # (a) a checkout of the parent commit, built
    python scripts/rank_loss_timing.py --weight 0                           # (b) this tree, the term off
    python scripts/rank_loss_timing.py --weight 0.5                         # (c) the term on: grouped batches, fs_group_loss
    python scripts/rank_loss_timing.py --loss-only                          # loss forward + backward alone: kernel / torch / mse_loss

--tree names the checkout whose flingbot_amd is imported (default: this one); without --weight, optimize is called without the rank
arguments, which is the only call a parent checkout accepts.  --loss-only also times the kernel alone with device events, at the
training shape and at one segment of 4096 samples.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--weight", type=float, default=None, help="None: call optimize without the rank arguments (the parent's call)")
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--steps", type=int, default=250)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--loss-only", action="store_true")
ap.add_argument("--tag", default="")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree))

import torch  # noqa: E402
from flingbot_amd import nets, replay, train  # noqa: E402

assert os.path.abspath(nets.__file__).startswith(os.path.abspath(a.tree)), nets.__file__
DEV = "cuda:0"
B = 128


def make_set():
    rng = np.random.default_rng(0)
    n = 512
    obs = rng.random((n, 4, 64, 64), dtype=np.float32)
    masks = np.zeros((n, 64, 64), bool)
    masks[np.arange(n), rng.integers(8, 56, n), rng.integers(8, 56, n)] = True
    labels = rng.uniform(-0.1, 0.2, n).astype(np.float32)
    kw = dict(groups=np.repeat(np.arange(n // 4), 4)) if a.weight is not None else {}
    return replay.ExperienceSet.from_arrays(obs, masks, labels, **kw).to_device(DEV)


def steps_windows():
    data = make_set()
    torch.manual_seed(1)
    net = nets.SpatialValueNet(rgb_only=True, device=DEV).to(DEV).train()
    opt = train.HipAdam(net.parameters(), lr=1e-3, weight_decay=1e-6)
    rng = np.random.default_rng(5)
    kw = {} if a.weight is None else dict(rank_weight=a.weight)

    def window(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        losses = train.optimize("fling", net, opt, data, steps, B, rng, hip_step=True, **kw)
        torch.cuda.synchronize()
        assert len(losses) == steps and np.isfinite(losses).all()
        return 1e3 * (time.perf_counter() - t0) / steps

    window(a.warmup)
    return [window(a.steps) for _ in range(a.windows)]


def loss_windows():
    from flingbot_amd import trainops

    rng = np.random.default_rng(0)
    pred0 = torch.from_numpy((rng.standard_normal(B) * 0.3).astype(np.float32)).to(DEV)
    label = torch.from_numpy(rng.uniform(-0.1, 0.2, B).astype(np.float32)).to(DEV)
    table = np.repeat(np.arange(0, B, 4), 4)
    table = np.stack([table, table + 4], 1).astype(np.int32)
    bounds = torch.from_numpy(table).to(DEV)
    bounds.host = table

    def kernel():
        p = pred0.clone().requires_grad_(True)
        loss, _ = trainops.GroupLossFunction.apply(p, label, bounds, 0.5, 0.1, 0.0)
        loss.backward()
        return p.grad

    def stated():
        p = pred0.clone().requires_grad_(True)
        loss, _ = trainops.group_loss_torch(p, label, bounds, 0.5, 0.1, 0.0)
        loss.backward()
        return p.grad

    def mse():
        p = pred0.clone().requires_grad_(True)
        torch.nn.functional.mse_loss(p, label).backward()
        return p.grad

    out = {}
    fns = {"kernel": kernel, "torch": stated, "mse_loss": mse}
    for fn in fns.values():
        for _ in range(50):
            fn()
    for _ in range(a.windows):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(500):
                fn()
            torch.cuda.synchronize()
            out.setdefault(name, []).append(1e3 * (time.perf_counter() - t0) / 500)
    # device time of the kernel alone at the training shape and at the largest single segment
    from flingbot_amd.trainops import GroupLossFunction
    for n, seg in ((B, table), (4096, np.tile(np.int32([[0, 4096]]), (4096, 1)))):
        p = torch.randn(n, device=DEV) * 0.3
        y = torch.randn(n, device=DEV) * 0.1
        b = torch.from_numpy(np.ascontiguousarray(seg)).to(DEV)
        for _ in range(3):
            GroupLossFunction._launch(p, y, b, 0.5, 0.1, 0.0)
        reps = 200 if n == B else 10
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for _ in range(5):
            e0.record()
            for _ in range(reps):
                GroupLossFunction._launch(p, y, b, 0.5, 0.1, 0.0)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / reps)
        out[f"kernel_back_to_back_B{n}"] = times
    return out


if a.loss_only:
    res = loss_windows()
    print(json.dumps({"tag": a.tag, "loss_only_ms": {k: {"median": float(np.median(v)), "min": min(v), "max": max(v)} for k, v in res.items()}}))
else:
    w = steps_windows()
    print(json.dumps({"tag": a.tag, "weight": a.weight, "median_ms": float(np.median(w)), "min": min(w), "max": max(w), "windows": [round(x, 4) for x in w]}))
