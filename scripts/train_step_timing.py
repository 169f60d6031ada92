"""One full value-net train step (forward, loss, backward, Adam) at B = 128 on the rgb net, four paths in ONE process,
alternating between them:
    hip_step  hip_bn plus the rest (csrc/fs_edgetrain.hip): the first layer, the last layer at the mask's pixel
            (SpatialValueNet.forward_selected inside nets.train_edge_hip()) and Adam as one launch (train.HipAdam).  No library
            convolution is left, so this path NEVER runs inside the deterministic context, with or without --deterministic
    hip_bn  nets._TRAIN_CONV_HIP = True, nets._TRAIN_BN_HIP = True: the hand-written 16 -> 16 convolution passes and the
            hand-written train-mode BatchNorm + activation (+ residual add) of all 17 sites (csrc/fs_bntrain.hip)
    hip     True / False: the convolution passes alone -- the step as it was before the BatchNorm kernels
    stock   False / False: every operator PyTorch / MIOpen

    python scripts/train_step_timing.py [--batch 128] [--steps 200] [--repeats 5] [--json out.json]
    python scripts/train_step_timing.py --kernels-only hip_step --steps 50  # a short run for a kernel trace of its own
    python scripts/train_step_timing.py --deterministic                   # as train.run() runs its updates

Each timed window is `--steps` steps between two device synchronisations; the windows of the paths alternate
(hip_step, hip_bn, hip, stock, hip_step, ...), `--repeats` of each after a warm-up of all; `--paths` picks a subset.  Reported:
the median window per path in ms per step, the spread between repeats (max - min), and three gates -- `gate`: hip against stock,
`bn_gate`: hip_bn against hip, `step_gate`: hip_step against hip_bn -- each "pass" when the difference of the medians exceeds
the larger of the two spreads.  With --deterministic, `step_gate` is the comparison that describes train.run: hip_bn inside
train.deterministic_library_convs() (what run() executes without hip_step) against hip_step outside it (what it executes with).
Bytes of the new kernels per step from the shapes (B images, C = 3 input channels, one activation tensor = B x 16 x 64 x 64
floats): the first layer's forward reads B x C x 4096 floats and writes one activation tensor, its weight gradient reads both;
the head's backward writes one activation tensor; Adam reads four and writes three floats per parameter.
Bytes per BatchNorm launch from the shapes (one activation tensor = B x 16 x 64 x 64 floats): the forward reads x for the
statistics, reads x (+ the residual) and writes y: 3 or 4 tensors; the backward reads x, y, dy twice and writes dx (+ the
residual's gradient): 7 or 8 tensors.
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
    ap.add_argument("--kernels-only", choices=["hip_step", "hip_bn", "hip", "stock"], default=None, help="run `--steps` steps of one path and stop")
    ap.add_argument("--paths", default="hip_step,hip_bn,hip,stock", help="comma-separated subset of the paths to time")
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

    def make_hip_step():
        net, _ = make()
        return net, train.HipAdam(net.parameters(), lr=1e-3, weight_decay=1e-6)

    makers = {"hip_step": lambda: ((True, True),) + make_hip_step(), "hip_bn": lambda: ((True, True),) + make(),
              "hip": lambda: ((True, False),) + make(), "stock": lambda: ((False, False),) + make()}
    wanted = [a.kernels_only] if a.kernels_only else [n.strip() for n in a.paths.split(",") if n.strip()]
    if not wanted or any(n not in makers for n in wanted):
        ap.error("--paths: a comma-separated subset of " + ", ".join(makers))
    paths = {name: makers[name]() for name in makers if name in wanted}
    defaults = (nets._TRAIN_CONV_HIP, nets._TRAIN_BN_HIP)

    def window(name, steps):
        flags, net, opt = paths[name]
        edge = name == "hip_step"
        nets._TRAIN_CONV_HIP, nets._TRAIN_BN_HIP = flags
        with train.deterministic_library_convs(a.deterministic and not edge), nets.train_edge_hip(edge):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                pred = net.forward_selected(obs, mask) if edge else torch.masked_select(net(obs).squeeze(), mask)
                loss = torch.nn.functional.mse_loss(pred, label)
                opt.zero_grad()
                loss.backward()
                opt.step()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        nets._TRAIN_CONV_HIP, nets._TRAIN_BN_HIP = defaults
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
    n_params = sum(p.numel() for p in next(iter(paths.values()))[1].parameters() if p.requires_grad)
    out = {"batch": B, "steps_per_window": a.steps, "repeats": a.repeats, "deterministic": a.deterministic,
           "per_layer_pass": {"conv_bytes": 2 * act, "wgrad_bytes": 2 * act + 2 * B * 8 * 2304 * 4, "flops": flops},
           "per_bn_launch_bytes": {"forward": 3 * act, "forward_residual": 4 * act, "backward": 7 * act, "backward_residual": 8 * act},
           "edge_bytes": {"convin_forward": B * 3 * 4096 * 4 + act, "convin_wgrad": B * 3 * 4096 * 4 + act + 2 * B * 4 * 432 * 4,
                          "head_backward": act, "adam": 7 * 4 * n_params}}
    for name, v in times.items():
        out[name] = {"median_ms": float(np.median(v)), "spread_ms": float(max(v) - min(v)), "windows_ms": [round(x, 4) for x in v]}

    def gate(slow, fast, gain_key, gate_key):
        if slow in out and fast in out:
            gain = out[slow]["median_ms"] - out[fast]["median_ms"]
            out[gain_key] = gain
            out[gate_key] = "pass" if gain > max(out[slow]["spread_ms"], out[fast]["spread_ms"]) else "fail"

    gate("stock", "hip", "gain_ms", "gate")
    gate("hip", "hip_bn", "bn_gain_ms", "bn_gate")
    gate("hip_bn", "hip_step", "step_gain_ms", "step_gate")
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
