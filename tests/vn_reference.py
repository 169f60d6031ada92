"""Plain float64 forward of SpatialValueNet (learning/nets.py:81-141) for the value-net tests.

Computed from the module's UNFOLDED parameters -- convolution, eval-mode BatchNorm formula, activations -- with torch
float64 conv2d on the host.  It does not go through fold_batchnorm or fs_value_net_pack, so a test comparing the HIP
forward with it checks the fold and the packing as well as the kernels.  NaN and Inf follow IEEE float64 through every
stage (relu / leaky_relu keep NaN), which is what the module itself does.

Helpers:
    forward_f64(net, obs)       float64 [B, 1, H, W] output of `net` on `obs` (any device; computed on the host)
    cpu_module(net)             fp32 CPU copy of the unfolded module graph (fresh module, same state_dict)
    error_f32(net, obs, ref)    max |fp32 CPU module - float64| on `obs`: the error fp32 itself causes (e32)
    randomise_bn(net, seed, gain)
    make_obs(batch, seed)       random observations with a depth-like channel 3
"""
import numpy as np
import torch
import torch.nn.functional as F


def _select_channels(net, obs):
    """The channel selection of SpatialValueNet.preprocess_obs."""
    c = obs.shape[1]
    if net.rgb_only:
        if c == 4:
            return obs[:, :3]
        if c != 3:
            raise ValueError(f"rgb net needs 3 or 4 channels, got {c}")
        return obs
    if net.depth_only:
        return obs[:, 3:4] if c == 4 else obs[:, :1]
    return obs


def _bn(x, bn):
    mean = bn.running_mean.detach().double().cpu().reshape(1, -1, 1, 1)
    var = bn.running_var.detach().double().cpu().reshape(1, -1, 1, 1)
    w = bn.weight.detach().double().cpu().reshape(1, -1, 1, 1)
    b = bn.bias.detach().double().cpu().reshape(1, -1, 1, 1)
    return (x - mean) / torch.sqrt(var + bn.eps) * w + b


def _conv(x, conv):
    assert conv.bias is None and conv.stride == (1, 1) and conv.padding == (1, 1)
    return F.conv2d(x, conv.weight.detach().double().cpu(), padding=1)


@torch.no_grad()
def forward_f64(net, obs, chunk=64):
    """float64 forward of `net` (a SpatialValueNet) on `obs` [B, C, H, W]; returns a float64 CPU tensor [B, 1, H, W]."""
    obs = torch.as_tensor(obs).detach().cpu()
    x = _select_channels(net, obs).double()
    mean = torch.as_tensor(net.mean).double().reshape(1, -1, 1, 1)
    std = torch.as_tensor(net.std).double().reshape(1, -1, 1, 1)
    blocks = list(net.net)
    head, tail = blocks[0].net, blocks[-1].net
    assert isinstance(head[2], torch.nn.LeakyReLU) and len(tail) == 1
    outs = []
    for s in range(0, x.shape[0], chunk):
        h = (x[s:s + chunk] - mean) / std
        h = F.leaky_relu(_bn(_conv(h, head[0]), head[1]), head[2].negative_slope)
        for blk in blocks[1:-1]:
            r = torch.relu(_bn(_conv(h, blk.conv1), blk.bn1))
            h = torch.relu(_bn(_conv(r, blk.conv2), blk.bn2) + h)
        outs.append(_conv(h, tail[0]))
    return torch.cat(outs) if outs else torch.empty((0, 1) + tuple(x.shape[-2:]), dtype=torch.float64)


def cpu_module(net):
    """A fresh fp32 CPU SpatialValueNet with `net`'s flags and state_dict, in eval mode and unfolded."""
    from flingbot_amd import nets

    cpu = nets.SpatialValueNet(rgb_only=net.rgb_only, depth_only=net.depth_only, device="cpu")
    cpu.load_state_dict({k: v.detach().cpu() for k, v in net.state_dict().items()})
    return cpu.eval()


@torch.no_grad()
def error_f32(net, obs, ref=None):
    """e32: max |fp32 CPU module - float64| over `obs` (finite entries of the reference only)."""
    obs = torch.as_tensor(obs).detach().cpu()
    ref = forward_f64(net, obs) if ref is None else ref
    out = cpu_module(net)(obs.float()).double()
    fin = torch.isfinite(ref) & torch.isfinite(out)
    return float((out - ref)[fin].abs().max()) if bool(fin.any()) else 0.0


def tolerance(e32, ref):
    """The per-case bound of the HIP forward against float64: set by fp32 itself, not fitted to the kernel."""
    fin = ref[torch.isfinite(ref)]
    scale = float(fin.abs().max()) if fin.numel() else 0.0
    return max(4.0 * e32, 2e-6 * max(1.0, scale))


def randomise_bn(net, seed, gain=None):
    """Random eval-mode BatchNorm statistics (as tests/test_valuenet_gpu.py does).  gain=(lo, hi): BN weights drawn from
    [lo, hi) instead of [0.5, 1.5), so activations grow down the residual chain."""
    g = torch.Generator().manual_seed(seed)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.2)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
            lo, hi = gain if gain is not None else (0.5, 1.5)
            m.weight.data.copy_(torch.rand(m.weight.shape, generator=g) * (hi - lo) + lo)
            m.bias.data.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    return net


def make_obs(batch, seed, channels=4):
    """Random observations in [0, 1) with a depth-like channel 3 (1.99 +- 0.005, the network's depth statistics)."""
    g = torch.Generator().manual_seed(seed)
    obs = torch.rand(batch, 4, 64, 64, generator=g)
    obs[:, 3] = 1.99 + 0.01 * (obs[:, 3] - 0.5)
    return obs[:, :channels].contiguous()


def worst_pixel(out, ref):
    """(image, row, col, |err|) of the largest finite error, and where it sits in the kernels' tiling."""
    err = (out.double().cpu() - ref).abs()
    err[~torch.isfinite(err)] = 0
    k = int(err.reshape(-1).argmax())
    b, _, r, c = np.unravel_index(k, tuple(err.shape))
    where = []
    if r % 8 in (0, 7):
        where.append("strip boundary row")
    if c % 16 in (0, 15):
        where.append("16-column MFMA tile edge")
    if r in (0, ref.shape[-2] - 1) or c in (0, ref.shape[-1] - 1):
        where.append("image border")
    return (int(b), int(r), int(c), float(err.reshape(-1)[k])), (", ".join(where) or "interior")
