"""The value net's training operators in libflingsim as autograd Functions: Conv16Function (csrc/fs_vntrain.hip),
BatchNormAct16Function (csrc/fs_bntrain.hip), ConvInFunction, HeadPixelFunction and HeadPixelsFunction (csrc/fs_edgetrain.hip:
the last layer at one pixel per sample, and at a list of pixels per image).  nets.py decides which layer goes through which of
them and re-exports the classes; train.HipAdam is the optimizer's step.
GroupLossFunction (csrc/fs_grouploss.hip) is the loss with a pairwise ranking term over the groups of a batch; train.optimize
uses it when rank_weight > 0, and group_loss_torch states the same formula in torch ops.
MapLossFunction (csrc/fs_maploss.hip) is that loss over images with many labels each -- no cap on the batch, per-label or
per-image normalisation; train.optimize_maps uses it with map_loss=True, and map_loss_torch is its statement in torch ops.
MapListFunction (csrc/fs_maplist.hip) is the listwise term over the same images -- per image the KL divergence between the
Boltzmann distributions of labels and predictions, O(K) -- which train.optimize_maps and train.optimize add with list_weight > 0;
map_list_torch is its statement in torch ops.
map_list_sweep (csrc/fs_mapsweep.hip; not differentiable) is that term at up to 64 prediction temperatures in one pass, with its
derivatives in 1 / T and the Boltzmann policy's earnings; fit_temperature minimises it over T -- train.score_maps and
train.optimize_maps use it -- and map_list_sweep_torch is its statement in torch ops.
map_score (csrc/fs_mapscore.hip; not differentiable) is the rank statistics of recorded maps under the weights that wrote the
dense value maps -- train.score_maps uses it -- with map_score_host its statement in numpy and summarize_scores the means.

Every Function validates its arguments before anything touches the library (ValueError, also without a GPU), brings them
into the kernels' form (`operand`) and queues its launches through sim.stream_call on the current stream of the tensors'
device.  The static launchers (_conv, _wgrad, _forward, _backward) take operands that already have that form.
"""
import torch

from .sim import stream_call, work_buffer


def operand(t):
    """What the kernels take: NCHW-contiguous and 16-byte aligned (a channels-last or strided tensor is copied, a
    storage-offset view off the boundary is cloned)."""
    t = t.contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def is_map(t, channels=(16,), like=None):
    """A CUDA fp32 [B >= 1, C, 64, 64] tensor with C in `channels` -- on the device of `like`, when that is given: what the
    training kernels serve."""
    return (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.shape[0] >= 1
            and t.shape[1] in channels and tuple(t.shape[2:]) == (64, 64) and (like is None or t.device == like.device))


def _require_map(name, t, channels=(16,)):
    if not is_map(t, channels):
        raise ValueError(f"{name} serves CUDA fp32 [B >= 1, {' | '.join(map(str, channels))}, 64, 64], "
                         f"got {t.dtype} {tuple(t.shape)} on {t.device}")


def _is_fp32(t, shape, like):
    """A CUDA fp32 tensor of `shape` on the device of `like`."""
    return t.is_cuda and t.device == like.device and t.dtype == torch.float32 and tuple(t.shape) == tuple(shape)


class Conv16Function(torch.autograd.Function):
    """Conv3x3(16 -> 16, stride 1, padding 1, no bias) on [B, 16, 64, 64] fp32 CUDA tensors with all three passes in
    libflingsim (csrc/fs_vntrain.hip): forward and data gradient are one kernel (fs_conv16_forward, transposed = 0 / 1),
    the weight gradient is fs_conv16_wgrad.  The weight is read on the device as it is: nothing is packed on the host."""
    n_forward = 0    # calls so far (the tests count them)
    n_backward = 0

    @staticmethod
    def _conv(x, weight, transposed):
        out = torch.empty_like(x)
        stream_call("fs_conv16_forward", x.device, x, weight, int(transposed), x.shape[0], 64, out)
        return out

    @staticmethod
    def _wgrad(x, grad):
        dw = torch.empty((16, 16, 3, 3), dtype=torch.float32, device=x.device)
        work = work_buffer("fs_conv16_work_bytes", x.device, x.shape[0], 64)   # partial tiles
        stream_call("fs_conv16_wgrad", x.device, x, grad, x.shape[0], 64, dw, work)
        return dw

    @staticmethod
    def forward(ctx, x, weight):
        _require_map("Conv16Function", x)
        if not _is_fp32(weight, (16, 16, 3, 3), x):
            raise ValueError("Conv16Function: the weight is CUDA fp32 [16, 16, 3, 3]")
        x, weight = operand(x.detach()), operand(weight.detach())
        ctx.save_for_backward(x, weight)
        Conv16Function.n_forward += 1
        return Conv16Function._conv(x, weight, 0)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        x, weight = ctx.saved_tensors
        grad = operand(grad)
        Conv16Function.n_backward += 1
        dx = Conv16Function._conv(grad, weight, 1) if ctx.needs_input_grad[0] else None
        dw = Conv16Function._wgrad(x, grad) if ctx.needs_input_grad[1] else None
        return dx, dw


class BatchNormAct16Function(torch.autograd.Function):
    """Train-mode BatchNorm2d(16) + activation (+ residual add in front of it) on [B, 16, 64, 64] fp32 CUDA tensors in
    libflingsim (csrc/fs_bntrain.hip): y = act(bn(x) [+ residual]) with act(z) = z > 0 ? z : slope * z -- slope 0 is ReLU,
    0.01 the first layer's LeakyReLU, 1 no activation.  `apply(x, weight, bias, residual_or_None, running_mean, running_var,
    momentum, eps, slope)` returns y, updates the two running buffers in place (both None: no update) and hands back the
    gradients of x, weight, bias and residual; the backward takes the activation's mask from the stored y."""
    n_forward = 0    # calls so far (the tests count them)
    n_backward = 0

    @staticmethod
    def _forward(x, weight, bias, residual, running_mean, running_var, momentum, eps, slope):
        """(y, save_mean, save_invstd) of operands that are already what the kernels take."""
        y = torch.empty_like(x)
        save_mean = torch.empty(16, dtype=torch.float32, device=x.device)
        save_invstd = torch.empty(16, dtype=torch.float32, device=x.device)
        work = work_buffer("fs_bn16_work_bytes", x.device, x.shape[0], 64)   # per-plane partial sums
        stream_call("fs_bn16_forward", x.device, x, residual, weight, bias, float(eps), float(slope), float(momentum),
                    running_mean, running_var, x.shape[0], 64, y, save_mean, save_invstd, work)
        return y, save_mean, save_invstd

    @staticmethod
    def _backward(x, y, dy, weight, save_mean, save_invstd, slope, with_residual):
        """(dx, dresidual or None, dweight, dbias)."""
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if with_residual else None
        dweight = torch.empty(16, dtype=torch.float32, device=x.device)
        dbias = torch.empty(16, dtype=torch.float32, device=x.device)
        work = work_buffer("fs_bn16_work_bytes", x.device, x.shape[0], 64)
        stream_call("fs_bn16_backward", x.device, x, y, dy, weight, save_mean, save_invstd, float(slope), x.shape[0], 64,
                    dx, dres, dweight, dbias, work)
        return dx, dres, dweight, dbias

    @staticmethod
    def forward(ctx, x, weight, bias, residual, running_mean, running_var, momentum, eps, slope):
        _require_map("BatchNormAct16Function", x)
        if residual is not None and not (is_map(residual, like=x) and residual.shape == x.shape):
            raise ValueError("BatchNormAct16Function: the residual has the shape, dtype and device of x")
        if (running_mean is None) != (running_var is None):
            raise ValueError("BatchNormAct16Function: running_mean and running_var are given together or not at all")
        for name, v in (("weight", weight), ("bias", bias), ("running_mean", running_mean), ("running_var", running_var)):
            if v is not None and not _is_fp32(v, (16,), x):
                raise ValueError(f"BatchNormAct16Function: {name} is CUDA fp32 [16] on the device of x")
        x, weight, bias = operand(x.detach()), operand(weight.detach()), operand(bias.detach())
        residual = None if residual is None else operand(residual.detach())
        rm = rv = None
        if running_mean is not None:
            rm, rv = operand(running_mean.detach()), operand(running_var.detach())
        y, save_mean, save_invstd = BatchNormAct16Function._forward(x, weight, bias, residual, rm, rv, momentum, eps, slope)
        if rm is not None:   # a buffer that had to be copied for the kernel gets its update back
            if rm.data_ptr() != running_mean.data_ptr():
                running_mean.detach().copy_(rm)
            if rv.data_ptr() != running_var.data_ptr():
                running_var.detach().copy_(rv)
        ctx.save_for_backward(x, y, weight, save_mean, save_invstd)
        ctx.slope, ctx.with_residual = float(slope), residual is not None
        BatchNormAct16Function.n_forward += 1
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        x, y, weight, save_mean, save_invstd = ctx.saved_tensors
        grad = operand(grad)
        BatchNormAct16Function.n_backward += 1
        dx, dres, dweight, dbias = BatchNormAct16Function._backward(x, y, grad, weight, save_mean, save_invstd, ctx.slope,
                                                                    ctx.with_residual)
        need = ctx.needs_input_grad
        return (dx if need[0] else None, dweight if need[1] else None, dbias if need[2] else None,
                dres if need[3] else None, None, None, None, None, None)


class ConvInFunction(torch.autograd.Function):
    """Conv3x3(C -> 16, stride 1, padding 1, no bias) on a [B, C, 64, 64] fp32 CUDA tensor with C in {1, 3, 4}: the value net's
    first layer in libflingsim (csrc/fs_edgetrain.hip) -- forward fs_convin_forward, weight gradient fs_convin_wgrad.  The
    input gets no gradient (it is the observation); the weight is read on the device as it is."""
    n_forward = 0    # calls so far (the tests count them)
    n_backward = 0

    @staticmethod
    def _forward(x, weight):
        batch, channels = x.shape[:2]
        out = torch.empty((batch, 16, 64, 64), dtype=torch.float32, device=x.device)
        stream_call("fs_convin_forward", x.device, x, weight, channels, batch, 64, out)
        return out

    @staticmethod
    def _wgrad(x, grad):
        batch, channels = x.shape[:2]
        dw = torch.empty((16, channels, 3, 3), dtype=torch.float32, device=x.device)
        work = work_buffer("fs_convin_work_bytes", x.device, channels, batch, 64)   # per-strip partials
        stream_call("fs_convin_wgrad", x.device, x, grad, channels, batch, 64, dw, work)
        return dw

    @staticmethod
    def forward(ctx, x, weight):
        _require_map("ConvInFunction", x, (1, 3, 4))
        if not _is_fp32(weight, (16, x.shape[1], 3, 3), x):
            raise ValueError("ConvInFunction: the weight is CUDA fp32 [16, C, 3, 3] on the device of x")
        x, weight = operand(x.detach()), operand(weight.detach())
        if ctx.needs_input_grad[0]:
            raise ValueError("ConvInFunction has no data gradient: its input must not require grad")
        ctx.save_for_backward(x)
        ConvInFunction.n_forward += 1
        return ConvInFunction._forward(x, weight)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        (x,) = ctx.saved_tensors
        ConvInFunction.n_backward += 1
        dw = ConvInFunction._wgrad(x, operand(grad)) if ctx.needs_input_grad[1] else None
        return None, dw


class HeadPixelFunction(torch.autograd.Function):
    """The value net's last layer, Conv3x3(16 -> 1, padding 1, no bias), at ONE pixel per sample: `apply(h, weight, pix)` with h
    a [B, 16, 64, 64] fp32 CUDA tensor, weight [1, 16, 3, 3] and pix an integer [B] tensor of flat pixel indices in [0, 4096)
    returns [B] -- the values the dense convolution has there -- in libflingsim (csrc/fs_edgetrain.hip, fs_head_forward).  The
    backward (fs_head_backward) writes the whole gradient of h, zero outside each sample's 3 x 3 x 16 patch, and the weight's."""
    n_forward = 0    # calls so far (the tests count them)
    n_backward = 0

    @staticmethod
    def _forward(h, weight, pix):
        pred = torch.empty(h.shape[0], dtype=torch.float32, device=h.device)
        stream_call("fs_head_forward", h.device, h, weight, pix, h.shape[0], 64, pred)
        return pred

    @staticmethod
    def _backward(h, weight, pix, gpred):
        """(dh, dweight)."""
        dh = torch.empty_like(h)
        dw = torch.empty((1, 16, 3, 3), dtype=torch.float32, device=h.device)
        stream_call("fs_head_backward", h.device, h, weight, pix, gpred, h.shape[0], 64, dh, dw)
        return dh, dw

    @staticmethod
    def forward(ctx, h, weight, pix):
        _require_map("HeadPixelFunction", h)
        if not _is_fp32(weight, (1, 16, 3, 3), h):
            raise ValueError("HeadPixelFunction: the weight is CUDA fp32 [1, 16, 3, 3] on the device of h")
        if not (torch.is_tensor(pix) and pix.is_cuda and pix.device == h.device and tuple(pix.shape) == (h.shape[0],)
                and pix.dtype in (torch.int32, torch.int64)):
            raise ValueError("HeadPixelFunction: pix is a CUDA int32 or int64 [B] tensor on the device of h")
        h, weight = operand(h.detach()), operand(weight.detach())
        pix = operand(pix.to(torch.int32))
        ctx.save_for_backward(h, weight, pix)
        HeadPixelFunction.n_forward += 1
        return HeadPixelFunction._forward(h, weight, pix)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        h, weight, pix = ctx.saved_tensors
        HeadPixelFunction.n_backward += 1
        dh, dw = HeadPixelFunction._backward(h, weight, pix, operand(grad.to(torch.float32)))
        return (dh if ctx.needs_input_grad[0] else None, dw if ctx.needs_input_grad[1] else None, None)


def check_pixel_table(offsets, pix_host, batch):
    """The pixel lists of a batch, validated on the host: offsets an integer [batch + 1] array in CSR form -- offsets[0] = 0,
    never falling, image b owning list entries [offsets[b], offsets[b + 1]), possibly none -- and pix_host the integer [L] list
    of flat pixels (None: the caller has no host copy, and only the offsets are checked), L = offsets[batch], every pixel in
    [0, 4096) and the pixels of ONE image distinct (fs_head_backward_pixels keeps one gradient per pixel of an image).
    ValueError otherwise.  Returns the offsets as int64 numpy [batch + 1]."""
    import numpy as np

    table = np.asarray(offsets)
    if table.shape != (int(batch) + 1,) or table.dtype.kind not in "iu":
        raise ValueError(f"pixel table: offsets are integers [{int(batch) + 1}], got {table.dtype} {table.shape}")
    table = table.astype(np.int64)
    if table[0] != 0:
        raise ValueError("pixel table: offsets[0] must be 0")
    if (np.diff(table) < 0).any():
        raise ValueError("pixel table: offsets must not fall")
    if pix_host is None:
        return table
    pix = np.asarray(pix_host)
    if pix.ndim != 1 or pix.dtype.kind not in "iu":
        raise ValueError(f"pixel table: pixels are integers [L], got {pix.dtype} {pix.shape}")
    if table[-1] != pix.shape[0]:
        raise ValueError(f"pixel table: offsets[{int(batch)}] = {int(table[-1])} for a list of {pix.shape[0]} pixels")
    pix = pix.astype(np.int64)
    if pix.size and (pix.min() < 0 or pix.max() >= 4096):
        raise ValueError("pixel table: pixels lie in [0, 4096)")
    image = np.repeat(np.arange(int(batch), dtype=np.int64), np.diff(table))
    if np.unique(image * 4096 + pix).size != pix.size:
        raise ValueError("pixel table: the pixels of one image must be distinct")
    return table


class HeadPixelsFunction(torch.autograd.Function):
    """The value net's last layer, Conv3x3(16 -> 1, padding 1, no bias), at MANY pixels per image: `apply(h, weight, offsets,
    pix)` with h a [B, 16, 64, 64] fp32 CUDA tensor, weight [1, 16, 3, 3], offsets a HOST integer array [B + 1] in CSR form
    (image b owns list entries [offsets[b], offsets[b + 1]), possibly none; uploaded here, once) and pix a CUDA integer [L]
    tensor of flat pixels in [0, 4096), L = offsets[B] >= 1, returns [L] -- the values the dense convolution has there -- in
    libflingsim (csrc/fs_edgetrain.hip, fs_head_forward_pixels).  The backward (fs_head_backward_pixels) writes the whole
    gradient of h and the weight's.  The table is validated on the host first (check_pixel_table, ValueError): the offsets
    always, the pixels when the tensor carries its host copy as `pix.host` (MapSet.sample_maps leaves it there) -- without one
    no download is made, and the kernels clamp what they read all the same."""
    n_forward = 0    # calls so far (the tests count them)
    n_backward = 0

    @staticmethod
    def _forward(h, weight, offsets, pix):
        pred = torch.empty(pix.shape[0], dtype=torch.float32, device=h.device)
        stream_call("fs_head_forward_pixels", h.device, h, weight, offsets, pix, h.shape[0], pix.shape[0], 64, pred)
        return pred

    @staticmethod
    def _backward(h, weight, offsets, pix, gpred):
        """(dh, dweight)."""
        dh = torch.empty_like(h)
        dw = torch.empty((1, 16, 3, 3), dtype=torch.float32, device=h.device)
        work = work_buffer("fs_head_pixels_work_bytes", h.device, h.shape[0], pix.shape[0], 64)   # per-chunk partials of dw
        stream_call("fs_head_backward_pixels", h.device, h, weight, offsets, pix, gpred, h.shape[0], pix.shape[0], 64, dh, dw, work)
        return dh, dw

    @staticmethod
    def forward(ctx, h, weight, offsets, pix):
        _require_map("HeadPixelsFunction", h)
        if not _is_fp32(weight, (1, 16, 3, 3), h):
            raise ValueError("HeadPixelsFunction: the weight is CUDA fp32 [1, 16, 3, 3] on the device of h")
        if not (torch.is_tensor(pix) and pix.is_cuda and pix.device == h.device and pix.dim() == 1 and pix.shape[0] >= 1
                and pix.dtype in (torch.int32, torch.int64)):
            raise ValueError("HeadPixelsFunction: pix is a CUDA int32 or int64 [L >= 1] tensor on the device of h")
        if torch.is_tensor(offsets):
            if offsets.is_cuda:
                raise ValueError("HeadPixelsFunction: offsets is a HOST integer array [B + 1]")
            offsets = offsets.numpy()
        table = check_pixel_table(offsets, getattr(pix, "host", None), h.shape[0])
        if table[-1] != pix.shape[0]:
            raise ValueError(f"HeadPixelsFunction: offsets[{h.shape[0]}] = {int(table[-1])} for a list of {pix.shape[0]} pixels")
        h, weight = operand(h.detach()), operand(weight.detach())
        pix = operand(pix.to(torch.int32))
        offsets = operand(torch.from_numpy(table.astype("int32")).to(h.device))
        ctx.save_for_backward(h, weight, offsets, pix)
        HeadPixelsFunction.n_forward += 1
        return HeadPixelsFunction._forward(h, weight, offsets, pix)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        h, weight, offsets, pix = ctx.saved_tensors
        HeadPixelsFunction.n_backward += 1
        dh, dw = HeadPixelsFunction._backward(h, weight, offsets, pix, operand(grad.to(torch.float32)))
        return (dh if ctx.needs_input_grad[0] else None, dw if ctx.needs_input_grad[1] else None, None, None)


def check_bounds(bounds, batch):
    """The segment table of a batch, validated on the host: int [batch, 2] rows [begin, end) with begin <= i < end <= batch for
    row i, and every sample of a segment naming that same segment.  ValueError otherwise.  Returns it as int64 numpy [batch, 2].
    A device tensor that carries its host copy as `bounds.host` (ExperienceSet.sample_groups leaves it there) is checked on
    that copy, without a download and the wait that comes with one; the kernel clamps what it reads all the same."""
    import numpy as np

    if torch.is_tensor(bounds):
        host = getattr(bounds, "host", None)
        table = np.asarray(host) if host is not None else bounds.detach().cpu().numpy()
    else:
        table = np.asarray(bounds)
    if table.shape != (int(batch), 2) or table.dtype.kind not in "iu":
        raise ValueError(f"group loss: bounds are integers [{int(batch)}, 2], got {table.dtype} {table.shape}")
    table = table.astype(np.int64)
    begin, end, i = table[:, 0], table[:, 1], np.arange(int(batch))
    if not ((0 <= begin) & (begin <= i) & (i < end) & (end <= int(batch))).all():
        raise ValueError("group loss: bounds[i] = [begin, end) must hold begin <= i < end <= batch")
    if not ((begin[begin] == begin) & (end[begin] == end) & (begin[end - 1] == begin) & (end[end - 1] == end)).all():
        raise ValueError("group loss: the samples of one segment must all name that segment")
    return table


def group_loss_torch(pred, label, bounds, weight=0.0, temperature=0.1, min_gap=0.0):
    """fs_group_loss (include/flingsim.h) in plain differentiable torch ops, on any device and dtype: (loss, stats [8] =
    loss, mse, rank, P, C, 0, 0, 0).  The pairs are the (i, j) of one segment with label_i > label_j + min_gap, the comparison
    in float64 like the kernel's; rank = mean over them of softplus(-(pred_i - pred_j) / temperature) in the stable form
    max(x, 0) + log1p(exp(-|x|)), exactly 0 without pairs.  A [B, B] mask and a dozen and more small ops: the CPU path, and what
    the kernel is compared with."""
    B = pred.shape[0]
    table = torch.as_tensor(check_bounds(bounds, B), device=pred.device)
    begin, end = table[:, 0], table[:, 1]
    j = torch.arange(B, device=pred.device)
    same = (j[None, :] >= begin[:, None]) & (j[None, :] < end[:, None])
    y = label.detach().double()
    pairs = same & (y[:, None] > y[None, :] + float(min_gap))                    # [i, j]: i should score higher than j
    mse = ((pred - label) ** 2).sum() / B
    n_pairs = pairs.sum()
    x = -(pred[:, None] - pred[None, :]) / float(temperature)
    softplus = torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs()))
    rank = torch.where(pairs, softplus, torch.zeros_like(softplus)).sum() / n_pairs.clamp(min=1).to(pred.dtype)   # P = 0: 0 / 1
    loss = mse + float(weight) * rank
    concordant = (pairs & (pred.detach()[:, None] > pred.detach()[None, :])).sum()
    zero = torch.zeros((), dtype=pred.dtype, device=pred.device)
    stats = torch.stack([loss.detach(), mse.detach(), rank.detach(), n_pairs.to(pred.dtype), concordant.to(pred.dtype),
                         zero, zero, zero])
    return loss, stats


class GroupLossFunction(torch.autograd.Function):
    """The training loss with the pairwise ranking term, value and gradient in ONE launch (libflingsim fs_group_loss,
    csrc/fs_grouploss.hip): `apply(pred, label, bounds, weight, temperature, min_gap)` returns (loss, stats) with pred and
    label [B] (1 <= B <= 4096), bounds an integer [B, 2] table of segments (ExperienceSet.sample_groups) and stats float [8] =
    loss, mse, rank, P, C, 0, 0, 0 (not differentiable).  forward launches the kernel with grad_scale 1 and keeps dpred; backward
    is grad_output * dpred: one multiply.  The table is validated on the host first (check_bounds, ValueError).  CUDA fp32
    predictions go through the kernel; anything else through group_loss_torch."""
    n_forward = 0    # kernel launches so far (the tests count them)

    @staticmethod
    def _launch(pred, label, bounds, weight, temperature, min_gap, scale=1.0):
        """(dpred [B], stats [8]) of operands that are already what the kernel takes."""
        dpred = torch.empty_like(pred)
        stats = torch.empty(8, dtype=torch.float32, device=pred.device)
        stream_call("fs_group_loss", pred.device, pred, label, bounds, pred.shape[0], float(weight), float(temperature),
                    float(min_gap), float(scale), dpred, stats)
        return dpred, stats

    @staticmethod
    def forward(ctx, pred, label, bounds, weight, temperature, min_gap):
        if not (torch.is_tensor(pred) and torch.is_tensor(label) and pred.dim() == 1 and label.shape == pred.shape
                and 1 <= pred.shape[0] <= 4096 and label.device == pred.device and label.dtype == pred.dtype):
            raise ValueError("GroupLossFunction: pred and label are [B] tensors of one dtype on one device, 1 <= B <= 4096")
        if not (float(weight) >= 0.0 and float(temperature) > 0.0 and float(min_gap) >= 0.0
                and all(abs(float(v)) < float("inf") for v in (weight, temperature, min_gap))):
            raise ValueError("GroupLossFunction: weight >= 0, temperature > 0 and min_gap >= 0, all finite")
        table = check_bounds(bounds, pred.shape[0])
        ctx.kernel = bool(pred.is_cuda and pred.dtype == torch.float32)
        if ctx.kernel:
            if torch.is_tensor(bounds) and bounds.device == pred.device and bounds.dtype == torch.int32:
                dev_bounds = bounds.contiguous()
            else:
                dev_bounds = torch.as_tensor(table, dtype=torch.int32).to(pred.device)
            dpred, stats = GroupLossFunction._launch(pred.detach().contiguous(), label.detach().contiguous(), dev_bounds, weight,
                                                     temperature, min_gap)
            GroupLossFunction.n_forward += 1
            loss = stats[0].clone()
        else:
            with torch.enable_grad():
                p = pred.detach().requires_grad_(True)
                loss, stats = group_loss_torch(p, label.detach(), table, weight, temperature, min_gap)
                (dpred,) = torch.autograd.grad(loss, p)
            loss = loss.detach()
        ctx.save_for_backward(dpred)
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss, grad_stats):
        (dpred,) = ctx.saved_tensors
        return (grad_loss * dpred if ctx.needs_input_grad[0] else None), None, None, None, None, None


def check_map_table(offsets, labels):
    """The offsets of a batch of images for the map loss, validated on the host: check_pixel_table's CSR rules for an integer
    [G + 1] array, and offsets[G] == labels >= 1 with no image longer than 4096 labels (what one workgroup of fs_map_loss holds).
    ValueError otherwise.  Returns int64 numpy [G + 1]."""
    import numpy as np

    if torch.is_tensor(offsets):
        if offsets.is_cuda:
            raise ValueError("map loss: offsets is a HOST integer array [G + 1]")
        offsets = offsets.numpy()
    shape = np.shape(offsets)
    if len(shape) != 1 or shape[0] < 2:
        raise ValueError(f"map loss: offsets are integers [G + 1] for G >= 1 images, got shape {shape}")
    table = check_pixel_table(offsets, None, shape[0] - 1)
    if table[-1] != int(labels):
        raise ValueError(f"map loss: offsets[{shape[0] - 1}] = {int(table[-1])} for {int(labels)} predictions")
    if int(labels) < 1:
        raise ValueError("map loss: at least one label")
    if np.diff(table).max() > 4096:
        raise ValueError(f"map loss: an image has {int(np.diff(table).max())} labels, more than 4096")
    return table


def map_loss_torch(pred, label, offsets, weight=0.0, temperature=0.1, min_gap=0.0, per_image=False):
    """fs_map_loss (include/flingsim.h) in plain differentiable torch ops, on any device and dtype: (loss, stats [8] = loss, mse,
    rank, P, C, G', G'', 0, table [G, 4] = per image S_b / K_b, R_b / P_b, P_b, C_b), stats and table detached.  offsets: a HOST
    integer [G + 1] array in CSR form; the pairs are the (i, j) of one image with label_i > label_j + min_gap, compared in float64
    like the kernel.  per_image = False is the mean over labels and over all pairs (group_loss_torch on the expanded bounds);
    True the mean over the images with labels, and over those with pairs, of the image's own mean.  An [L, L] mask and two
    dozen small ops: the CPU path, and what the kernel is timed against."""
    L = pred.shape[0]
    table = check_map_table(offsets, L)
    G = len(table) - 1
    dev = pred.device
    counts = torch.as_tensor(table[1:] - table[:-1], device=dev)
    image = torch.repeat_interleave(torch.arange(G, device=dev), counts)                  # [L]: the image of a label
    y = label.detach().double()
    pairs = (image[:, None] == image[None, :]) & (y[:, None] > y[None, :] + float(min_gap))   # [i, j]: i should score higher
    x = -(pred[:, None] - pred[None, :]) / float(temperature)
    softplus = torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs()))
    zeros = torch.zeros(G, dtype=pred.dtype, device=dev)
    S = zeros.index_add(0, image, (pred - label) ** 2)
    R = zeros.index_add(0, image, torch.where(pairs, softplus, torch.zeros_like(softplus)).sum(dim=1))
    P_b = torch.zeros(G, dtype=torch.int64, device=dev).index_add(0, image, pairs.sum(dim=1))
    C_b = torch.zeros(G, dtype=torch.int64, device=dev).index_add(
        0, image, (pairs & (pred.detach()[:, None] > pred.detach()[None, :])).sum(dim=1))
    K = counts.to(pred.dtype)
    image_mse = S / K.clamp(min=1)                                                        # (an empty image: 0 / 1)
    image_rank = R / P_b.clamp(min=1).to(pred.dtype)                                      # (P_b = 0: 0 / 1)
    filled, ranked, n_pairs = (counts > 0).sum(), (P_b > 0).sum(), P_b.sum()
    if per_image:
        mse = image_mse.sum() / filled.clamp(min=1).to(pred.dtype)
        rank = image_rank.sum() / ranked.clamp(min=1).to(pred.dtype)
    else:
        mse = S.sum() / L
        rank = R.sum() / n_pairs.clamp(min=1).to(pred.dtype)
    loss = mse + float(weight) * rank
    as_value = lambda t: t.detach().to(pred.dtype)   # noqa: E731
    stats = torch.stack([as_value(loss), as_value(mse), as_value(rank), as_value(n_pairs), as_value(C_b.sum()), as_value(filled),
                         as_value(ranked), torch.zeros((), dtype=pred.dtype, device=dev)])
    rows = torch.stack([as_value(image_mse), as_value(image_rank), as_value(P_b), as_value(C_b)], dim=1)
    return loss, stats, rows


class MapLossFunction(torch.autograd.Function):
    """The training loss with the pairwise ranking term over IMAGES with many labels each (libflingsim fs_map_loss,
    csrc/fs_maploss.hip: two launches, any number of images and labels): `apply(pred, label, offsets, weight, temperature, min_gap,
    per_image)` returns (loss, stats, table) with pred and label [L], offsets a HOST integer array [G + 1] in CSR form (image b
    owns entries [offsets[b], offsets[b + 1]), at most 4096 of them, possibly none; offsets[G] = L >= 1; check_map_table,
    ValueError before anything touches the library), stats [8] = loss, mse, rank, P, C, G', G'', 0 and table [G, 4] = per image
    S_b / K_b, R_b / P_b, P_b, C_b (neither differentiable; float64 and float32 from the kernel).  per_image: the mean over images
    of the image's mean instead of the mean over labels and over pairs.  forward launches the kernels with grad_scale 1 and keeps
    dpred; the loss is float32, built from stats[0]; backward is grad_output * dpred.  CUDA fp32 predictions go through the
    kernels; anything else through map_loss_torch."""
    n_forward = 0    # kernel calls so far (the tests count them)

    @staticmethod
    def _launch(pred, label, offsets, weight, temperature, min_gap, per_image, scale=1.0):
        """(dpred [L], stats float64 [8], table [G, 4]) of operands that are already what the kernels take; offsets a device
        int32 [G + 1] tensor."""
        images, labels = offsets.shape[0] - 1, pred.shape[0]
        dpred = torch.empty_like(pred)
        stats = torch.empty(8, dtype=torch.float64, device=pred.device)
        table = torch.empty((images, 4), dtype=torch.float32, device=pred.device)
        work = work_buffer("fs_map_loss_work_bytes", pred.device, images, labels)   # chunk sums and g
        stream_call("fs_map_loss", pred.device, pred, label, offsets, images, labels, float(weight), float(temperature),
                    float(min_gap), int(bool(per_image)), float(scale), dpred, stats, table, work)
        return dpred, stats, table

    @staticmethod
    def forward(ctx, pred, label, offsets, weight, temperature, min_gap, per_image):
        if not (torch.is_tensor(pred) and torch.is_tensor(label) and pred.dim() == 1 and label.shape == pred.shape
                and label.device == pred.device and label.dtype == pred.dtype):
            raise ValueError("MapLossFunction: pred and label are [L] tensors of one dtype on one device")
        if not (float(weight) >= 0.0 and float(temperature) > 0.0 and float(min_gap) >= 0.0
                and all(abs(float(v)) < float("inf") for v in (weight, temperature, min_gap))):
            raise ValueError("MapLossFunction: weight >= 0, temperature > 0 and min_gap >= 0, all finite")
        table = check_map_table(offsets, pred.shape[0])
        if pred.is_cuda and pred.dtype == torch.float32:
            dev_offsets = torch.from_numpy(table.astype("int32")).to(pred.device)
            dpred, stats, rows = MapLossFunction._launch(pred.detach().contiguous(), label.detach().contiguous(), dev_offsets,
                                                         weight, temperature, min_gap, per_image)
            MapLossFunction.n_forward += 1
            loss = stats[0].to(torch.float32)
        else:
            with torch.enable_grad():
                p = pred.detach().requires_grad_(True)
                loss, stats, rows = map_loss_torch(p, label.detach(), table, weight, temperature, min_gap, per_image)
                (dpred,) = torch.autograd.grad(loss, p)
            loss = loss.detach()
        ctx.save_for_backward(dpred)
        ctx.mark_non_differentiable(stats, rows)
        return loss, stats, rows

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss, grad_stats, grad_table):
        (dpred,) = ctx.saved_tensors
        return (grad_loss * dpred if ctx.needs_input_grad[0] else None), None, None, None, None, None, None


def _list_scalars(name, weight, pred_temperature, label_temperature):
    """(weight, T_p, T_y) as floats, label_temperature=None meaning T_p; ValueError unless weight >= 0 and both temperatures are
    positive, all finite with finite reciprocals."""
    try:
        w, tp = float(weight), float(pred_temperature)
        ty = tp if label_temperature is None else float(label_temperature)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: weight and the temperatures are numbers") from None
    inf = float("inf")
    if not (0.0 <= w < inf and 0.0 < tp < inf and 0.0 < ty < inf and 1.0 / tp < inf and 1.0 / ty < inf):
        raise ValueError(f"{name}: weight >= 0 and both temperatures > 0, all finite")
    return w, tp, ty


def map_list_torch(pred, label, offsets, weight, pred_temperature, label_temperature=None, per_image=False):
    """fs_map_list_loss (include/flingsim.h) in plain differentiable torch ops, on any device and dtype: (term, stats [8] =
    weight * list, list, G_l, L_l, H, chosen_mass, best_mass, 0, table [G, 4] = per image D_b, q at the arg-max of pred, the
    arg-max of pred, the arg-max of label; 0, 0, -1, -1 for an image with fewer than two labels), stats and table detached.
    offsets: a HOST integer [G + 1] array in CSR form.  Per listed image D_b = KL(softmax(label / T_y) || softmax(pred / T_p)),
    both as log-softmax with the image's maximum taken out; per_image = False weighs an image by its label count, True weighs
    the listed images alike.  label_temperature=None means equal to pred_temperature, where D_b = 0 exactly when pred - label is
    constant over the image.  Segment maxima and sums by scatter ops, some thirty small launches: the CPU path, and what the
    kernel is timed against."""
    w, tp, ty = _list_scalars("map_list_torch", weight, pred_temperature, label_temperature)
    L = pred.shape[0]
    table = check_map_table(offsets, L)
    G = len(table) - 1
    dev, dtype = pred.device, pred.dtype
    counts = torch.as_tensor(table[1:] - table[:-1], device=dev)
    begin = torch.as_tensor(table[:-1], device=dev)
    image = torch.repeat_interleave(torch.arange(G, device=dev), counts)                  # [L]: the image of a label
    within = torch.arange(L, device=dev) - begin[image]                                   # [L]: the index inside the image
    listed = counts >= 2
    zeros = torch.zeros(G, dtype=dtype, device=dev)
    low = torch.full((G,), float("-inf"), dtype=dtype, device=dev)

    def top(v):
        """(maximum [G], arg-max within the image [G]) with NaN below everything and ties to the lowest index."""
        v = torch.where(torch.isnan(v), torch.full_like(v, float("-inf")), v.detach())
        m = low.scatter_reduce(0, image, v, "amax", include_self=True)
        k = torch.full((G,), L, dtype=torch.int64, device=dev).scatter_reduce(
            0, image, torch.where(v == m[image], within, torch.full_like(within, L)), "amin", include_self=True)
        return m, k

    def log_softmax(x, m):
        z = zeros.index_add(0, image, torch.exp(x - m[image]))
        return (x - m[image]) - torch.log(z)[image]

    max_p, chosen = top(pred)
    max_y, best = top(label)
    ls = log_softmax(pred / tp, max_p / tp)
    lq = log_softmax(label.detach() / ty, max_y / ty)
    q = torch.exp(lq)
    addend = torch.where(q == 0, torch.zeros_like(q), q * (lq - ls))                      # an underflowed q: exactly 0
    D = zeros.index_add(0, image, addend)
    n_listed, n_labels = listed.sum(), (counts * listed).sum()
    if per_image:
        coef = listed.to(dtype) / n_listed.clamp(min=1).to(dtype)
    else:
        coef = (counts * listed).to(dtype) / n_labels.clamp(min=1).to(dtype)
    list_term = torch.where(listed, coef * D, zeros).sum()
    term = w * list_term
    at = (begin + chosen).clamp(max=L - 1)                                                # (an image without labels: masked below)
    q_chosen = torch.where(listed, q.detach()[at], zeros)
    q_best = torch.where(listed, zeros.scatter_reduce(0, image, q.detach(), "amax", include_self=True), zeros)
    mean = lambda v: v.sum() / n_listed.clamp(min=1).to(dtype)   # noqa: E731
    as_value = lambda t: t.detach().to(dtype)   # noqa: E731
    stats = torch.stack([as_value(term), as_value(list_term), as_value(n_listed), as_value(n_labels),
                         as_value((listed & (chosen == best)).sum()), mean(q_chosen), mean(q_best),
                         torch.zeros((), dtype=dtype, device=dev)])
    minus = torch.full((G,), -1.0, dtype=dtype, device=dev)
    rows = torch.stack([torch.where(listed, as_value(D), zeros), q_chosen, torch.where(listed, as_value(chosen), minus),
                        torch.where(listed, as_value(best), minus)], dim=1)
    return term, stats, rows


class MapListFunction(torch.autograd.Function):
    """The listwise term over IMAGES with many labels each (libflingsim fs_map_list_loss, csrc/fs_maplist.hip: two launches, O(K)
    per image): `apply(pred, label, offsets, weight, pred_temperature, label_temperature, per_image)` returns (term, stats, table)
    with pred and label [L], offsets a HOST integer array [G + 1] in CSR form (check_map_table: ValueError before anything touches
    the library, as for the scalars), label_temperature None for equal temperatures, stats [8] = weight * list, list, G_l, L_l, H,
    chosen_mass, best_mass, 0 and table [G, 4] = per image D_b, q at the arg-max of pred, the arg-max of pred, the arg-max of label
    (neither differentiable; float64 and float32 from the kernel).  forward launches the kernels with grad_scale 1 and keeps
    dpred; the term is float32, built from stats[0]; backward is grad_output * dpred.  CUDA fp32 predictions go through the
    kernels; anything else through map_list_torch."""
    n_forward = 0    # kernel calls so far (the tests count them)

    @staticmethod
    def _launch(pred, label, offsets, weight, pred_temperature, label_temperature, per_image, scale=1.0):
        """(dpred [L], stats float64 [8], table [G, 4]) of operands that are already what the kernels take; offsets a device
        int32 [G + 1] tensor."""
        images, labels = offsets.shape[0] - 1, pred.shape[0]
        dpred = torch.empty_like(pred)
        stats = torch.empty(8, dtype=torch.float64, device=pred.device)
        table = torch.empty((images, 4), dtype=torch.float32, device=pred.device)
        work = work_buffer("fs_map_list_work_bytes", pred.device, images, labels)   # the images' records and g
        stream_call("fs_map_list_loss", pred.device, pred, label, offsets, images, labels, float(weight), float(pred_temperature),
                    float(label_temperature), int(bool(per_image)), float(scale), dpred, stats, table, work)
        return dpred, stats, table

    @staticmethod
    def forward(ctx, pred, label, offsets, weight, pred_temperature, label_temperature, per_image):
        if not (torch.is_tensor(pred) and torch.is_tensor(label) and pred.dim() == 1 and label.shape == pred.shape
                and label.device == pred.device and label.dtype == pred.dtype):
            raise ValueError("MapListFunction: pred and label are [L] tensors of one dtype on one device")
        w, tp, ty = _list_scalars("MapListFunction", weight, pred_temperature, label_temperature)
        table = check_map_table(offsets, pred.shape[0])
        if pred.is_cuda and pred.dtype == torch.float32:
            dev_offsets = torch.from_numpy(table.astype("int32")).to(pred.device)
            dpred, stats, rows = MapListFunction._launch(pred.detach().contiguous(), label.detach().contiguous(), dev_offsets,
                                                         w, tp, ty, per_image)
            MapListFunction.n_forward += 1
            term = stats[0].to(torch.float32)
        else:
            with torch.enable_grad():
                p = pred.detach().requires_grad_(True)
                term, stats, rows = map_list_torch(p, label.detach(), table, w, tp, ty, per_image)
                (dpred,) = torch.autograd.grad(term, p)
            term = term.detach()
        ctx.save_for_backward(dpred)
        ctx.mark_non_differentiable(stats, rows)
        return term, stats, rows

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_term, grad_stats, grad_table):
        (dpred,) = ctx.saved_tensors
        return (grad_term * dpred if ctx.needs_input_grad[0] else None), None, None, None, None, None, None


SWEEP_COLUMNS = ("list", "slope", "curvature", "expected_regret", "best_draw", "greedy_draw", "listed_images", "listed_labels")


def _sweep_scalars(name, temperatures, label_temperature):
    """(temperatures float64 numpy [S], T_y float); ValueError unless there are 1 to 64 temperatures and each of them, T_y and
    their reciprocals is positive and finite, as a double and as a float (fs_map_list_sweep's rule)."""
    import numpy as np

    try:
        if torch.is_tensor(temperatures):
            temperatures = temperatures.detach().cpu().numpy()
        temps = np.array(temperatures, dtype=np.float64)
        ty = float(label_temperature)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: the temperatures are numbers") from None
    if temps.ndim != 1 or not 1 <= temps.shape[0] <= 64:
        raise ValueError(f"{name}: 1 to 64 temperatures in a [S] array, got shape {temps.shape}")
    both = np.concatenate([temps, [ty]])
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        both = np.concatenate([both, 1.0 / both])
        fine = np.isfinite(both) & (both > 0.0) & np.isfinite(both.astype(np.float32)) & (both.astype(np.float32) > 0.0)
    if not fine.all():
        raise ValueError(f"{name}: every temperature and label_temperature > 0, finite with finite reciprocals (also as floats)")
    return temps, ty


def _sweep_operands(name, pred, label):
    if not (torch.is_tensor(pred) and torch.is_tensor(label) and pred.dim() == 1 and label.shape == pred.shape
            and label.device == pred.device and label.dtype == pred.dtype and pred.is_floating_point()):
        raise ValueError(f"{name}: pred and label are floating-point [L] tensors of one dtype on one device")


def map_list_sweep_torch(pred, label, offsets, temperatures, label_temperature, per_image=False):
    """fs_map_list_sweep (include/flingsim.h) in plain torch ops, on any device and dtype: (curve [S, 8], rows [G, S, 4], images
    [G, 4]) in pred's dtype, nothing differentiable.  offsets: a HOST integer [G + 1] array in CSR form; temperatures: S = 1 to 64
    prediction temperatures T_s, beta_s = 1 / T_s.  Per listed image (at least two labels), with q = softmax(label / T_y) and s =
    softmax(beta_s pred):  rows[b, s] = D_b(beta_s) = KL(q || s), E_s[p] - E_q[p] (its derivative in beta), Var_s[p] (its second),
    E_s[y];  images[b] = K_b, y at the arg-max of y, y at the arg-max of pred, E_q[p];  zeros for the other images.  curve[s] =
    SWEEP_COLUMNS: list (map_list_torch's stats[1] at pred_temperature T_s), slope and curvature (the same coef-weighted sums of the
    two derivatives), expected_regret / best_draw / greedy_draw (the means over the listed images of y_best - E_s[y], of s at the
    arg-max of y and of s at the arg-max of pred), G_l, L_l.  Formed as the kernel forms it: the log-sums as log1p without the
    arg-max's own addend, the moments about the image's largest prediction, D_b from the three sums over q that do not depend on
    the temperature; an image with a NaN or an infinity has non-finite rows.  [S, L] intermediates: the CPU path, the float64
    reference of the tests, and what the kernel is timed against."""
    temps, ty = _sweep_scalars("map_list_sweep_torch", temperatures, label_temperature)
    _sweep_operands("map_list_sweep_torch", pred, label)
    L = pred.shape[0]
    table = check_map_table(offsets, L)
    G, S = len(table) - 1, len(temps)
    dev, dtype = pred.device, pred.dtype
    p, y = pred.detach(), label.detach()
    counts = torch.as_tensor(table[1:] - table[:-1], device=dev)
    begin = torch.as_tensor(table[:-1], device=dev)
    image = torch.repeat_interleave(torch.arange(G, device=dev), counts)                  # [L]: the image of a label
    within = torch.arange(L, device=dev) - begin[image]                                   # [L]: the index inside the image
    listed = counts >= 2
    zeros = torch.zeros(G, dtype=dtype, device=dev)
    low = torch.full((G,), float("-inf"), dtype=dtype, device=dev)

    def top(v):
        """(maximum [G], arg-max within the image [G]) with NaN below everything and ties to the lowest index."""
        v = torch.where(torch.isnan(v), torch.full_like(v, float("-inf")), v)
        m = low.scatter_reduce(0, image, v, "amax", include_self=True)
        k = torch.full((G,), L, dtype=torch.int64, device=dev).scatter_reduce(
            0, image, torch.where(v == m[image], within, torch.full_like(within, L)), "amin", include_self=True)
        return m, k

    total = lambda v: zeros.index_add(0, image, v)   # noqa: E731
    max_p, chosen = top(p)
    max_y, best = top(y)
    is_chosen, is_best = within == chosen[image], within == best[image]
    c = y / ty - (max_y / ty)[image]
    lq = c - torch.log1p(total(torch.where(is_best, torch.zeros_like(c), torch.exp(c))))[image]
    q = torch.exp(lq)
    d, u = p - max_p[image], y - max_y[image]
    counted = q != 0                                                                      # an underflowed q: exactly 0
    nothing = torch.zeros_like(q)
    q_lq = total(torch.where(counted, q * lq, nothing))
    q_d = total(torch.where(counted, q * d, nothing))
    q_sum = total(torch.where(counted, q, nothing))
    mark = total((p - p) + (y - y))                                                       # 0, or NaN for an image with a non-finite value
    beta = torch.as_tensor(1.0 / temps, dtype=dtype, device=dev)[:, None]                 # [S, 1]
    e = torch.exp(beta * d)                                                               # [S, L]
    totals = lambda v: torch.zeros((S, G), dtype=dtype, device=dev).index_add(1, image, v)   # noqa: E731
    rest = totals(torch.where(is_chosen, torch.zeros_like(e), e))                         # Z'
    z = 1.0 + rest
    mean_d = totals(e * d) / z
    spread = torch.clamp(totals(e * d * d) / z - mean_d * mean_d, min=0.0)
    at_chosen, at_best = (begin + chosen).clamp(max=L - 1), (begin + best).clamp(max=L - 1)   # (no labels: masked below)
    columns = [((q_lq - beta * q_d) + q_sum * torch.log1p(rest)) + mark, (mean_d - q_d) + mark, spread + mark,
               (max_y + totals(e * u) / z) + mark]
    draws = [torch.exp(beta * d[at_best]) / z + mark, 1.0 / z + mark]                       # s at the arg-max of y, of p
    blank = torch.zeros((S, G), dtype=dtype, device=dev)
    columns = [torch.where(listed, v, blank) for v in columns]
    rows = torch.stack(columns, dim=-1).permute(1, 0, 2).contiguous()                     # [G, S, 4]
    images = torch.stack([torch.where(listed, counts.to(dtype), zeros), torch.where(listed, max_y, zeros),
                          torch.where(listed, y[at_chosen], zeros), torch.where(listed, max_p + q_d, zeros)], dim=1)
    n_listed, n_labels = listed.sum(), (counts * listed).sum()
    weight = listed.to(dtype) if per_image else (counts * listed).to(dtype)
    norm = (n_listed if per_image else n_labels).clamp(min=1).to(dtype)
    mean = lambda v: torch.where(listed, v, blank).sum(dim=1) / n_listed.clamp(min=1).to(dtype)   # noqa: E731
    curve = torch.stack([(weight * columns[0]).sum(dim=1) / norm, (weight * columns[1]).sum(dim=1) / norm,
                         (weight * columns[2]).sum(dim=1) / norm, mean(max_y - columns[3]), mean(draws[0]), mean(draws[1]),
                         n_listed.to(dtype).expand(S), n_labels.to(dtype).expand(S)], dim=1)
    return curve, rows, images


class MapListSweep:
    """The launcher and the call counter of map_list_sweep (libflingsim fs_map_list_sweep, csrc/fs_mapsweep.hip: two launches)."""
    n_forward = 0    # kernel calls so far (the tests count them)

    @staticmethod
    def _launch(pred, label, offsets, temperatures, label_temperature, per_image):
        """(curve [S, 8], rows [G, S, 4], images [G, 4]), float64, of operands that are already what the kernels take; offsets a
        device int32 [G + 1] tensor, temperatures a float64 numpy [S] array."""
        import ctypes as C

        images, labels, S = offsets.shape[0] - 1, pred.shape[0], len(temperatures)
        curve = torch.empty((S, 8), dtype=torch.float64, device=pred.device)
        rows = torch.empty((images, S, 4), dtype=torch.float64, device=pred.device)
        table = torch.empty((images, 4), dtype=torch.float64, device=pred.device)
        work = work_buffer("fs_map_list_sweep_work_bytes", pred.device, images, labels, S)   # s at the two arg-maxes
        stream_call("fs_map_list_sweep", pred.device, pred, label, offsets, images, labels,
                    temperatures.ctypes.data_as(C.POINTER(C.c_double)), S, float(label_temperature), int(bool(per_image)), curve,
                    rows, table, work)
        return curve, rows, table


def map_list_sweep(pred, label, offsets, temperatures, label_temperature, per_image=False):
    """The listwise term of MapListFunction at S = 1 to 64 prediction temperatures at once, with its two derivatives in 1 / T and
    what a Boltzmann policy at each T earns on the recorded cells (libflingsim fs_map_list_sweep, csrc/fs_mapsweep.hip: ONE pass
    over the labels, two launches): (curve [S, 8], rows [G, S, 4], images [G, 4]) in float64 on pred's device -- map_list_sweep_torch
    has the columns, SWEEP_COLUMNS names the curve's.  pred and label [L], offsets a HOST integer array [G + 1] in CSR form
    (check_map_table), temperatures a sequence of numbers; ValueError before anything touches the library for a malformed table
    or a temperature (label_temperature included) that is not positive and finite with a finite reciprocal, also as a float.
    CUDA fp32 inputs go through the kernels (MapListSweep.n_forward counts those calls); anything else through
    map_list_sweep_torch in float64.  Not differentiable."""
    _sweep_operands("map_list_sweep", pred, label)
    temps, ty = _sweep_scalars("map_list_sweep", temperatures, label_temperature)
    table = check_map_table(offsets, pred.shape[0])
    if pred.is_cuda and pred.dtype == torch.float32:
        import numpy as np

        dev_offsets = torch.from_numpy(table.astype("int32")).to(pred.device)
        out = MapListSweep._launch(pred.detach().contiguous(), label.detach().contiguous(), dev_offsets, np.ascontiguousarray(temps), ty,
                                   per_image)
        MapListSweep.n_forward += 1
        return out
    return map_list_sweep_torch(pred.detach().double(), label.detach().double(), table, temps, ty, per_image)


def fit_temperature(pred, label, offsets, label_temperature, per_image=False, lo=1e-3, hi=1e2, points=33, rounds=8, ratio=1e-4):
    """The prediction temperature in [lo, hi] at which the listwise term of MapListFunction over these images is smallest, for a
    fixed label temperature: the term is convex in 1 / T, so it has one minimum or is smallest at an end.  A zoom over
    map_list_sweep, one sweep per round: the grid is t_k = exp(log lo + k (log hi - log lo) / (points - 1)) in float64 with t_0 = lo
    and t_last = hi exactly; the point with the smallest `list` is taken (the lowest index among equals); the zoom stops there
    when hi / lo < 1 + ratio or after `rounds` sweeps, and otherwise goes on between that point's two neighbours (the point itself
    at an end of the grid).  With the defaults the bracket's log-width shrinks 16-fold per round: six sweeps from five decades.
    Device tensors and host tensors walk the same rounds; one download of a [points, 8] curve per round.
    Returns {'temperature', 'list' (the term there), 'slope' (its derivative in 1 / T there), 'at_bound' (None, or 'low' / 'high'
    when the point is the original lo or hi: the minimum lies outside the range -- predictions that rank the labels backwards
    fit T -> infinity), 'sweeps', 'chosen' (the index taken in each round), 'first_curve' (the first round's curve: per
    temperature {'temperature', **SWEEP_COLUMNS})}.  A set without a listed image, or whose term is not finite, has nothing to
    fit: temperature, list and slope are None.  ValueError for 0 < lo < hi, points in 3..64, rounds >= 1 and ratio > 0 violated, and
    map_list_sweep's refusals."""
    import numpy as np

    _sweep_operands("fit_temperature", pred, label)
    try:
        lo, hi, ratio, points, rounds = float(lo), float(hi), float(ratio), int(points), int(rounds)
    except (TypeError, ValueError):
        raise ValueError("fit_temperature: lo, hi, ratio, points and rounds are numbers") from None
    if not (0.0 < lo < hi < float("inf") and 3 <= points <= 64 and rounds >= 1 and 0.0 < ratio < float("inf")):
        raise ValueError("fit_temperature: 0 < lo < hi, points in 3..64, rounds >= 1 and ratio > 0")
    _sweep_scalars("fit_temperature", [lo, hi], label_temperature)
    table = check_map_table(offsets, pred.shape[0])
    out = dict(temperature=None, list=None, slope=None, at_bound=None, sweeps=0, chosen=[], first_curve=[])
    if not (np.diff(table) >= 2).any():
        return out
    low, high = lo, hi
    while True:
        grid = np.exp(np.log(low) + np.arange(points) * (np.log(high) - np.log(low)) / (points - 1))
        grid[0], grid[-1] = low, high
        curve = map_list_sweep(pred, label, table, grid, label_temperature, per_image)[0].cpu().numpy()
        out["sweeps"] += 1
        if out["sweeps"] == 1:
            out["first_curve"] = [dict(temperature=float(t), **{name: float(v) for name, v in zip(SWEEP_COLUMNS, row)})
                                  for t, row in zip(grid, curve)]
        if not np.isfinite(curve[:, 0]).all():
            return out
        k = int(np.argmin(curve[:, 0]))
        out["chosen"].append(k)
        if high / low < 1.0 + ratio or out["sweeps"] >= rounds:
            break
        low, high = float(grid[max(k - 1, 0)]), float(grid[min(k + 1, points - 1)])
    t = float(grid[k])
    out.update(temperature=t, list=float(curve[k, 0]), slope=float(curve[k, 1]),
               at_bound="low" if t == lo else "high" if t == hi else None)
    return out


SCORE_COLUMNS = ("n", "chosen", "best", "chosen_rank", "pairs", "concordant", "Sab", "Saa", "Sbb", "spearman", "regret", "se")


def empty_score_rows(images):
    """[images, 12] float64 numpy: the row fs_map_score writes for an image without a counted position."""
    import numpy as np

    rows = np.zeros((int(images), len(SCORE_COLUMNS)), np.float64)
    rows[:, 1:4] = -1.0
    rows[:, 9:11] = np.nan
    return rows


def map_score_host(value, offsets, pix, label, min_gap=0.0):
    """fs_map_score (include/flingsim.h) in numpy on the host, image by image: value [G, S] (the dense maps, S values each), offsets
    int [G + 1], pix int [L], label [L] -> float64 [G, 12] rows (SCORE_COLUMNS).  Predictions and labels are taken as float32, as the
    kernel reads them.  The ranks come from a sort (searchsorted on both sides: the values below and the values equal), the pairs
    from an [n, n] comparison in float64: the CPU path of map_score."""
    import numpy as np

    value = np.asarray(value, np.float32)
    off, pix, label = np.asarray(offsets, np.int64), np.asarray(pix, np.int64), np.asarray(label, np.float32)
    rows = empty_score_rows(len(off) - 1)
    for b in range(len(off) - 1):
        p_all, y_all = value[b, pix[off[b]:off[b + 1]]], label[off[b]:off[b + 1]]
        keep = np.flatnonzero(np.isfinite(p_all) & np.isfinite(y_all))
        n = len(keep)
        if n == 0:
            continue
        p, y = p_all[keep], y_all[keep]
        p64, y64 = p.astype(np.float64), y.astype(np.float64)
        chosen, best = int(np.argmax(p)), int(np.argmax(y))          # (the first among equals)
        wins = y64[:, None] > y64[None, :] + float(min_gap)
        ranks = []
        for v in (p, y):
            s = np.sort(v)
            below, upto = np.searchsorted(s, v, "left"), np.searchsorted(s, v, "right")
            ranks.append((below + upto - n).astype(np.int64))         # 2 below + equal - n
        a, c = ranks
        sab, saa, sbb = int((a * c).sum()), int((a * a).sum()), int((c * c).sum())
        spearman = np.nan if n < 2 or saa == 0 or sbb == 0 else float(sab) / np.sqrt(float(saa) * float(sbb))
        rows[b] = (n, keep[chosen], keep[best], int((y > y[chosen]).sum()), int(wins.sum()),
                   int((wins & (p[:, None] > p[None, :])).sum()), sab, saa, sbb, spearman, y64[best] - y64[chosen],
                   float(((p64 - y64) ** 2).sum()))
    return rows


def map_score(value, offsets, pix, label, min_gap=0.0):
    """The rank statistics of a batch of recorded maps under the weights that wrote `value` (libflingsim fs_map_score,
    csrc/fs_mapscore.hip: one launch, one workgroup per image): value [G, 1, 64, 64] or [G, 4096], the dense maps of the eval
    forward; offsets a HOST integer array [G + 1] in CSR form, pix an integer [L] tensor of flat pixels, label [L] (what
    replay.MapSet.take_maps returns) -> float64 [G, 12] rows on value's device, SCORE_COLUMNS: n, chosen, best, chosen_rank, pairs,
    concordant, Sab, Saa, Sbb, spearman, regret, se per image over its positions with finite prediction and label
    (include/flingsim.h has the rule in full; summarize_scores turns rows into means).  The table is validated on the host first
    (check_map_table, and check_pixel_table on `pix.host` when the tensor carries its host copy): ValueError before anything
    touches the library.  CUDA fp32 maps go through the kernel; anything else through map_score_host."""
    if not (torch.is_tensor(value) and value.dim() in (2, 4) and value.shape[0] >= 1 and tuple(value.shape[1:]) in ((1, 64, 64), (4096,))):
        raise ValueError("map_score: value is a [G >= 1, 1, 64, 64] or [G, 4096] tensor")
    if not (torch.is_tensor(pix) and torch.is_tensor(label) and pix.dim() == 1 and label.shape == pix.shape
            and pix.dtype in (torch.int32, torch.int64) and label.is_floating_point()):
        raise ValueError("map_score: pix is an integer [L] tensor and label a floating-point [L] tensor")
    min_gap = float(min_gap)
    if not (0.0 <= min_gap < float("inf")):
        raise ValueError("map_score: min_gap >= 0 and finite")
    images = int(value.shape[0])
    table = check_map_table(offsets, pix.shape[0])
    if len(table) != images + 1:
        raise ValueError(f"map_score: offsets are integers [{images + 1}] for {images} maps, got [{len(table)}]")
    check_pixel_table(table, getattr(pix, "host", None), images)
    if value.is_cuda and value.dtype == torch.float32:
        if pix.device != value.device or label.device != value.device:
            raise ValueError("map_score: pix and label live on value's device")
        dense = operand(value.detach().reshape(images, 4096))
        rows = torch.empty((images, len(SCORE_COLUMNS)), dtype=torch.float64, device=value.device)
        stream_call("fs_map_score", value.device, dense, 4096, operand(pix.to(torch.int32)), operand(label.detach().to(torch.float32)),
                    torch.from_numpy(table.astype("int32")).to(value.device), images, int(pix.shape[0]), min_gap, rows)
        return rows
    rows = map_score_host(value.detach().reshape(images, 4096).float().cpu().numpy(), table, pix.cpu().numpy(),
                          label.detach().float().cpu().numpy(), min_gap)
    return torch.from_numpy(rows).to(value.device)


def summarize_scores(rows):
    """The rows of map_score, in image order, as one summary on the host in float64: n_maps (the rows with n >= 1), labels (sum of
    n), regret, chosen_rank (their means over those rows) and top1 (the fraction of them with chosen_rank == 0), spearman (the mean
    over the maps_with_spearman rows that have one), pairs, concordant (sums), pair_accuracy = concordant / pairs,
    map_pair_accuracy (the mean of C_b / P_b over the rows with pairs) and mse = sum of se / labels.  None where undefined.  The
    totals are formed from per-image rows, so they do not depend on how the set was cut into batches."""
    import numpy as np

    rows = np.asarray(rows.cpu() if torch.is_tensor(rows) else rows, np.float64).reshape(-1, len(SCORE_COLUMNS))
    filled = rows[rows[:, 0] >= 1]
    ranked = filled[np.isfinite(filled[:, 9])]
    paired = filled[filled[:, 4] > 0]
    labels, pairs, concordant = int(filled[:, 0].sum()), int(filled[:, 4].sum()), int(filled[:, 5].sum())
    mean = lambda v: float(np.mean(v)) if len(v) else None   # noqa: E731
    return dict(n_maps=int(len(filled)), labels=labels, regret=mean(filled[:, 10]), chosen_rank=mean(filled[:, 3]),
                top1=mean(filled[:, 3] == 0), spearman=mean(ranked[:, 9]), maps_with_spearman=int(len(ranked)), pairs=pairs,
                concordant=concordant, pair_accuracy=concordant / pairs if pairs else None,
                map_pair_accuracy=mean(paired[:, 5] / paired[:, 4]), mse=float(filled[:, 11].sum() / labels) if labels else None)
