"""The value net's training operators in libflingsim as autograd Functions: Conv16Function (csrc/fs_vntrain.hip),
BatchNormAct16Function (csrc/fs_bntrain.hip), ConvInFunction and HeadPixelFunction (csrc/fs_edgetrain.hip).  nets.py decides
which layer goes through which of them and re-exports the four classes; train.HipAdam is the optimizer's step.

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
