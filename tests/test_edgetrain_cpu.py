"""What of the all-HIP value-net update (csrc/fs_edgetrain.hip, nets.ConvInFunction, nets.HeadPixelFunction, train.HipAdam) can
be checked without a GPU: the entry points exist in the header and in the library and refuse what they do not serve before any
HIP call, forward_selected on the host is the dense forward's pixel, the float64 restatement of Adam that judges the kernel on
the GPU is itself stock Adam, and the flags exist and default to off."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fs_convin_work_bytes", "fs_convin_forward", "fs_convin_wgrad", "fs_head_forward", "fs_head_backward", "fs_adam_step")


# ---- the float64 restatement of torch.optim.Adam that tests/test_edgetrain_gpu.py uses as its reference ---------------------
def adam_f64(params, grads, state, t, lr, betas, eps, weight_decay):
    """One Adam step, number `t` (1-based), in float64 on lists of tensors, in place: `params`, and `state` = (exp_avgs,
    exp_avg_sqs).  A grad of None skips its parameter.  The formulas are the issue's, which are torch.optim.Adam's."""
    beta1, beta2 = betas
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    for p, g, m, v in zip(params, grads, state[0], state[1]):
        if g is None:
            continue
        assert p.dtype == m.dtype == v.dtype == torch.float64
        g = g.double() + weight_decay * p
        m += (g - m) * (1.0 - beta1)
        v.mul_(beta2).add_((1.0 - beta2) * g * g)
        p -= (lr / bc1) * m / (v.sqrt() / np.sqrt(bc2) + eps)


def adam_gradients(sizes, step, seed, device="cpu"):
    """Gradients of step `step` for segments of `sizes` elements: magnitudes 10^u with u uniform in [-6, 1], random signs, one
    element in sixteen exactly 0.  A function of (seed, step) alone, never of the parameters."""
    gen = torch.Generator().manual_seed(1000 * seed + step)
    out = []
    for n in sizes:
        mag = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 7.0 - 6.0)
        sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
        zero = torch.rand(n, generator=gen) < 1.0 / 16.0
        out.append(torch.where(zero, torch.zeros((), dtype=torch.float64), mag * sign).float().to(device))
    return out


ADAM_SIZES = (1, 7, 16, 144, 432, 2304, 4099)


def adam_parameters(seed, dtype=torch.float32, device="cpu"):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=gen).to(dtype=dtype, device=device) for n in ADAM_SIZES]


# ---- header and library ------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    from flingbot_amd import sim as fsim

    with open(os.path.join(ROOT, "include", "flingsim.h")) as fh:
        header = fh.read()
    lib = fsim.load_library()
    for name in ENTRIES:
        assert re.search(r"^(size_t|int) " + name + r"\(", header, re.M), name
        assert getattr(lib, name) is not None
    assert "typedef struct fs_adam_segment" in header
    assert C.sizeof(fsim.AdamSegment) == 40


def _aligned():
    buf = np.zeros(8192, np.float32)
    base = (buf.ctypes.data + 63) // 64 * 64
    return buf, (lambda k: C.c_void_p(base + 64 * k)), C.c_void_p(base + 4), C.c_void_p(None)


def _refuses(lib, name, call, ok, cases):
    for kw in cases:
        assert call(**{**ok, **kw}) == -1, (name, kw)            # FS_ERR_ARG
        assert name.encode() in lib.fs_last_error(), (name, kw)


def test_entry_points_refuse_what_they_do_not_serve():
    """A null pointer, batch 0, dim 32, channels 2 or 5, a misaligned pointer: FS_ERR_ARG before any HIP call (the pointers are
    host addresses that are never dereferenced), and fs_last_error() names the entry."""
    from flingbot_amd import sim as fsim

    lib = fsim.load_library()
    buf, at, off, null = _aligned()
    shape = [dict(batch=0), dict(batch=-2), dict(dim=32)]
    channels = [dict(channels=2), dict(channels=5), dict(channels=0)]

    ok = dict(x=at(0), w=at(1), channels=3, batch=2, dim=64, y=at(2))
    call = lambda **a: lib.fs_convin_forward(a["x"], a["w"], a["channels"], a["batch"], a["dim"], a["y"], None)
    ptrs = ("x", "w", "y")
    _refuses(lib, "fs_convin_forward", call, ok, shape + channels + [{k: null} for k in ptrs] + [{k: off} for k in ptrs])

    ok = dict(x=at(0), g=at(1), channels=3, batch=2, dim=64, dw=at(2), work=at(3))
    call = lambda **a: lib.fs_convin_wgrad(a["x"], a["g"], a["channels"], a["batch"], a["dim"], a["dw"], a["work"], None)
    ptrs = ("x", "g", "dw", "work")
    _refuses(lib, "fs_convin_wgrad", call, ok, shape + channels + [{k: null} for k in ptrs] + [{k: off} for k in ptrs])

    ok = dict(h=at(0), w=at(1), pix=at(2), batch=2, dim=64, pred=at(3))
    call = lambda **a: lib.fs_head_forward(a["h"], a["w"], a["pix"], a["batch"], a["dim"], a["pred"], None)
    ptrs = ("h", "w", "pix", "pred")
    _refuses(lib, "fs_head_forward", call, ok, shape + [{k: null} for k in ptrs] + [{k: off} for k in ptrs])

    ok = dict(h=at(0), w=at(1), pix=at(2), gpred=at(3), batch=2, dim=64, dh=at(4), dw=at(5))
    call = lambda **a: lib.fs_head_backward(a["h"], a["w"], a["pix"], a["gpred"], a["batch"], a["dim"], a["dh"], a["dw"], None)
    ptrs = ("h", "w", "pix", "gpred", "dh", "dw")
    _refuses(lib, "fs_head_backward", call, ok, shape + [{k: null} for k in ptrs] + [{k: off} for k in ptrs] + [dict(dh=ok["h"])])


def test_adam_entry_point_refuses_what_it_does_not_serve():
    from flingbot_amd import sim as fsim

    lib = fsim.load_library()
    buf, at, off, null = _aligned()

    def table(**kw):
        seg = dict(param=at(0).value, grad=at(1).value, exp_avg=at(2).value, exp_avg_sq=at(3).value, count=16)
        seg.update(kw)
        t = (fsim.AdamSegment * 2)()
        t[0].param, t[0].grad, t[0].exp_avg, t[0].exp_avg_sq, t[0].count = at(4).value, at(5).value, at(6).value, at(7).value, 4
        t[1].param, t[1].grad, t[1].exp_avg, t[1].exp_avg_sq, t[1].count = seg["param"], seg["grad"], seg["exp_avg"], seg["exp_avg_sq"], seg["count"]
        return t

    ok = dict(table=table(), n=2, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, bc1=0.1, bc2=0.001)
    call = lambda **a: lib.fs_adam_step(a["table"], a["n"], a["lr"], a["beta1"], a["beta2"], a["eps"], a["wd"], a["bc1"], a["bc2"], None)
    cases = [dict(table=None), dict(n=0), dict(lr=-1.0), dict(beta1=1.0), dict(beta2=-0.1), dict(eps=-1e-8), dict(wd=-1.0),
             dict(bc1=0.0), dict(bc2=1.5), dict(lr=float("nan"))]
    cases += [dict(table=table(**{k: None})) for k in ("param", "grad", "exp_avg", "exp_avg_sq")]
    cases += [dict(table=table(**{k: at(0).value + 2})) for k in ("param", "grad", "exp_avg", "exp_avg_sq")]   # not a float address
    cases += [dict(table=table(count=0)), dict(table=table(count=-5))]
    _refuses(lib, "fs_adam_step", call, ok, cases)


def test_work_bytes():
    from flingbot_amd import sim as fsim

    lib = fsim.load_library()
    for args in ((2, 3, 64), (5, 3, 64), (0, 3, 64), (3, 0, 64), (3, -1, 64), (3, 3, 32)):
        assert lib.fs_convin_work_bytes(*args) == 0, args
    assert lib.fs_convin_work_bytes(3, 3, 64) > 0
    assert lib.fs_convin_work_bytes(1, 1, 64) > 0 and lib.fs_convin_work_bytes(4, 9, 64) > lib.fs_convin_work_bytes(3, 9, 64)


# ---- the Python surface on the host ------------------------------------------------------------------------------------------
def test_functions_and_switch_exist_and_refuse_host_tensors():
    from flingbot_amd import nets

    assert nets._TRAIN_EDGE_HIP is False
    with nets.train_edge_hip():
        assert nets._TRAIN_EDGE_HIP is True
        with nets.train_edge_hip(False):
            assert nets._TRAIN_EDGE_HIP is False
        assert nets._TRAIN_EDGE_HIP is True
    assert nets._TRAIN_EDGE_HIP is False
    with pytest.raises(RuntimeError):
        with nets.train_edge_hip():
            raise RuntimeError("inside")
    assert nets._TRAIN_EDGE_HIP is False
    for fn in (nets.ConvInFunction, nets.HeadPixelFunction):
        assert issubclass(fn, torch.autograd.Function) and isinstance(fn.n_forward, int) and isinstance(fn.n_backward, int)
    with pytest.raises(ValueError):
        nets.ConvInFunction.apply(torch.zeros(2, 3, 64, 64), torch.zeros(16, 3, 3, 3))
    with pytest.raises(ValueError):
        nets.HeadPixelFunction.apply(torch.zeros(2, 16, 64, 64), torch.zeros(1, 16, 3, 3), torch.zeros(2, dtype=torch.int32))


@pytest.mark.parametrize("mode", ["rgb", "depth", "rgbd"])
@pytest.mark.parametrize("training", [True, False])
def test_forward_selected_on_the_host_is_the_dense_forward(mode, training):
    """Bit for bit, with the edge switch on and off, and no Function is called."""
    import copy
    from flingbot_amd import nets

    torch.manual_seed(3)
    net = nets.SpatialValueNet(rgb_only=mode == "rgb", depth_only=mode == "depth", device="cpu")
    obs = torch.rand(3, 4, 64, 64)
    mask = torch.zeros(3, 64, 64, dtype=torch.bool)
    for k, (y, x) in enumerate(((0, 0), (63, 17), (20, 40))):
        mask[k, y, x] = True
    calls = (nets.ConvInFunction.n_forward, nets.HeadPixelFunction.n_forward)
    outs = []
    for edge in (False, True):
        a, b = copy.deepcopy(net).train(training), copy.deepcopy(net).train(training)
        with torch.no_grad(), nets.train_edge_hip(edge):
            got = a.forward_selected(obs, mask)
            want = torch.masked_select(b(obs).squeeze(1), mask)
        assert got.shape == (3,) and torch.equal(got, want), (mode, training, edge)
        outs.append(got)
    assert torch.equal(outs[0], outs[1])
    assert (nets.ConvInFunction.n_forward, nets.HeadPixelFunction.n_forward) == calls


@pytest.mark.parametrize("weight_decay", [0.0, 1e-6])
def test_float64_adam_restatement_is_stock_adam(weight_decay):
    """25 steps of adam_f64 against torch.optim.Adam on float64 CPU parameters: the same to rounding (a few ulp of float64: the
    two write the same formulas with differently associated products).  One parameter never gets a gradient."""
    lr, betas, eps = 1e-3, (0.9, 0.999), 1e-8
    params = [p.clone().requires_grad_(True) for p in adam_parameters(5, torch.float64)] + [torch.ones(3, dtype=torch.float64, requires_grad=True)]
    opt = torch.optim.Adam(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    mine = [p.detach().clone() for p in params]
    state = ([torch.zeros_like(p) for p in mine], [torch.zeros_like(p) for p in mine])
    for t in range(1, 26):
        grads = adam_gradients(ADAM_SIZES, t, 5) + [None]
        for p, g in zip(params, grads):
            p.grad = None if g is None else g.double()
        opt.step()
        adam_f64(mine, grads, state, t, lr, betas, eps, weight_decay)
    worst = 0.0
    for k, (p, q) in enumerate(zip(params, mine)):
        if k == len(params) - 1:
            assert torch.equal(q, torch.ones(3, dtype=torch.float64)) and p not in opt.state
            continue
        st = opt.state[p]
        for a, b in ((p.detach(), q), (st["exp_avg"], state[0][k]), (st["exp_avg_sq"], state[1][k])):
            rel = float(((a - b).abs() / b.abs().clamp_min(1e-300)).max())
            worst = max(worst, rel)
            assert float((a - b).abs().max()) <= 1e-13 * max(1.0, float(b.abs().max())), (k, rel)
    print(f"adam_f64 against stock float64 Adam, weight decay {weight_decay}: largest relative difference {worst:.2e}")


def test_hip_adam_refuses_what_it_does_not_serve():
    from flingbot_amd import train

    assert issubclass(train.HipAdam, torch.optim.Adam)
    p = torch.nn.Parameter(torch.ones(4))
    for flag in ("amsgrad", "maximize", "capturable", "differentiable", "fused"):
        with pytest.raises(ValueError):
            train.HipAdam([p], **{flag: True})
    opt = train.HipAdam([p], lr=1e-3, weight_decay=1e-6)
    stock = torch.optim.Adam([torch.nn.Parameter(torch.ones(4))], lr=1e-3, weight_decay=1e-6)
    assert opt.state_dict()["param_groups"] == stock.state_dict()["param_groups"]
    opt.step()                                  # no gradient anywhere: nothing to do, as for stock Adam
    assert len(opt.state) == 0
    p.grad = torch.ones(4)
    with pytest.raises(ValueError):
        opt.step()                              # a host parameter


def test_flags_exist_and_default_to_off():
    from flingbot_amd import nets, train

    a = train.build_parser().parse_args(["--log", "x", "--tasks", "y"])
    assert a.hip_step is False
    assert train.build_parser().parse_args(["--log", "x", "--tasks", "y", "--hip-step"]).hip_step is True
    for fn in (train.optimize, train.run):
        assert inspect.signature(fn).parameters["hip_step"].default is False
    assert inspect.signature(train.make_optimizer).parameters["hip"].default is False
    policy = nets.MaximumValuePolicy(action_primitives=["fling"], num_rotations=12, scale_factors=[1.0], obs_dim=64, pix_grasp_dist=8,
                                     pix_drag_dist=8, pix_place_dist=5, rgb_only=True, depth_only=False, action_expl_prob=0.0,
                                     action_expl_decay=1.0, value_expl_prob=0.0, value_expl_decay=1.0, device="cpu")
    assert type(train.make_optimizer(policy)) is torch.optim.Adam
    assert type(train.make_optimizer(policy, hip=True)) is train.HipAdam
