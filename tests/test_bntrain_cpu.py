"""What of the train-mode BatchNorm path (csrc/fs_bntrain.hip, nets.BatchNormAct16Function) can be checked without a GPU: the
entry points exist in the header and in the library, refuse what they do not serve before any HIP call, and the routing switch
changes nothing for a network on the host."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fs_bn16_work_bytes", "fs_bn16_forward", "fs_bn16_backward")


def test_header_declares_and_library_exports_the_entry_points():
    from flingbot_amd import sim as fsim

    with open(os.path.join(ROOT, "include", "flingsim.h")) as fh:
        header = fh.read()
    lib = fsim.load_library()
    for name in ENTRIES:
        assert re.search(r"^(size_t|int) " + name + r"\(", header, re.M), name
        assert getattr(lib, name) is not None
    for phrase in ("IN PLACE", "No atomics", "16-byte aligned", "STORED forward output", "z > 0 ? z : slope * z"):
        assert phrase in header, phrase


def test_bn16_entry_points_refuse_what_they_do_not_serve():
    """dim = 32, batch < 1, a null or misaligned pointer, one running pointer without the other, in place: FS_ERR_ARG before any
    HIP call (the pointers are host addresses that are never dereferenced)."""
    from flingbot_amd import sim as fsim

    lib = fsim.load_library()
    buf = np.zeros(4096, np.float32)
    base = (buf.ctypes.data + 63) // 64 * 64
    at = lambda k: C.c_void_p(base + 64 * k)
    off, null = C.c_void_p(base + 4), C.c_void_p(None)
    ok_fwd = dict(x=at(0), residual=at(1), gamma=at(2), beta=at(3), eps=1e-5, slope=0.0, momentum=0.1, running_mean=at(4),
                  running_var=at(5), batch=2, dim=64, y=at(6), save_mean=at(7), save_invstd=at(8), work=at(9))
    ok_bwd = dict(x=at(0), y=at(1), dy=at(2), gamma=at(3), save_mean=at(4), save_invstd=at(5), slope=0.0, batch=2, dim=64, dx=at(6),
                  dresidual=at(7), dgamma=at(8), dbeta=at(9), work=at(10))

    def fwd(**kw):
        a = {**ok_fwd, **kw}
        return lib.fs_bn16_forward(a["x"], a["residual"], a["gamma"], a["beta"], a["eps"], a["slope"], a["momentum"], a["running_mean"],
                                   a["running_var"], a["batch"], a["dim"], a["y"], a["save_mean"], a["save_invstd"], a["work"], None)

    def bwd(**kw):
        a = {**ok_bwd, **kw}
        return lib.fs_bn16_backward(a["x"], a["y"], a["dy"], a["gamma"], a["save_mean"], a["save_invstd"], a["slope"], a["batch"],
                                    a["dim"], a["dx"], a["dresidual"], a["dgamma"], a["dbeta"], a["work"], None)

    bad = [dict(dim=32), dict(batch=0), dict(batch=-3)]
    required = ("x", "gamma", "beta", "y", "save_mean", "save_invstd", "work")
    cases = bad + [{k: null} for k in required] + [{k: off} for k in required + ("residual", "running_mean", "running_var")]
    cases += [dict(running_mean=null), dict(running_var=null), dict(y=ok_fwd["x"])]
    for kw in cases:
        assert fwd(**kw) == -1, kw           # FS_ERR_ARG
        assert b"fs_bn16_forward" in lib.fs_last_error(), kw
    required = ("x", "y", "dy", "gamma", "save_mean", "save_invstd", "dx", "dgamma", "dbeta", "work")
    cases = bad + [{k: null} for k in required] + [{k: off} for k in required + ("dresidual",)] + [dict(dx=ok_bwd["dy"])]
    for kw in cases:
        assert bwd(**kw) == -1, kw
        assert b"fs_bn16_backward" in lib.fs_last_error(), kw
    assert lib.fs_bn16_work_bytes(0, 64) == 0 and lib.fs_bn16_work_bytes(3, 32) == 0
    assert lib.fs_bn16_work_bytes(3, 64) > 0


def test_function_and_switch_exist_and_refuse_host_tensors():
    from flingbot_amd import nets

    fn = nets.BatchNormAct16Function
    assert issubclass(fn, torch.autograd.Function) and isinstance(nets._TRAIN_BN_HIP, bool)
    assert isinstance(fn.n_forward, int) and isinstance(fn.n_backward, int)
    x = torch.zeros(2, 16, 64, 64)
    v = torch.ones(16)
    with pytest.raises(ValueError):
        fn.apply(x, v, v, None, v.clone(), v.clone(), 0.1, 1e-5, 0.0)


@pytest.mark.parametrize("conv_switch", [True, False])
def test_host_network_does_not_see_the_switch(conv_switch):
    """A CPU SpatialValueNet in train mode: outputs, gradients and the buffers after one step are the same bits with
    nets._TRAIN_BN_HIP on and off, and the Function is never called."""
    from flingbot_amd import nets

    torch.manual_seed(4)
    net = nets.SpatialValueNet(rgb_only=True, device="cpu").train()
    obs = torch.rand(2, 3, 64, 64)
    label = torch.rand(2, 1, 64, 64)
    saved = (nets._TRAIN_BN_HIP, nets._TRAIN_CONV_HIP)
    calls = (nets.BatchNormAct16Function.n_forward, nets.BatchNormAct16Function.n_backward)
    results = []
    try:
        nets._TRAIN_CONV_HIP = conv_switch
        for flag in (True, False):
            nets._TRAIN_BN_HIP = flag
            m = copy.deepcopy(net)
            opt = torch.optim.Adam(m.parameters(), lr=1e-3)
            out = m(obs)
            F.mse_loss(out, label).backward()
            grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
            opt.step()
            results.append((out.detach().clone(), grads, {k: v.clone() for k, v in m.state_dict().items()}))
    finally:
        nets._TRAIN_BN_HIP, nets._TRAIN_CONV_HIP = saved
    (out_a, grads_a, state_a), (out_b, grads_b, state_b) = results
    assert torch.equal(out_a, out_b)
    assert set(grads_a) == set(grads_b) and len(grads_a) == 2 + 16 + 2 * 17
    for k in grads_a:
        assert torch.equal(grads_a[k], grads_b[k]), k
    assert list(state_a) == list(state_b) == list(net.state_dict())
    for k in state_a:
        assert torch.equal(state_a[k], state_b[k]), k
    assert all(int(v) == 1 for k, v in state_a.items() if k.endswith("num_batches_tracked"))
    assert (nets.BatchNormAct16Function.n_forward, nets.BatchNormAct16Function.n_backward) == calls
