"""The all-HIP value-net update (csrc/fs_edgetrain.hip): the first layer (nets.ConvInFunction), the last layer at one pixel per
sample (nets.HeadPixelFunction) and Adam (train.HipAdam), one call at a time against float64, and the update that uses them
(train.optimize(hip_step=True), train.run(hip_step=True)).

The float64 references are F.conv2d and its autograd on the host, and for Adam the restatement adam_f64 of
tests/test_edgetrain_cpu.py (compared there with stock float64 Adam).  The bound everywhere is the project's own
(vn_reference.tolerance): max(4 e32, 2e-6 max(1, max |f64|)), where e32 is the larger error of the two stock fp32 paths -- host
and GPU -- on the same tensors.  Every comparison prints the kernel's error over e32."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_edgetrain_cpu as ec
import vn_reference as ref

pytestmark = pytest.mark.gpu

D = 64
DEV = "cuda:0"
CHANNELS = [1, 3, 4]
# where the first layer's kernels split an image: the forward's 8-row strips (rows 7 | 8, 15 | 16, ...) and its wavefronts'
# 4-row halves (3 | 4, 11 | 12, ...), the weight gradient's 16-row strips (15 | 16, 31 | 32, 47 | 48) and its 4-row groups, a
# quarter-wavefront's rows (every row), the float4 edges (columns 3 | 4, ..., 59 | 60) and the last column
ROWS = [0, 3, 4, 7, 8, 11, 12, 15, 16, 19, 20, 31, 32, 47, 48, 55, 56, 59, 60, 63]
COLS = [0, 3, 4, 31, 32, 59, 60, 62, 63]
POSITIONS = [(0, 0), (0, 63), (63, 0), (63, 63)] + [(r, COLS[k % len(COLS)]) for k, r in enumerate(ROWS)] + [(ROWS[k % len(ROWS)], c) for k, c in enumerate(COLS)]


def _nets():
    from flingbot_amd import nets
    return nets


def compare(what, out, f64, host, stock, failed):
    """`out` (device fp32) against `f64` under the bound; host / stock: the two stock fp32 results as float64 host tensors."""
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(f64.shape), what
    e32 = max(float((host - f64).abs().max()), float((stock - f64).abs().max()))
    err = float((out.double().cpu() - f64).abs().max())
    bound = ref.tolerance(e32, f64)
    ratio = err / e32 if e32 > 0 else 0.0
    print(f"{what}: err {err:.3e}  e32 {e32:.3e}  ratio {ratio:.2f}  bound {bound:.3e}  max|f64| {float(f64.abs().max()):.3e}")
    if not (bool(torch.isfinite(out).all()) and err <= bound):
        failed.append((what, err, e32, bound))
    return ratio


# ---- the first layer --------------------------------------------------------------------------------------------------------
def convin(x, w, g=None):
    """(y, dw or None) of the kernels for host tensors."""
    fn = _nets().ConvInFunction
    xd, wd = x.to(DEV).contiguous(), w.to(DEV).contiguous()
    y = fn._forward(xd, wd)
    return y, None if g is None else fn._wgrad(xd, g.to(DEV).contiguous())


def convin_stock(x, w, g, dtype, device):
    x, w = x.to(device=device, dtype=dtype), w.to(device=device, dtype=dtype).requires_grad_(True)
    y = F.conv2d(x, w, padding=1)
    (dw,) = torch.autograd.grad(y, w, g.to(device=device, dtype=dtype))
    return y.detach().double().cpu(), dw.double().cpu()


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("channels", CHANNELS)
def test_first_layer_ones_count_every_term(gpu_required, channels, batch):
    y, dw = convin(torch.ones(batch, channels, D, D), torch.ones(16, channels, 3, 3), torch.ones(batch, 16, D, D))
    count = F.conv2d(torch.ones(1, 1, D, D), torch.ones(1, 1, 3, 3), padding=1)[0, 0]      # 9 / 6 / 4
    assert float(count[5, 5]) == 9 and float(count[0, 5]) == 6 and float(count[63, 0]) == 4
    assert torch.equal(y.cpu(), (count * channels).expand(batch, 16, D, D))
    taps = torch.tensor([[3969.0, 4032.0, 3969.0], [4032.0, 4096.0, 4032.0], [3969.0, 4032.0, 3969.0]]) * batch
    assert torch.equal(dw.cpu(), taps.expand(16, channels, 3, 3))


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("channels", CHANNELS)
def test_first_layer_impulses_at_every_split_of_an_image(gpu_required, channels, batch):
    """Small-integer impulses at POSITIONS, spread over images and channels, against distinct small-integer weights (the forward)
    and small-integer fields (the weight gradient, impulses in x and then in g): every sum is an integer below 2^24, so the
    float64 reference is exact in fp32 whatever the order, and the comparison is for equality."""
    gen = torch.Generator().manual_seed(channels * 10 + batch)
    w = (torch.arange(16 * channels * 9, dtype=torch.float32) - 8 * channels * 9).reshape(16, channels, 3, 3)
    assert w.unique().numel() == w.numel()
    imp_x, imp_g = torch.zeros(batch, channels, D, D), torch.zeros(batch, 16, D, D)
    for k, (r, c) in enumerate(POSITIONS):
        imp_x[k % batch, k % channels, r, c] = 1 + k % 5
        imp_g[k % batch, (5 * k) % 16, r, c] = 1 + k % 3
    field_x = torch.randint(-3, 4, (batch, channels, D, D), generator=gen).float()
    field_g = torch.randint(-3, 4, (batch, 16, D, D), generator=gen).float()
    for what, x, g in (("impulses in x", imp_x, field_g), ("impulses in g", field_x, imp_g), ("impulses in both", imp_x, imp_g)):
        y, dw = convin(x, w, g)
        want_y, want_dw = convin_stock(x, w, g, torch.float64, "cpu")
        assert float(want_y.abs().max()) < 2 ** 24 and float(want_dw.abs().max()) < 2 ** 24
        assert torch.equal(y.double().cpu(), want_y), what
        assert torch.equal(dw.double().cpu(), want_dw), what


@pytest.mark.parametrize("batch", [1, 5, 9])
@pytest.mark.parametrize("channels", CHANNELS)
def test_first_layer_random_against_float64(gpu_required, channels, batch):
    gen = torch.Generator().manual_seed(100 * channels + batch)
    x = torch.randn(batch, channels, D, D, generator=gen)
    w = torch.randn(16, channels, 3, 3, generator=gen) * 0.3
    g = torch.randn(batch, 16, D, D, generator=gen)
    y, dw = convin(x, w, g)
    want = convin_stock(x, w, g, torch.float64, "cpu")
    host = convin_stock(x, w, g, torch.float32, "cpu")
    stock = convin_stock(x, w, g, torch.float32, DEV)
    failed = []
    compare(f"C={channels} B={batch} y", y, want[0], host[0], stock[0], failed)
    compare(f"C={channels} B={batch} dw", dw, want[1], host[1], stock[1], failed)
    assert not failed, failed


@pytest.mark.parametrize("channels", CHANNELS)
def test_first_layer_repeatability_and_batch_invariance(gpu_required, channels):
    gen = torch.Generator().manual_seed(7 + channels)
    x = torch.randn(9, channels, D, D, generator=gen)
    w = torch.randn(16, channels, 3, 3, generator=gen)
    g = torch.randn(9, 16, D, D, generator=gen)
    y, dw = convin(x, w, g)
    for _ in range(2):
        y2, dw2 = convin(x, w, g)
        assert torch.equal(y, y2) and torch.equal(dw, dw2)
    alone, _ = convin(x[:1], w)
    for index in (0, 4, 8):
        moved = x.clone()
        moved[index] = x[0]
        assert torch.equal(convin(moved, w)[0][index], alone[0]), index


def test_first_layer_function_takes_strided_and_offset_inputs(gpu_required):
    fn = _nets().ConvInFunction
    gen = torch.Generator().manual_seed(17)
    x = torch.randn(2, 3, D, D, generator=gen).to(DEV)
    w = torch.randn(16, 3, 3, 3, generator=gen).to(DEV)
    g = torch.randn(2, 16, D, D, generator=gen).to(DEV)

    def run(xi, wi, gi):
        wi = wi.detach().requires_grad_(True)
        y = fn.apply(xi, wi)
        y.backward(gi)
        return y.detach(), wi.grad

    def off(t):
        o = torch.empty(t.numel() + 1, device=DEV)[1:].view(t.shape).copy_(t)
        assert o.data_ptr() % 16 == 4
        return o

    def wide(t):
        v = torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), device=DEV)
        v[..., ::2] = t
        return v[..., ::2]

    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    want = run(x, w, g)
    before = (fn.n_forward, fn.n_backward)
    for form in (cl, off, wide):
        got = run(form(x), form(w), form(g))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), form
    assert (fn.n_forward, fn.n_backward) == (before[0] + 3, before[1] + 3)
    for bad in (x[:, :2], x[:, :, :32, :32], x.double(), x.clone().requires_grad_(True)):
        with pytest.raises(ValueError):
            fn.apply(bad, w)
    with pytest.raises(ValueError):
        fn.apply(x, w[:8])


# ---- the head -----------------------------------------------------------------------------------------------------------------
NINE = [(0, 0), (0, 63), (63, 0), (63, 63), (0, 31), (31, 0), (63, 31), (31, 63), (20, 40)]
HEAD_CASES = {"nine pixels": (NINE, 4), "two samples on one pixel": (NINE + [(20, 40), (63, 63)], 9)}   # (pixels, the sample with gpred = 0)


def head(h, w, pix, gpred=None):
    fn = _nets().HeadPixelFunction
    hd, wd = h.to(DEV).contiguous(), w.to(DEV).contiguous()
    pd = torch.tensor([y * D + x for y, x in pix], dtype=torch.int32, device=DEV)
    pred = fn._forward(hd, wd, pd)
    if gpred is None:
        return pred, None, None
    dh, dw = fn._backward(hd, wd, pd, gpred.to(DEV).contiguous())
    return pred, dh, dw


def head_stock(h, w, pix, gpred, dtype, device):
    """dense F.conv2d -> masked_select -> autograd."""
    h = h.to(device=device, dtype=dtype).requires_grad_(True)
    w = w.to(device=device, dtype=dtype).requires_grad_(True)
    mask = torch.zeros(len(pix), D, D, dtype=torch.bool)
    for k, (y, x) in enumerate(pix):
        mask[k, y, x] = True
    pred = torch.masked_select(F.conv2d(h, w, padding=1).squeeze(1), mask.to(device))
    dh, dw = torch.autograd.grad(pred, (h, w), gpred.to(device=device, dtype=dtype))
    return tuple(t.detach().double().cpu() for t in (pred, dh, dw))


def head_case(name, seed):
    pix, zero = HEAD_CASES[name]
    gen = torch.Generator().manual_seed(seed)
    h = torch.randn(len(pix), 16, D, D, generator=gen)
    w = torch.randn(1, 16, 3, 3, generator=gen) * 0.3
    gpred = torch.randn(len(pix), generator=gen)
    gpred[zero] = 0.0
    return pix, h, w, gpred


@pytest.mark.parametrize("name", list(HEAD_CASES))
def test_head_against_float64(gpu_required, name):
    pix, h, w, gpred = head_case(name, 31)
    pred, dh, dw = head(h, w, pix, gpred)
    want = head_stock(h, w, pix, gpred, torch.float64, "cpu")
    host = head_stock(h, w, pix, gpred, torch.float32, "cpu")
    stock = head_stock(h, w, pix, gpred, torch.float32, DEV)
    failed = []
    for k, (what, out) in enumerate((("pred", pred), ("dh", dh), ("dw", dw))):
        compare(f"head, {name}: {what}", out, want[k], host[k], stock[k], failed)
    assert not failed, failed
    # +0 bit for bit at every element outside the clipped patches
    outside = torch.ones(len(pix), 16, D, D, dtype=torch.bool)
    for k, (y, x) in enumerate(pix):
        outside[k, :, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = False
    bits = dh.cpu().view(torch.int32)
    assert int(outside.sum()) > 0 and bool((bits[outside] == 0).all())
    assert bool((want[1][outside] == 0).all())


def test_head_ones_count_every_term(gpu_required):
    pred, dh, dw = head(torch.ones(9, 16, D, D), torch.ones(1, 16, 3, 3), NINE, torch.ones(9))
    assert pred.cpu().tolist() == [64.0] * 4 + [96.0] * 4 + [144.0]
    count = torch.zeros(3, 3)      # how many of the nine samples have tap (ky, kx) inside the image
    for y, x in NINE:
        for ky in range(3):
            for kx in range(3):
                count[ky, kx] += 0 <= y + ky - 1 < D and 0 <= x + kx - 1 < D
    assert torch.equal(dw.cpu(), count.expand(1, 16, 3, 3))
    assert float(dh.sum()) == float(sum(pred.cpu().tolist()))


def test_head_three_calls_give_identical_bits(gpu_required):
    pix, h, w, gpred = head_case("two samples on one pixel", 33)
    first = head(h, w, pix, gpred)
    for _ in range(2):
        for a, b in zip(first, head(h, w, pix, gpred)):
            assert torch.equal(a, b)


def test_head_function_and_what_it_refuses(gpu_required):
    fn = _nets().HeadPixelFunction
    pix, h, w, gpred = head_case("nine pixels", 35)
    hd, wd = h.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    pd = torch.tensor([y * D + x for y, x in pix], device=DEV)            # int64, as argmax gives it
    before = (fn.n_forward, fn.n_backward)
    pred = fn.apply(hd, wd, pd)
    pred.backward(gpred.to(DEV))
    assert (fn.n_forward, fn.n_backward) == (before[0] + 1, before[1] + 1)
    want = head(h, w, pix, gpred)
    assert torch.equal(pred.detach(), want[0]) and torch.equal(hd.grad, want[1]) and torch.equal(wd.grad, want[2])
    with pytest.raises(ValueError):
        fn.apply(hd[:, :8], wd, pd)
    with pytest.raises(ValueError):
        fn.apply(hd, wd, pd[:4])
    with pytest.raises(ValueError):
        fn.apply(hd, wd, pd.float())


# ---- Adam -----------------------------------------------------------------------------------------------------------------------
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8


class AdamPaths:
    """The same parameters under four optimizers: HipAdam on the GPU, stock fp32 Adam on the host and on the GPU, adam_f64.
    The last parameter of each never gets a gradient."""

    def __init__(self, seed, weight_decay):
        from flingbot_amd import train

        self.seed, self.wd, self.t = seed, weight_decay, 0
        make = lambda device: [torch.nn.Parameter(p) for p in ec.adam_parameters(seed, device=device)] + [torch.nn.Parameter(torch.ones(5, device=device))]
        self.hip, self.host, self.stock = make(DEV), make("cpu"), make(DEV)
        kw = dict(lr=LR, betas=BETAS, eps=EPS, weight_decay=weight_decay)
        self.opt_hip, self.opt_host, self.opt_stock = train.HipAdam(self.hip, **kw), torch.optim.Adam(self.host, **kw), torch.optim.Adam(self.stock, **kw)
        self.f64 = [p.detach().double().cpu().clone() for p in self.host]
        self.f64_state = ([torch.zeros_like(p) for p in self.f64], [torch.zeros_like(p) for p in self.f64])

    def step(self):
        self.t += 1
        grads = ec.adam_gradients(ec.ADAM_SIZES, self.t, self.seed) + [None]
        for params, opt in ((self.hip, self.opt_hip), (self.host, self.opt_host), (self.stock, self.opt_stock)):
            for p, g in zip(params, grads):
                p.grad = None if g is None else g.to(p.device).clone()
            opt.step()
        ec.adam_f64(self.f64, grads, self.f64_state, self.t, LR, BETAS, EPS, self.wd)

    def check(self, what):
        failed = []
        for k, n in enumerate(ec.ADAM_SIZES):
            rows = (("p", lambda ps, opt: ps[k].detach(), self.f64[k]),
                    ("exp_avg", lambda ps, opt: opt.state[ps[k]]["exp_avg"], self.f64_state[0][k]),
                    ("exp_avg_sq", lambda ps, opt: opt.state[ps[k]]["exp_avg_sq"], self.f64_state[1][k]))
            for name, get, want in rows:
                compare(f"{what} n={n} {name}", get(self.hip, self.opt_hip), want, get(self.host, self.opt_host).double(),
                        get(self.stock, self.opt_stock).double().cpu(), failed)
        assert not failed, failed
        last = self.hip[-1]
        assert torch.equal(last.detach().cpu(), torch.ones(5)) and last not in self.opt_hip.state


@pytest.mark.parametrize("weight_decay", [0.0, 1e-6])
def test_adam_against_float64(gpu_required, weight_decay):
    from flingbot_amd import train

    paths = AdamPaths(11, weight_decay)
    launches = train.HipAdam.n_launches
    paths.step()
    assert train.HipAdam.n_launches == launches + 1          # seven segments, one launch
    paths.check(f"Adam wd={weight_decay} after 1 step")
    for _ in range(24):
        paths.step()
    paths.check(f"Adam wd={weight_decay} after 25 steps")
    # the state_dict is stock Adam's: keys, dtypes, shapes, devices
    mine, theirs = paths.opt_hip.state_dict(), paths.opt_stock.state_dict()
    assert mine["param_groups"] == theirs["param_groups"] and list(mine["state"]) == list(theirs["state"]) == list(range(len(ec.ADAM_SIZES)))
    for k in mine["state"]:
        assert list(mine["state"][k]) == list(theirs["state"][k]) == ["step", "exp_avg", "exp_avg_sq"]
        for name in mine["state"][k]:
            a, b = mine["state"][k][name], theirs["state"][k][name]
            assert (a.dtype, a.shape, a.device) == (b.dtype, b.shape, b.device), (k, name)
        assert float(mine["state"][k]["step"]) == 25.0


def test_adam_state_loads_in_both_directions(gpu_required):
    """After 5 steps the HipAdam state goes into a stock Adam and the stock state into a HipAdam (over swapped parameter
    values, too); one more step each way ends where the float64 path ends, under the bound."""
    from flingbot_amd import train

    paths = AdamPaths(12, 1e-6)
    for _ in range(5):
        paths.step()
    kw = dict(lr=LR, betas=BETAS, eps=EPS, weight_decay=1e-6)
    from_hip = [torch.nn.Parameter(p.detach().clone()) for p in paths.hip]
    from_stock = [torch.nn.Parameter(p.detach().clone()) for p in paths.stock]
    stock_opt, hip_opt = torch.optim.Adam(from_hip, **kw), train.HipAdam(from_stock, **kw)
    stock_opt.load_state_dict(copy.deepcopy(paths.opt_hip.state_dict()))
    hip_opt.load_state_dict(copy.deepcopy(paths.opt_stock.state_dict()))
    paths.step()
    grads = ec.adam_gradients(ec.ADAM_SIZES, paths.t, paths.seed, DEV) + [None]
    for params, opt in ((from_hip, stock_opt), (from_stock, hip_opt)):
        for p, g in zip(params, grads):
            p.grad = g
        opt.step()
    failed = []
    for k, n in enumerate(ec.ADAM_SIZES):
        host, stock = paths.host[k].detach().double(), paths.stock[k].detach().double().cpu()
        compare(f"HipAdam state -> stock Adam, n={n}", from_hip[k].detach(), paths.f64[k], host, stock, failed)
        compare(f"stock state -> HipAdam, n={n}", from_stock[k].detach(), paths.f64[k], host, stock, failed)
        assert float(hip_opt.state[from_stock[k]]["step"]) == float(stock_opt.state[from_hip[k]]["step"]) == 6.0
    assert not failed, failed


def test_adam_refuses_other_gradients(gpu_required):
    """torch itself keeps a gradient's dtype and device those of its parameter, so a gradient that is not CUDA fp32 belongs to a
    parameter that is not: float64 on the GPU here, fp32 on the host in tests/test_edgetrain_cpu.py."""
    from flingbot_amd import train

    p = torch.nn.Parameter(torch.ones(8, device=DEV, dtype=torch.float64))
    opt = train.HipAdam([p])
    p.grad = torch.ones(8, device=DEV, dtype=torch.float64)
    with pytest.raises(ValueError):
        opt.step()
    assert torch.equal(p.detach().cpu(), torch.ones(8, dtype=torch.float64)) and len(opt.state) == 0


# ---- a real network ---------------------------------------------------------------------------------------------------------------
def _net(seed, **mode):
    torch.manual_seed(seed)
    mode = mode or dict(rgb_only=True)
    net = _nets().SpatialValueNet(device=DEV, **mode).to(DEV)
    return ref.randomise_bn(net, seed)


def _batch(batch, seed):
    rng = np.random.default_rng(seed)
    obs = ref.make_obs(batch, seed, channels=3)
    mask = torch.zeros(batch, D, D, dtype=torch.bool)
    for k in range(batch):
        mask[k, int(rng.integers(8, 56)), int(rng.integers(8, 56))] = True
    label = torch.from_numpy(rng.uniform(-0.1, 0.2, batch).astype(np.float32))
    return obs, mask, label


class OneBatch:
    """What train.optimize asks of a data set, serving one fixed batch."""

    def __init__(self, obs, mask, label):
        self.batch = (obs, mask, label)

    def __len__(self):
        return int(self.batch[0].shape[0])

    def sample(self, batch_size, rng):
        assert batch_size == len(self)
        return self.batch


def test_recorded_sites_of_a_real_step(gpu_required):
    """The operands of the first layer and of the head in one optimize(hip_step=True) step (rgb net, B = 8), recorded where the
    Functions hand them to the kernels, replayed against float64."""
    from flingbot_amd import nets, train

    net = _net(41).train()
    data = OneBatch(*(t.to(DEV) for t in _batch(8, 41)))
    opt = train.HipAdam(net.parameters(), lr=1e-3, weight_decay=1e-6)
    seen = {}
    saved = (nets.ConvInFunction._forward, nets.ConvInFunction._wgrad, nets.HeadPixelFunction._forward, nets.HeadPixelFunction._backward)

    def record(key, inner):
        def call(*args):
            seen[key] = tuple(a.detach().clone().cpu() for a in args)
            return inner(*args)
        return staticmethod(call)

    try:
        nets.ConvInFunction._forward, nets.ConvInFunction._wgrad = record("in_fwd", saved[0]), record("in_wgrad", saved[1])
        nets.HeadPixelFunction._forward, nets.HeadPixelFunction._backward = record("head_fwd", saved[2]), record("head_bwd", saved[3])
        losses = train.optimize("fling", net, opt, data, 1, 8, np.random.default_rng(0), hip_step=True)
    finally:
        nets.ConvInFunction._forward, nets.ConvInFunction._wgrad = staticmethod(saved[0]), staticmethod(saved[1])
        nets.HeadPixelFunction._forward, nets.HeadPixelFunction._backward = staticmethod(saved[2]), staticmethod(saved[3])
    assert len(losses) == 1 and set(seen) == {"in_fwd", "in_wgrad", "head_fwd", "head_bwd"}
    x, w = seen["in_fwd"]
    x2, g = seen["in_wgrad"]
    assert tuple(x.shape) == (8, 3, D, D) and torch.equal(x, x2) and tuple(g.shape) == (8, 16, D, D) and float(g.abs().max()) > 0
    failed = []
    y, dw = convin(x, w, g)
    want, host, stock = (convin_stock(x, w, g, dt, dv) for dt, dv in ((torch.float64, "cpu"), (torch.float32, "cpu"), (torch.float32, DEV)))
    compare("recorded first layer y", y, want[0], host[0], stock[0], failed)
    compare("recorded first layer dw", dw, want[1], host[1], stock[1], failed)
    h, hw, pix, gpred = seen["head_bwd"]
    assert torch.equal(h, seen["head_fwd"][0]) and tuple(h.shape) == (8, 16, D, D) and pix.dtype == torch.int32 and float(gpred.abs().max()) > 0
    pixels = [divmod(int(p), D) for p in pix]
    assert pixels == [tuple(int(v) for v in m.nonzero()[0]) for m in data.batch[1].cpu()]
    got = head(h, hw, pixels, gpred)
    want, host, stock = (head_stock(h, hw, pixels, gpred, dt, dv) for dt, dv in ((torch.float64, "cpu"), (torch.float32, "cpu"), (torch.float32, DEV)))
    for k, what in enumerate(("pred", "dh", "dw")):
        compare(f"recorded head {what}", got[k], want[k], host[k], stock[k], failed)
    assert not failed, failed


def test_wiring_of_a_hip_step(gpu_required, monkeypatch):
    """With F.conv2d and F.batch_norm made to raise, an optimize(hip_step=True) update with a HipAdam completes: one first-layer
    call and one head call, forward and backward, one fs_adam_step, value_net.steps + 1, and the library's determinism switch
    is never touched."""
    from flingbot_amd import nets, train

    net = _net(43).train()
    data = OneBatch(*(t.to(DEV) for t in _batch(8, 43)))
    opt = train.HipAdam(net.parameters(), lr=1e-3, weight_decay=1e-6)
    before_state = {k: v.clone() for k, v in net.state_dict().items()}

    def refuse(*args, **kwargs):
        raise AssertionError("a library operator was called inside a hip_step update")

    deterministic = torch.backends.cudnn.deterministic
    monkeypatch.setattr(F, "conv2d", refuse)
    monkeypatch.setattr(F, "batch_norm", refuse)
    fns = (nets.ConvInFunction, nets.HeadPixelFunction, nets.Conv16Function, nets.BatchNormAct16Function)
    calls = [(f.n_forward, f.n_backward) for f in fns]
    launches, steps = train.HipAdam.n_launches, int(net.steps)
    entered = []
    real = train.deterministic_library_convs
    monkeypatch.setattr(train, "deterministic_library_convs", lambda *a, **k: (entered.append(1), real(*a, **k))[1])
    losses = train.optimize("fling", net, opt, data, 1, 8, np.random.default_rng(0), hip_step=True)
    monkeypatch.undo()
    assert len(losses) == 1 and np.isfinite(losses[0])
    assert [(f.n_forward - c[0], f.n_backward - c[1]) for f, c in zip(fns, calls)] == [(1, 1), (1, 1), (16, 16), (17, 17)]
    assert train.HipAdam.n_launches == launches + 1 and int(net.steps) == steps + 1
    assert not entered and torch.backends.cudnn.deterministic == deterministic
    assert nets._TRAIN_EDGE_HIP is False
    after = net.state_dict()
    changed = [k for k in after if not torch.equal(after[k], before_state[k])]
    assert len(changed) == len(after), sorted(set(after) - set(changed))     # every weight, buffer and counter moved


@pytest.mark.parametrize("mode", ["rgb", "depth", "rgbd"])
def test_forward_selected_agrees_with_the_dense_forward(gpu_required, mode):
    """forward_selected with the edge switch on against masked_select of the switch-off dense forward, same net and batch: both
    within the bound of the float64 train-mode forward, e32 from the host and the all-stock GPU forward."""
    from flingbot_amd import nets

    flags = dict(rgb_only=mode == "rgb", depth_only=mode == "depth")
    net = _net(47, **flags)
    obs = ref.make_obs(8, 47)
    _, mask, _ = _batch(8, 47)
    sel = lambda out: torch.masked_select(out.squeeze(1), mask.to(out.device))
    with torch.no_grad():
        want = sel(copy.deepcopy(net).cpu().double().train()(obs.double()))
        host = sel(copy.deepcopy(net).cpu().train()(obs)).double()
        saved = (nets._TRAIN_CONV_HIP, nets._TRAIN_BN_HIP)
        try:
            nets._TRAIN_CONV_HIP, nets._TRAIN_BN_HIP = False, False
            stock = sel(copy.deepcopy(net).train()(obs.to(DEV))).double().cpu()
        finally:
            nets._TRAIN_CONV_HIP, nets._TRAIN_BN_HIP = saved
        dense = sel(copy.deepcopy(net).train()(obs.to(DEV)))
        calls = (nets.ConvInFunction.n_forward, nets.HeadPixelFunction.n_forward)
        with nets.train_edge_hip():
            got = copy.deepcopy(net).train().forward_selected(obs.to(DEV), mask.to(DEV))
        assert (nets.ConvInFunction.n_forward, nets.HeadPixelFunction.n_forward) == (calls[0] + 1, calls[1] + 1)
        eval_net = copy.deepcopy(net).eval()
        with nets.train_edge_hip():
            assert torch.equal(eval_net.forward_selected(obs.to(DEV), mask.to(DEV)), sel(eval_net(obs.to(DEV))))
    failed = []
    compare(f"{mode}: forward_selected, switch on", got, want, host, stock, failed)
    compare(f"{mode}: dense forward, switch off", dense, want, host, stock, failed)
    assert not failed, failed


def _updates(n_updates, batch, n_samples, seed=0):
    import test_vntrain_gpu as vt
    from flingbot_amd import nets, train

    torch.manual_seed(seed)
    net = nets.SpatialValueNet(rgb_only=True, device=DEV).to(DEV)
    opt = train.HipAdam(net.parameters(), lr=1e-3, weight_decay=1e-6)
    data = vt.learning_set(n=n_samples).to_device(DEV)
    net.train()
    losses = train.optimize("fling", net, opt, data, n_updates, batch, np.random.default_rng(seed), hip_step=True)
    net.eval()
    return losses, net, opt


def test_two_runs_end_with_the_same_bits(gpu_required):
    """30 updates at B = 16 from one seed, twice, outside deterministic_library_convs(): every entry of the state_dict and of
    the optimizer's state is the same, bit for bit."""
    assert torch.backends.cudnn.deterministic is False
    losses, net, opt = _updates(30, 16, 64)
    losses_again, net_again, opt_again = _updates(30, 16, 64)
    assert len(losses) == 30 and all(np.isfinite(losses)) and losses == losses_again and int(net.steps) == 30
    a, b = net.state_dict(), net_again.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    sa, sb = opt.state_dict()["state"], opt_again.state_dict()["state"]
    assert list(sa) == list(sb) and len(sa) == 2 + 16 + 2 * 17
    for k in sa:
        for name in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(sa[k][name], sb[k][name]), (k, name)


def test_hip_step_learns(gpu_required):
    losses, _, _ = _updates(60, 16, 64)
    first, last = float(np.mean(losses[:10])), float(np.mean(losses[50:60]))
    print(f"mean loss of updates 1-10 {first:.4e}, of updates 51-60 {last:.4e}")
    assert all(np.isfinite(losses)) and last < first


def test_train_run_with_hip_step_twice_from_scratch(gpu_required, tmp_path):
    """The sizes of test_vntrain_gpu.test_train_run_end_to_end: two runs of two rounds from scratch with hip_step=True and a
    HipAdam leave identical replay files and identical final checkpoints."""
    import random

    from flingbot_amd import nets, sim as fsim, tasks as ftasks, train
    from flingbot_amd.env import BatchedFlingEnv

    random.seed(1); np.random.seed(1); torch.manual_seed(1)
    n = 3
    gen = fsim.FlingSim(n_envs=n, solver=0)
    tasks = ftasks.generate_tasks(gen, [ftasks.draw_task_parameters(min_cloth_size=24, strict_min_edge_length=24, max_cloth_size=32) for _ in range(n)])
    gen.close()

    def fresh(env):
        torch.manual_seed(7)
        policy = nets.MaximumValuePolicy(action_primitives=["fling"], num_rotations=12, scale_factors=list(env.scale_factors),
                                         obs_dim=64, pix_grasp_dist=8, pix_drag_dist=8, pix_place_dist=5, rgb_only=True,
                                         depth_only=False, action_expl_prob=0.5, action_expl_decay=0.9, value_expl_prob=0.5,
                                         value_expl_decay=0.9, device=DEV)
        return policy, train.make_optimizer(policy, hip=True)

    logs = [str(tmp_path / "a"), str(tmp_path / "b")]
    launches = train.HipAdam.n_launches
    ctx = fsim.FlingSim(n_envs=n, solver=0)
    try:
        env = BatchedFlingEnv(ctx, image_dim=128, episode_length=2, record_experience=True)
        for log_dir in logs:
            policy, opt = fresh(env)
            assert type(opt) is train.HipAdam
            out = train.run(policy, opt, env, tasks, log_dir, rounds=2, tasks_per_round=n, seed=3, batch_size=2, warmup=0, hip_step=True)
            assert out["rounds"][-1]["updates"] > 0 and int(policy.steps()) > 0
    finally:
        ctx.close()
    assert train.HipAdam.n_launches > launches and torch.backends.cudnn.deterministic is False
    names = [[os.path.basename(p) for p in train.replay_files(d)] for d in logs]
    assert names[0] == names[1] == ["replay_00000.npz", "replay_00001.npz"]
    for name in names[0]:
        a, b = (np.load(os.path.join(d, name), allow_pickle=False) for d in logs)
        assert set(a.files) == set(b.files)
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (name, k)
    ckpts = [torch.load(os.path.join(d, train.LATEST), map_location="cpu") for d in logs]
    for k, v in ckpts[0]["net"].items():
        assert torch.equal(v, ckpts[1]["net"][k]), k
    sa, sb = ckpts[0]["optimizer"]["state"], ckpts[1]["optimizer"]["state"]
    assert list(sa) == list(sb) and len(sa) > 0
    for k in sa:
        for name in sa[k]:
            assert torch.equal(sa[k][name], sb[k][name]), (k, name)
