"""The train-mode BatchNorm kernels (csrc/fs_bntrain.hip) through nets.BatchNormAct16Function, one call at a time against
float64, and the network that routes its 17 BatchNorm sites through them.

The float64 reference is F.batch_norm(training=True) plus the activation on the host.  For the backward the activation is
written as a multiplication by where(y > 0, 1, slope) with y the KERNEL's own forward output: that map is linear, autograd gives
its exact gradient under the kernel's mask, no element is left out of a comparison, and a sign that fp32 and float64 decide
differently within rounding of zero cannot fail a correct kernel.  The bound is the project's own (vn_reference.tolerance):
max(4 e32, 2e-6 max(1, max |f64|)), where e32 is the larger error of the two stock fp32 paths on the same tensors -- host and GPU
F.batch_norm with the same mask factor.  It is applied to y, save_mean, save_invstd, both running buffers, dx, dresidual, dgamma
and dbeta.  (save_mean / save_invstd of the stock paths come from torch.native_batch_norm, the one stock interface that returns
them.)  slope is the float32 value the kernel receives, in every path."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vn_reference as ref

pytestmark = pytest.mark.gpu

D = 64
DEV = "cuda:0"
EPS, MOMENTUM = 1e-5, 0.1
# where a channel's work is split: between float4s of neighbouring threads (3 | 4), between wavefronts (255 | 256), between a
# thread's four float4s (1023 | 1024), between planes = workgroups (4095 | 0 of the next image)
POSITIONS = [0, 3, 4, 255, 256, 1023, 1024, 4095]
IMAGES = [0, 4, 8]


def _fn():
    from flingbot_amd import nets
    return nets.BatchNormAct16Function


def _slope32(slope):
    return float(np.float32(slope))


class Case:
    """Host fp32 tensors of one call: x, gamma, beta, residual (or None), dy, the running buffers before the call."""

    def __init__(self, x, gamma, beta, residual, dy, slope, running_mean=None, running_var=None, eps=EPS, momentum=MOMENTUM):
        self.x, self.gamma, self.beta, self.residual, self.dy = x, gamma, beta, residual, dy
        self.slope, self.eps, self.momentum = _slope32(slope), float(eps), float(momentum)
        self.running_mean = torch.zeros(16) if running_mean is None else running_mean
        self.running_var = torch.ones(16) if running_var is None else running_var


def random_case(batch, slope, with_residual, seed, mean=0.0, std=1.0):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, 16, D, D, generator=gen) * std + mean
    gamma = torch.rand(16, generator=gen) + 0.5
    beta = torch.randn(16, generator=gen)
    residual = torch.randn(batch, 16, D, D, generator=gen) if with_residual else None
    dy = torch.randn(batch, 16, D, D, generator=gen)
    return Case(x, gamma, beta, residual, dy, slope, torch.randn(16, generator=gen) * 0.2, torch.rand(16, generator=gen) + 0.5)


NAMES = ("y", "save_mean", "save_invstd", "running_mean", "running_var", "dx", "dgamma", "dbeta", "dresidual")


def hip_outputs(case):
    """The nine outputs of the kernels as device tensors (dresidual None without a residual)."""
    fn = _fn()
    dev = lambda t: None if t is None else t.to(DEV).contiguous()
    x, gamma, beta, res, dy = dev(case.x), dev(case.gamma), dev(case.beta), dev(case.residual), dev(case.dy)
    rm, rv = dev(case.running_mean).clone(), dev(case.running_var).clone()
    y, save_mean, save_invstd = fn._forward(x, gamma, beta, res, rm, rv, case.momentum, case.eps, case.slope)
    dx, dres, dgamma, dbeta = fn._backward(x, y, dy, gamma, save_mean, save_invstd, case.slope, res is not None)
    return dict(y=y, save_mean=save_mean, save_invstd=save_invstd, running_mean=rm, running_var=rv, dx=dx, dgamma=dgamma,
                dbeta=dbeta, dresidual=dres)


def stock_outputs(case, y_mask, dtype, device):
    """The same outputs of the stock operators in `dtype` on `device`, as float64 host tensors; the backward's mask factor is
    where(y_mask > 0, 1, slope)."""
    to = lambda t: t.detach().to(device=device, dtype=dtype)   # (detach: requires_grad_ below must not reach the case)
    x, gamma, beta = (to(t).requires_grad_(True) for t in (case.x, case.gamma, case.beta))
    res = None if case.residual is None else to(case.residual).requires_grad_(True)
    rm, rv = to(case.running_mean).clone(), to(case.running_var).clone()
    z = F.batch_norm(x, rm, rv, gamma, beta, True, case.momentum, case.eps)
    if res is not None:
        z = z + res
    y = torch.where(z > 0, z, z * case.slope)
    one = torch.ones((), dtype=dtype, device=device)
    factor = torch.where(y_mask.to(device) > 0, one, one * case.slope)
    inputs = (x, gamma, beta) + (() if res is None else (res,))
    grads = torch.autograd.grad(z * factor, inputs, to(case.dy))
    with torch.no_grad():
        _, save_mean, save_invstd = torch.native_batch_norm(x, gamma, beta, None, None, True, case.momentum, case.eps)
    out = dict(y=y, save_mean=save_mean, save_invstd=save_invstd, running_mean=rm, running_var=rv, dx=grads[0], dgamma=grads[1],
               dbeta=grads[2], dresidual=None if res is None else grads[3])
    return {k: None if v is None else v.detach().double().cpu() for k, v in out.items()}


def check_case(case, what):
    """The kernels on `case` against float64 under the bound of the module docstring; returns {name: kernel error / e32}."""
    got = hip_outputs(case)
    y_mask = got["y"].cpu()
    want = stock_outputs(case, y_mask, torch.float64, "cpu")
    host = stock_outputs(case, y_mask, torch.float32, "cpu")
    stock = stock_outputs(case, y_mask, torch.float32, DEV)
    ratios, failed = {}, []
    for name in NAMES:
        f64 = want[name]
        if f64 is None:
            assert got[name] is None
            continue
        out = got[name]
        assert out.dtype == torch.float32 and tuple(out.shape) == tuple(f64.shape), name
        e32 = max(float((host[name] - f64).abs().max()), float((stock[name] - f64).abs().max()))
        err = float((out.double().cpu() - f64).abs().max())
        bound = ref.tolerance(e32, f64)
        ratios[name] = err / e32 if e32 > 0 else 0.0
        print(f"{what} {name}: err {err:.3e}  e32 {e32:.3e}  ratio {ratios[name]:.2f}  bound {bound:.3e}  max|f64| {float(f64.abs().max()):.3e}")
        if not (bool(torch.isfinite(out).all()) and err <= bound):
            failed.append((name, err, e32, bound))
    assert not failed, (what, failed)
    return ratios


# ---- (a) exact cases --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 9])
def test_constant_channels_are_exact(gpu_required, batch):
    """x[b, c] = c + 1: save_mean is c + 1 and y is act(beta_c (+ r)) bit for bit; with dy = 1 and slope 1, dbeta_c counts
    every one of the batch * 4096 terms once."""
    gen = torch.Generator().manual_seed(batch)
    x = (torch.arange(16, dtype=torch.float32) + 1).reshape(1, 16, 1, 1).expand(batch, 16, D, D).contiguous()
    gamma, beta = torch.rand(16, generator=gen) + 0.5, torch.randn(16, generator=gen)
    res = torch.randn(batch, 16, D, D, generator=gen)
    ones = torch.ones(batch, 16, D, D)
    for slope in (0.0, 0.01, 1.0):
        for r in (None, res):
            case = Case(x, gamma, beta, r, ones, slope)
            got = hip_outputs(case)
            assert torch.equal(got["save_mean"].cpu(), torch.arange(16, dtype=torch.float32) + 1), (slope, r is not None)
            z = beta.reshape(1, 16, 1, 1).expand(batch, 16, D, D)
            z = z if r is None else z + r
            want = torch.where(z > 0, z, z * torch.tensor(case.slope, dtype=torch.float32))
            assert torch.equal(got["y"].cpu(), want), (slope, r is not None)
            # variance exactly 0: invstd = 1 / sqrt(eps) to fp32 rounding of a float64 result
            assert torch.equal(got["save_invstd"].cpu(), torch.full((16,), 1.0 / np.sqrt(np.float64(np.float32(EPS)))).float())
            if slope == 1.0:
                assert torch.equal(got["dbeta"].cpu(), torch.full((16,), float(batch * D * D))), (slope, r is not None)
                assert torch.equal(got["dgamma"].cpu(), torch.zeros(16))
                if r is not None:
                    assert torch.equal(got["dresidual"].cpu(), ones)


# ---- (b) impulses -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1, 2])
def test_impulses_at_every_split_of_the_work(gpu_required, shift):
    """One non-zero element per channel, in x and then in dy, at the first and last element of a plane, in the first, a middle
    and the last image and on both sides of every place where a channel's work is split (POSITIONS); the three shifts put
    every position into every one of the three images."""
    batch = 9
    base = random_case(batch, 0.0, True, 40 + shift)
    imp = torch.zeros(batch, 16, D, D)
    for c in range(16):
        pos, img = POSITIONS[c % 8], IMAGES[(c + shift) % 3]
        imp[img, c].view(-1)[pos] = 1.5 + c
    assert int((imp != 0).sum()) == 16
    for slope, with_res in ((0.0, True), (0.01, False)):
        res = base.residual if with_res else None
        check_case(Case(imp, base.gamma, base.beta, res, base.dy, slope), f"impulse in x, shift {shift} slope {slope}")
        check_case(Case(base.x, base.gamma, base.beta, res, imp, slope), f"impulse in dy, shift {shift} slope {slope}")
    # slope 1, dy the impulse: dbeta is the impulse's value and dresidual the impulse itself, exactly
    got = hip_outputs(Case(base.x, base.gamma, base.beta, base.residual, imp, 1.0))
    assert torch.equal(got["dbeta"].cpu(), torch.arange(16, dtype=torch.float32) + 1.5)
    assert torch.equal(got["dresidual"].cpu(), imp)


# ---- (c) random cases -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_residual", [False, True])
@pytest.mark.parametrize("slope", [0.0, 0.01, 1.0])
@pytest.mark.parametrize("batch", [1, 3, 9])
def test_random_against_float64(gpu_required, batch, slope, with_residual):
    """x = randn, gamma in [0.5, 1.5), beta = randn, r = randn, dy = randn.  Every run prints the kernel-to-e32 ratios (the
    bound is 4); the measured ranges are in DESIGN.md 4.9."""
    check_case(random_case(batch, slope, with_residual, 1000 * batch + int(100 * slope) + with_residual),
               f"B={batch} slope={slope} res={int(with_residual)}")


def test_random_mean_large_against_spread(gpu_required):
    """Channels of mean 100 and standard deviation 0.01: E[x^2] - E[x]^2 in fp32 has no correct digit here."""
    case = random_case(9, 0.0, True, 71, mean=100.0, std=0.01)
    ratios = check_case(case, "mean 100 std 0.01")
    got = hip_outputs(case)
    var = case.x.double().var(dim=(0, 2, 3), unbiased=False)
    assert float(((1.0 / got["save_invstd"].double().cpu() ** 2 - case.eps) / var - 1).abs().max()) < 1e-3, ratios


def test_random_with_a_constant_channel(gpu_required):
    case = random_case(9, 0.01, True, 72)
    case.x[:, 7] = case.x[0, 7, 0, 0]
    check_case(case, "channel 7 constant")
    got = hip_outputs(case)
    assert float(got["save_mean"][7]) == float(case.x[0, 7, 0, 0]) and float(got["dgamma"][7]) == 0.0


def test_random_more_planes_than_lanes(gpu_required):
    """B = 70: a wavefront's sweep over a channel's per-plane partial sums takes a second round (lanes 0 .. 5)."""
    check_case(random_case(70, 0.0, True, 73), "B=70")


# ---- (d) repeatability, operand forms ---------------------------------------------------------------------------------
def test_three_calls_give_identical_bits(gpu_required):
    case = random_case(9, 0.01, True, 81)
    first = hip_outputs(case)
    for _ in range(2):
        again = hip_outputs(case)
        for name in NAMES:
            assert torch.equal(first[name], again[name]), name


def test_function_takes_strided_and_offset_inputs(gpu_required):
    """Channels-last, a strided view and a view 4 bytes off a 16-byte boundary (inputs, parameters and running buffers) give
    the bits of the contiguous tensors."""
    fn = _fn()
    case = random_case(2, 0.0, True, 82)
    x, res, dy, gamma, beta = (t.to(DEV) for t in (case.x, case.residual, case.dy, case.gamma, case.beta))

    def run(xi, ri, gi, wi, bi, rm, rv):
        xi, ri = xi.detach().requires_grad_(True), ri.detach().requires_grad_(True)
        wi, bi = wi.detach().requires_grad_(True), bi.detach().requires_grad_(True)
        y = fn.apply(xi, wi, bi, ri, rm, rv, MOMENTUM, EPS, 0.0)
        y.backward(gi)
        return y.detach(), xi.grad, ri.grad, wi.grad, bi.grad, rm.clone(), rv.clone()

    def buffers():
        return case.running_mean.to(DEV).clone(), case.running_var.to(DEV).clone()

    def off(t):
        o = torch.empty(t.numel() + 1, device=DEV)[1:].view(t.shape).copy_(t)
        assert o.data_ptr() % 16 == 4
        return o

    def wide(t):
        w = torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), device=DEV)
        w[..., ::2] = t
        return w[..., ::2]

    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    want = run(x, res, dy, gamma, beta, *buffers())
    assert not torch.equal(want[5], case.running_mean.to(DEV)) and not torch.equal(want[6], case.running_var.to(DEV))
    before = (fn.n_forward, fn.n_backward)
    for form in (cl, off, wide):
        rm, rv = buffers()
        got = run(form(x), form(res), form(dy), gamma, beta, rm, rv)
        for a, b in zip(got, want):
            assert torch.equal(a, b), form
    rm, rv = buffers()
    got = run(x, res, dy, off(gamma), wide(beta), off(rm), wide(rv))   # the buffers get their update back through the copies
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert (fn.n_forward, fn.n_backward) == (before[0] + 4, before[1] + 4)
    # without running buffers nothing is updated and y is the same; other shapes are refused
    y = fn.apply(x, gamma, beta, res, None, None, MOMENTUM, EPS, 0.0)
    assert torch.equal(y, want[0])
    with pytest.raises(ValueError):
        fn.apply(x[:, :, :32, :32], gamma, beta, None, None, None, MOMENTUM, EPS, 0.0)
    with pytest.raises(ValueError):
        fn.apply(x, gamma, beta, None, rm, None, MOMENTUM, EPS, 0.0)


# ---- (e) / (f) a real network -----------------------------------------------------------------------------------------
def _net(seed):
    from flingbot_amd import nets

    torch.manual_seed(seed)
    net = nets.SpatialValueNet(rgb_only=True, device=DEV).to(DEV)
    return ref.randomise_bn(net, seed)


def _batch(batch, seed):
    rng = np.random.default_rng(seed)
    obs = ref.make_obs(batch, seed, channels=3)
    mask = torch.zeros(batch, D, D, dtype=torch.bool)
    for k in range(batch):
        mask[k, int(rng.integers(8, 56)), int(rng.integers(8, 56))] = True
    label = torch.from_numpy(rng.uniform(-0.1, 0.2, batch).astype(np.float32))
    return obs, mask, label


def _loss(out, mask, label):
    return F.mse_loss(torch.masked_select(out.squeeze(1), mask), label)


class _switches:
    def __init__(self, conv, bn):
        self.want = (conv, bn)

    def __enter__(self):
        from flingbot_amd import nets
        self.saved = (nets._TRAIN_CONV_HIP, nets._TRAIN_BN_HIP)
        nets._TRAIN_CONV_HIP, nets._TRAIN_BN_HIP = self.want

    def __exit__(self, *exc):
        from flingbot_amd import nets
        nets._TRAIN_CONV_HIP, nets._TRAIN_BN_HIP = self.saved


def _sites(net):
    """(BatchNorm module, slope, has a residual) of the 17 sites in the order of the forward."""
    blocks = list(net.net)
    first = blocks[0].net
    sites = [(first[1], first[2].negative_slope, False)]
    for blk in blocks[1:-1]:
        sites += [(blk.bn1, 0.0, False), (blk.bn2, 0.0, True)]
    assert len(sites) == 17
    return sites


def test_per_site_replay_on_a_real_network(gpu_required):
    """x, residual and output gradient of all 17 BatchNorm sites, recorded from one stock train-mode step (B = 9, both switches
    off), through the kernels: every site meets the bound of the random cases."""
    net = _net(11).train()
    obs, mask, label = (t.to(DEV) for t in _batch(9, 11))
    blocks = list(net.net)
    seen, hooks = {}, []

    def keep_grad(key):
        return lambda grad: seen.__setitem__(key, grad.detach().clone().cpu())

    def on_bn(k):
        def record(module, inputs):
            seen[("x", k)] = inputs[0].detach().clone().cpu()
            seen[("rm", k)], seen[("rv", k)] = module.running_mean.detach().clone().cpu(), module.running_var.detach().clone().cpu()
        return record

    # site 0: the first block's output; site 2 j + 1: the input of conv2 of residual block j; site 2 j + 2: that block's output
    def first_done(module, inputs, out):          # (hooks return nothing: a returned value would replace the tensor)
        out.register_hook(keep_grad(("g", 0)))

    hooks.append(blocks[0].net[1].register_forward_pre_hook(on_bn(0)))
    hooks.append(blocks[0].register_forward_hook(first_done))
    for j, blk in enumerate(blocks[1:-1]):
        hooks.append(blk.bn1.register_forward_pre_hook(on_bn(2 * j + 1)))
        hooks.append(blk.bn2.register_forward_pre_hook(on_bn(2 * j + 2)))

        def before_conv2(module, inputs, k=2 * j + 1):
            inputs[0].register_hook(keep_grad(("g", k)))

        def block_done(module, inputs, out, k=2 * j + 2):
            seen[("r", k)] = inputs[0].detach().clone().cpu()
            out.register_hook(keep_grad(("g", k)))

        hooks.append(blk.conv2.register_forward_pre_hook(before_conv2))
        hooks.append(blk.register_forward_hook(block_done))
    try:
        with _switches(False, False):
            _loss(net(obs), mask, label).backward()
    finally:
        for h in hooks:
            h.remove()
    for k, (bn, slope, with_res) in enumerate(_sites(net)):
        x, g = seen[("x", k)], seen[("g", k)]
        assert tuple(x.shape) == tuple(g.shape) == (9, 16, D, D) and float(g.abs().max()) > 0 and (("r", k) in seen) == with_res
        case = Case(x, bn.weight.detach().cpu(), bn.bias.detach().cpu(), seen.get(("r", k)), g, slope, seen[("rm", k)], seen[("rv", k)],
                    eps=bn.eps, momentum=bn.momentum)
        check_case(case, f"site {k:2d}")


def test_whole_network_forward_and_wiring(gpu_required):
    from flingbot_amd import nets

    net = _net(21)
    obs, mask, label = _batch(9, 21)
    running_keys = [k for k in net.state_dict() if "running_" in k]
    tracked_keys = [k for k in net.state_dict() if k.endswith("num_batches_tracked")]
    assert len(running_keys) == 34 and len(tracked_keys) == 17
    before = {k: v.clone() for k, v in net.state_dict().items()}

    f64 = copy.deepcopy(net).cpu().double().train()
    with torch.no_grad():
        want = f64(obs.double())
    host = copy.deepcopy(net).cpu().train()
    with torch.no_grad():
        out_host = host(obs)
    stock = copy.deepcopy(net).train()
    with _switches(False, False):
        out_stock = stock(obs.to(DEV))
        _loss(out_stock, mask.to(DEV), label.to(DEV)).backward()
    e32 = max(float((out_host.double() - want).abs().max()), float((out_stock.detach().double().cpu() - want).abs().max()))

    bn, conv = nets.BatchNormAct16Function, nets.Conv16Function
    calls = (bn.n_forward, bn.n_backward, conv.n_forward, conv.n_backward)
    net.train()
    with _switches(True, True):
        out = net(obs.to(DEV))
        assert (bn.n_forward - calls[0], bn.n_backward - calls[1], conv.n_forward - calls[2], conv.n_backward - calls[3]) == (17, 0, 16, 0)
        err = float((out.detach().double().cpu() - want).abs().max())
        bound = ref.tolerance(e32, want)
        print(f"whole network: err {err:.3e}  e32 {e32:.3e}  ratio {err / e32:.2f}  bound {bound:.3e}")
        assert bool(torch.isfinite(out).all()) and err <= bound
        _loss(out, mask.to(DEV), label.to(DEV)).backward()
    assert (bn.n_forward - calls[0], bn.n_backward - calls[1], conv.n_forward - calls[2], conv.n_backward - calls[3]) == (17, 17, 16, 16)

    after, f64_state, host_state, stock_state = net.state_dict(), f64.state_dict(), host.state_dict(), stock.state_dict()
    assert list(after) == list(before)
    for k in tracked_keys:
        assert int(after[k]) == int(before[k]) + 1 == int(stock_state[k]), k
    worst = 0.0
    for k in running_keys:
        assert not torch.equal(after[k], before[k]), k
        w = f64_state[k]
        e = max(float((host_state[k].double() - w).abs().max()), float((stock_state[k].double().cpu() - w).abs().max()))
        err_k = float((after[k].double().cpu() - w).abs().max())
        worst = max(worst, err_k / e if e > 0 else 0.0)
        assert err_k <= ref.tolerance(e, w), (k, err_k, e)
    print(f"running buffers: worst error / e32 {worst:.2f}")

    with_grad, dists = 0, []
    for (name, p), (_, q) in zip(net.named_parameters(), stock.named_parameters()):
        if q.grad is None:
            assert p.grad is None, name
            continue
        with_grad += 1
        assert p.grad is not None and p.grad.shape == q.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), name
        dist = float((p.grad.double() - q.grad.double()).norm() / q.grad.double().norm())
        dists.append(dist)
        print(f"gradient of {name}: relative L2 distance to the stock path {dist:.3e}")
        assert dist <= 1e-2, (name, dist)
    assert with_grad == 2 + 16 + 2 * 17          # 18 convolutions, 17 BatchNorms (weight and bias)
    print(f"gradients: largest relative L2 distance {max(dists):.3e}")


# ---- (g) learning -----------------------------------------------------------------------------------------------------
def test_optimize_learns_a_fixed_set_twice_the_same(gpu_required):
    """The recipe of test_vntrain_gpu.test_optimize_learns_a_fixed_set with the BatchNorm switch on, inside
    train.deterministic_library_convs() as train.run runs its updates: the loss falls below half, every update goes through
    the kernels, and a second run from the same seed ends with the same bits in every entry of the state_dict."""
    import test_vntrain_gpu as vt
    from flingbot_amd import nets, train

    def one_run():
        torch.manual_seed(0)
        net = nets.SpatialValueNet(rgb_only=True, device=DEV).to(DEV)
        opt = torch.optim.Adam(net.parameters(), lr=1e-3, weight_decay=1e-6)
        data = vt.learning_set().to_device(DEV)
        before = nets.BatchNormAct16Function.n_backward
        net.train()
        with _switches(True, True), train.deterministic_library_convs():
            losses = train.optimize("fling", net, opt, data, vt.LEARN_UPDATES, 8, np.random.default_rng(0))
        net.eval()
        assert nets.BatchNormAct16Function.n_backward - before == 17 * vt.LEARN_UPDATES
        return losses, {k: v.clone() for k, v in net.state_dict().items()}

    losses, state = one_run()
    print(f"loss {losses[0]:.4e} -> {losses[-1]:.4e} in {len(losses)} updates")
    assert len(losses) == vt.LEARN_UPDATES and all(np.isfinite(losses)) and int(state["steps"]) == vt.LEARN_UPDATES
    assert losses[-1] < 0.5 * losses[0]
    losses_again, state_again = one_run()
    assert losses_again == losses and list(state_again) == list(state)
    for k in state:
        assert torch.equal(state[k], state_again[k]), k
