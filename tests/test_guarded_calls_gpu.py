"""Every device entry point of libflingsim behind guard bands and poisoned scratch (tests/guarded_calls.py).

Each case runs the public wrapper three times on identical inputs -- plainly, then under the interposer with poison A (0xFF) and
with poison B (a seeded byte stream) -- and asserts: (a) every guard byte around every device argument is intact, (b) every
const argument is bit-identical after the call (both inside the interposer, per call), (c) every result -- device outputs, host
outputs, returned values -- is bit-identical across the three runs and no output byte kept both poisons, (d) the entry points
the case names were reached through the interposer.  A work slot is exactly as long as the matching *_work_bytes function says
for the call's own dimensions.  The reference of (c) is the plain wrapper path, which the other suites pin to float64 or to the
oracle; bit equality needs no tolerance.  The last test of the module asserts that the cases before it reached all 27 stream
entry points and the three fs_observe* entry points (run the module as a whole)."""
import ctypes as C

import numpy as np
import pytest
import torch

import guarded_calls as gc
from conftest import cloth_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REACHED = set()


# ---- the three runs ------------------------------------------------------------------------------------------------------------
def _freeze(x, out, path="result"):
    """Flatten a result into [(path, bytes-comparable numpy array or plain value)]."""
    if torch.is_tensor(x):
        out.append((path, gc.byte_view(x.detach().contiguous()).cpu().numpy().copy()))
    elif isinstance(x, np.ndarray):
        out.append((path, np.ascontiguousarray(x).view(np.uint8).copy()))
    elif isinstance(x, dict):
        for k in sorted(x):
            _freeze(x[k], out, f"{path}[{k!r}]")
    elif isinstance(x, (list, tuple)):
        for k, v in enumerate(x):
            _freeze(v, out, f"{path}[{k}]")
    elif isinstance(x, float):
        out.append((path, np.float64(x).tobytes()))
    else:
        out.append((path, x))
    return out


def _same(tag, a, b):
    assert [p for p, _ in a] == [p for p, _ in b], tag
    for (path, x), (_, y) in zip(a, b):
        if isinstance(x, np.ndarray):
            assert x.shape == y.shape, (tag, path)
            bad = np.flatnonzero(x != y)
            assert bad.size == 0, f"{tag}: {path} differs in {bad.size} bytes, first at byte {int(bad[0])}"
        else:
            assert x == y, (tag, path, x, y)


def _clear_scratch():
    from flingbot_amd import action

    action._work.clear()


def three_runs(fn, must_hit):
    """fn() -> result, from fresh outputs each time.  Returns the plain result."""
    _clear_scratch()
    plain = fn()
    want = _freeze(plain, [])
    runs = []
    for poison in gc.POISONS:
        _clear_scratch()
        with gc.interposed(poison) as guard:
            got = _freeze(fn(), [])
        missing = [name for name in must_hit if not guard.counts.get(name)]
        assert not missing, f"not reached through the interposer: {missing} (reached {guard.counts})"
        REACHED.update(guard.counts)
        runs.append((guard, got))
    gc.assert_outputs_written(runs[0][0], runs[1][0])
    _same("plain run against poison A", want, runs[0][1])
    _same("poison A against poison B", runs[0][1], runs[1][1])
    return plain


def _randn(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


# ---- observation transforms and action selection ------------------------------------------------------------------------------
@pytest.mark.parametrize("channels,S,dim,T", [(4, 5, 7, 1), (3, 40, 16, 5)])
def test_prepare_image(gpu_required, channels, S, dim, T):
    import test_prepare_image_gpu as tp
    from flingbot_amd import nets

    img = torch.tensor(tp._test_image(channels, S, seed=10 * S + channels)).to(DEV)
    tf = [(tp.ROTATIONS[4], 1.5)] if T == 1 else [(-90.0, 1.0), (tp.ROTATIONS[6], 0.75), (37.0, 1.5), (90.0, 2.75),
                                                  (tp.ROTATIONS[4], 1.05)]
    assert len(tf) == T
    out = three_runs(lambda: nets.prepare_image_device(img, tf, dim), ["fs_prepare_image"])
    assert tuple(out.shape) == (T, channels, dim, dim)


def test_select_action_and_transform_winners(gpu_required):
    import test_transform_winners_gpu as tw

    sel = tw._selector()
    values, depth = tw.make_case()
    d_values, d_depth = torch.tensor(values).to(DEV), torch.tensor(depth).to(DEV)
    action, params = three_runs(lambda: sel.select(d_values[0], tw.SCALES[0], depth[0]), ["fs_select_action"])
    assert action in tw.PRIMS and params["flat_index"] >= 0
    index, value = three_runs(lambda: sel.winners(d_values, tw.SCALES, d_depth), ["fs_transform_winners"])
    assert index.shape == (tw.N, len(tw.PRIMS), tw.T) and (index >= 0).any() and (index < 0).any()


@pytest.mark.parametrize("radius", [0, 3])
def test_lattice_actions(gpu_required, radius):
    import test_probe_gpu as tp

    sel = tp._selector()
    values, depth = tp.make_lattice_case()
    requests = tp.lattice_requests()
    cells = {r[6] * r[7] for r in requests}
    assert len(cells) > 1 and min(cells) < max(cells)          # rows shorter than the pitch
    d_values, d_depth = torch.tensor(values).to(DEV), torch.tensor(depth).to(DEV)
    valid, on1, on2, value = three_runs(lambda: sel.lattice(d_values, tp.SCALES, d_depth, requests, radius), ["fs_lattice_actions"])
    assert valid.any() and not valid.all()


@pytest.mark.parametrize("first_greedy", [True, False])
def test_sample_actions(gpu_required, first_greedy):
    import sample_cases as sc
    from flingbot_amd import action

    sel = sc.selector()
    values, depth = sc.make_case()
    d_values, d_depth = torch.tensor(values).to(DEV), torch.tensor(depth).to(DEV)
    noise = action.gumbel_table(torch.device(DEV))
    keys = np.stack([sc.key_of(e) for e in range(sc.N)])
    index, value, key, pixels = three_runs(
        lambda: sel.sample(d_values, sc.SCALES, d_depth, 16, keys, 4.0, noise, first_greedy=first_greedy, on_cloth=True, radius=1),
        ["fs_sample_actions"])
    assert index.shape == (sc.N, 16) and (index[:3] >= 0).all() and (index[sc.NONE] == -1).all()


def test_sample_actions_candidate_count_off_the_pad(gpu_required):
    """P = 1, T = 3, D - 2 g = 23: 1587 candidates per observation, padded to 1600."""
    import sample_cases as sc
    from flingbot_amd import action

    sel = action.ActionSelector(["fling"], [-35.0, 0.0, 35.0], 31, 4, sc.DRAG, sc.PLACE, sc.REACH)
    assert 1 * 3 * (31 - 8) ** 2 == 1587 and 1587 % 16 != 0
    g = torch.Generator().manual_seed(23)
    d_values = (torch.round(torch.rand(1, 1, 3, 31, 31, generator=g) * 64) / 64).to(DEV)
    d_depth = torch.tensor(sc.make_case()[1][1:2]).to(DEV)
    noise = action.gumbel_table(torch.device(DEV))
    index, value, key, pixels = three_runs(
        lambda: sel.sample(d_values, [np.array([1.0])], d_depth, 16, sc.key_of(0)[None], 4.0, noise, first_greedy=True,
                           on_cloth=True, radius=1), ["fs_sample_actions"])
    assert (index >= 0).any()


# ---- the value net and its training kernels -------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("kind", ["rgb", "depth", "rgbd"])
def test_value_net_forward(gpu_required, kind, batch):
    import test_valuenet_gpu as tv
    from flingbot_amd import nets

    torch.manual_seed(3)
    net = nets.SpatialValueNet(rgb_only=kind == "rgb", depth_only=kind == "depth", device=torch.device(DEV))
    tv._randomise_bn(net, 4)
    net = net.to(DEV).eval()
    net.fold_batchnorm()
    assert net._hip is not None
    obs = tv._obs(batch, 5).to(DEV)

    def run():
        with torch.no_grad():
            return net(obs)

    assert tuple(three_runs(run, ["fs_value_net_forward"]).shape) == (batch, 1, 64, 64)


@pytest.mark.parametrize("batch", [1, 9])
def test_conv16(gpu_required, batch):
    from flingbot_amd.trainops import Conv16Function as F

    x, g, w = _randn(batch, 16, 64, 64, seed=1), _randn(batch, 16, 64, 64, seed=2), _randn(16, 16, 3, 3, seed=3, scale=0.1)
    three_runs(lambda: (F._conv(x, w, 0), F._conv(g, w, 1), F._wgrad(x, g)), ["fs_conv16_forward", "fs_conv16_wgrad"])


@pytest.mark.parametrize("batch", [1, 9])
def test_bn16(gpu_required, batch):
    from flingbot_amd.trainops import BatchNormAct16Function as F

    x, res, dy = _randn(batch, 16, 64, 64, seed=4), _randn(batch, 16, 64, 64, seed=5), _randn(batch, 16, 64, 64, seed=6)
    gamma, beta = _randn(16, seed=7).abs() + 0.5, _randn(16, seed=8, scale=0.1)
    for with_residual in (False, True):
        for with_running in (False, True):
            def forward():
                rm = _randn(16, seed=9, scale=0.2) if with_running else None
                rv = (_randn(16, seed=10).abs() + 0.5) if with_running else None
                return F._forward(x, gamma, beta, res if with_residual else None, rm, rv, 0.1, 1e-5, 0.01), rm, rv

            (y, mean, invstd), rm, rv = three_runs(forward, ["fs_bn16_forward"])
            assert with_running == (rm is not None)
        three_runs(lambda: F._backward(x, y, dy, gamma, mean, invstd, 0.01, with_residual), ["fs_bn16_backward"])


@pytest.mark.parametrize("channels", [1, 3, 4])
def test_convin(gpu_required, channels):
    from flingbot_amd.trainops import ConvInFunction as F

    x, g, w = _randn(3, channels, 64, 64, seed=11), _randn(3, 16, 64, 64, seed=12), _randn(16, channels, 3, 3, seed=13, scale=0.2)
    three_runs(lambda: (F._forward(x, w), F._wgrad(x, g)), ["fs_convin_forward", "fs_convin_wgrad"])


def test_head_at_one_pixel(gpu_required):
    from flingbot_amd.trainops import HeadPixelFunction as F

    h, w, gpred = _randn(7, 16, 64, 64, seed=14), _randn(1, 16, 3, 3, seed=15, scale=0.2), _randn(7, seed=16)
    pix = torch.tensor([0, 63, 4032, 4095, 64 * 31 + 17, 1, 4094], dtype=torch.int32, device=DEV)   # the corners, an edge, inside
    three_runs(lambda: (F._forward(h, w, pix), F._backward(h, w, pix, gpred)), ["fs_head_forward", "fs_head_backward"])


@pytest.mark.parametrize("offsets", [[0, 40, 40, 65], [0, 0, 1, 1]])
def test_head_at_listed_pixels(gpu_required, offsets):
    """65 entries (one past a 64-entry chunk) and 1 entry, over batch 3 with an image that has no pixel."""
    from flingbot_amd.trainops import HeadPixelsFunction as F

    L = offsets[-1]
    h, w, gpred = _randn(3, 16, 64, 64, seed=17), _randn(1, 16, 3, 3, seed=18, scale=0.2), _randn(L, seed=19)
    rng = np.random.default_rng(L)
    pix = np.concatenate([1 + rng.permutation(4094)[:b - a] for a, b in zip(offsets, offsets[1:])]).astype(np.int32)
    pix[0] = 0 if L > 1 else 4095                                      # a corner: the patch is clipped (and no pixel twice)
    d_pix, d_off = torch.from_numpy(pix).to(DEV), torch.tensor(offsets, dtype=torch.int32, device=DEV)
    three_runs(lambda: (F._forward(h, w, d_off, d_pix), F._backward(h, w, d_off, d_pix, gpred)),
               ["fs_head_forward_pixels", "fs_head_backward_pixels"])


def test_adam_step_on_arena_slots(gpu_required):
    """The four arrays of a segment are reachable only through the table, so they are arena slots here: guards between all 28
    arrays, the gradients unchanged, and the same bits as the call on plain tensors."""
    import test_edgetrain_cpu as te
    from flingbot_amd import sim as fsim

    sizes = te.ADAM_SIZES
    params = te.adam_parameters(3, device=DEV)
    grads = te.adam_gradients(sizes, 1, 3, device=DEV)
    moments = [_randn(n, seed=20 + k, scale=0.01) for k, n in enumerate(sizes)]
    seconds = [_randn(n, seed=40 + k, scale=0.01).abs() for k, n in enumerate(sizes)]
    scalars = (1e-3, 0.9, 0.999, 1e-8, 1e-6, 1.0 - 0.9 ** 3, 1.0 - 0.999 ** 3)

    def table_of(pointers):
        table = (fsim.AdamSegment * len(sizes))()
        for seg, n, (p, g, m, v) in zip(table, sizes, pointers):
            seg.param, seg.grad, seg.exp_avg, seg.exp_avg_sq, seg.count = p, g, m, v, n
        return table

    plain = [[t.clone() for t in group] for group in (params, grads, moments, seconds)]
    fsim.stream_call("fs_adam_step", 0, table_of([[t.data_ptr() for t in row] for row in zip(*plain)]), len(sizes), *scalars)
    torch.cuda.synchronize()
    want = _freeze(plain, [])
    assert not torch.equal(plain[0][6], params[6])
    for poison in gc.POISONS:
        slots = []
        for k in range(len(sizes)):
            for j, (group, role) in enumerate(zip((params, grads, moments, seconds), ("inout", "in", "inout", "inout"))):
                slots.append(gc.Slot(4 * k + j, 4 * sizes[k], role, gc.byte_view(group[k])))
        arena = gc.Arena(DEV, slots, poison, "fs_adam_step")
        with gc.interposed(poison) as guard:
            fsim.stream_call("fs_adam_step", 0, table_of([[arena.ptr(4 * k + j) for j in range(4)] for k in range(len(sizes))]),
                             len(sizes), *scalars)
        arena.check()        # the 29 guard bands, and the seven gradient slots against what went in
        assert guard.counts == {"fs_adam_step": 1}
        REACHED.update(guard.counts)
        got = [[arena.typed(4 * k + j, torch.float32).clone() for k in range(len(sizes))] for j in range(4)]
        _same(f"plain tensors against arena slots, poison {poison}", want, _freeze(got, []))


# ---- replay and the losses ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["rgb_jitter", "four_channel"])
def test_replay_sample(gpu_required, tmp_path, mode):
    import test_replay_gpu as tr
    from flingbot_amd import replay

    rng = np.random.default_rng(107)
    path = str(tmp_path / "set.npz")
    tr._write_set(path, tr._observations(rng, 37), rng)
    data = replay.ExperienceSet(path, **(dict() if mode == "rgb_jitter" else dict(rgb_only=False))).to_device(DEV)
    assert len(data) == 37 and data.jitters == (mode == "rgb_jitter")
    obs, mask, label = three_runs(lambda: data.sample(7, np.random.default_rng(1)), ["fs_replay_sample"])
    assert tuple(obs.shape) == (7, 3 if mode == "rgb_jitter" else 4, 64, 64) and (mask.sum(dim=(1, 2)) == 1).all()


def test_group_loss(gpu_required):
    from flingbot_amd.trainops import GroupLossFunction as F

    pred, label = _randn(7, seed=60), (torch.round(_randn(7, seed=61) * 4) / 4)
    bounds = torch.tensor([[0, 1], [1, 3], [1, 3], [3, 7], [3, 7], [3, 7], [3, 7]], dtype=torch.int32, device=DEV)   # groups of 1, 2, 4
    dpred, stats = three_runs(lambda: F._launch(pred, label, bounds, 0.5, 0.1, 0.0), ["fs_group_loss"])
    assert float(stats[3]) >= 1


OFFSETS = [0, 1, 3, 260, 260, 4360]      # images of 1 (not listed), 2, 257, 0 and 4100 labels (served: the first 4096)
OWNED = 260 + 4096                       # d_dpred entries 4356 .. 4359 belong to no clamped image: documented as not written


def _map_inputs():
    L = OFFSETS[-1]
    pred, label = _randn(L, seed=62), torch.round(_randn(L, seed=63) * 4) / 4
    return pred, label, torch.tensor(OFFSETS, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("per_image", [False, True])
def test_map_loss_and_map_list_loss(gpu_required, per_image):
    from flingbot_amd.trainops import MapListFunction, MapLossFunction

    pred, label, offsets = _map_inputs()

    def pairwise():
        dpred, stats, table = MapLossFunction._launch(pred, label, offsets, 0.5, 0.1, 0.0, per_image)
        return dpred[:OWNED], stats, table

    def listwise():
        dpred, stats, table = MapListFunction._launch(pred, label, offsets, 0.5, 0.3, 0.2, per_image)
        return dpred[:OWNED], stats, table

    dpred, stats, table = three_runs(pairwise, ["fs_map_loss"])
    assert float(stats[3]) > 0 and float(stats[5]) == 4
    dpred, stats, table = three_runs(listwise, ["fs_map_list_loss"])
    assert float(stats[2]) == 3 and float(stats[3]) == 2 + 257 + 4096 and table[0].tolist() == [0.0, 0.0, -1.0, -1.0]


@pytest.mark.parametrize("n_temperatures", [1, 33])
@pytest.mark.parametrize("per_image", [False, True])
def test_map_list_sweep(gpu_required, per_image, n_temperatures):
    from flingbot_amd.trainops import MapListSweep

    pred, label, offsets = _map_inputs()
    temperatures = np.ascontiguousarray(np.geomspace(0.02, 20.0, n_temperatures))
    curve, rows, images = three_runs(lambda: MapListSweep._launch(pred, label, offsets, temperatures, 0.2, per_image),
                                     ["fs_map_list_sweep"])
    assert tuple(curve.shape) == (n_temperatures, 8) and float(curve[0, 6]) == 3 and images[3].tolist() == [0.0] * 4


def test_map_score(gpu_required):
    from flingbot_amd import trainops

    _, label, offsets = _map_inputs()
    L, images = OFFSETS[-1], len(OFFSETS) - 1
    value = _randn(images, 4096, seed=64)
    rng = np.random.default_rng(65)
    pix = torch.from_numpy(rng.integers(0, 4096, L).astype(np.int32)).to(DEV)

    def run():
        rows = torch.empty((images, 12), dtype=torch.float64, device=DEV)
        trainops.stream_call("fs_map_score", value.device, value, 4096, pix, label, offsets, images, L, 0.0, rows)
        return rows

    rows = three_runs(run, ["fs_map_score"])
    assert rows[:, 0].tolist() == [1.0, 2.0, 257.0, 0.0, 4096.0]


# ---- the report's kernels -------------------------------------------------------------------------------------------------------
def test_value_range(gpu_required):
    from flingbot_amd import report

    items = [_randn(1, seed=66), _randn(255, seed=67), _randn(4097, seed=68)]
    items[1][100] = float("nan")
    got = three_runs(lambda: report.value_range(items), ["fs_value_range"])
    assert tuple(got.shape) == (3, 2) and bool(torch.isfinite(got).all())


def test_action_lane_and_probe_panels(gpu_required):
    import test_lane_panels_gpu as tl
    import test_probe_gpu as tp
    import test_report_gpu as tr
    from flingbot_amd import report

    actions = [tr._to_device(it) for it in tr._items(8, 50, seed=8050)]
    got = three_runs(lambda: report.compose(actions, panel=40), ["fs_action_panels"])
    assert got.shape == (3, 40, 200, 3) and got.any()
    lanes = [tl._item(r) for r in tl._records(33, 3, 5, seed=3305)]
    got = three_runs(lambda: report.compose_lanes(lanes, 3, panel=40), ["fs_lane_panels"])
    assert got.shape == (5, 40, 160, 3) and got.any()
    probed = [tp._probe_item(r) for r in tp._probe_records(seed=40)]
    got = three_runs(lambda: report.compose_probe(probed, panel=40), ["fs_probe_panels"])
    assert got.shape == (4, 40, 160, 3) and got.any()


# ---- the observation stage: context calls, driven on an arena -----------------------------------------------------------------------
S_OBS = 77


@pytest.fixture(scope="module")
def scenes(gpu_required):
    """Three small cloths rendered at 300 x 300, and two synthetic frames of different sizes."""
    import test_observe_frames_gpu as tf
    from flingbot_amd import sim as fsim

    ctx = fsim.FlingSim(n_envs=3, solver=0)
    for e, dims in enumerate([(20, 15), (30, 12), (12, 28)]):
        env = ctx.env(e)
        env.set_scene(cloth_params(dims[0], dims[1], pos=(0.05 * e, 0.3, -0.04 * e)))
        rng = np.random.RandomState(e)
        p = env.get_positions().reshape(-1, 4)
        p[:, :3] += rng.randn(*p[:, :3].shape).astype(np.float32) * 0.004
        env.set_positions(p.ravel())
    ctx.step(2)
    for e in range(3):
        cp = ctx.get_camera_params(e)
        ctx.set_camera_params(e, [*cp[2:8], 300, 300])
    rng = np.random.RandomState(9)
    frames = [tf._noise_frame(rng, 120, 91), tf._frame_of_mask(tf._serpentine(61), rng, size=(150, 180))]
    rgba = [torch.from_numpy(np.array(c, np.uint8, order="C")).to(DEV) for c, _ in frames]
    depth = [torch.from_numpy(np.array(d, np.float32, order="C")).to(DEV) for _, d in frames]
    yield ctx, rgba, depth
    ctx.close()


def _observe_on_arena(ctx, entry, first_arg, n, with_mask, poison, call):
    """One fs_observe* call with d_obs, d_mask and d_work in arena slots; the work slot is exactly n * fs_observe_work_bytes(S).
    call(d_obs, d_mask, bbox, d_work) -> return code.  Returns (results, arena, still-poisoned masks of the outputs)."""
    S = S_OBS
    slots = [gc.Slot(first_arg, n * 4 * S * S * 4, "out")]
    if with_mask:
        slots.append(gc.Slot(first_arg + 1, n * S * S, "out"))
    slots.append(gc.Slot(first_arg + 3, n * int(ctx.lib.fs_observe_work_bytes(S)), "work"))
    arena = gc.Arena(DEV, slots, poison, entry)
    bbox = np.zeros((n, 5), np.int32)
    torch.cuda.synchronize()
    rc = call(C.c_void_p(arena.ptr(0)), C.c_void_p(arena.ptr(1)) if with_mask else None,
              bbox.ctypes.data_as(C.POINTER(C.c_int)), C.c_void_p(arena.ptr(len(slots) - 1)))
    assert rc == 0, ctx.lib.fs_last_error().decode()
    arena.check()
    work = arena.view(len(slots) - 1)
    labels = work[:4 * n * S * S].view(torch.int32).view(n, S, S).clone()   # documented: the final labels
    results = dict(obs=arena.typed(0, torch.float32, (n, 4, S, S)).clone(), bbox=bbox, labels=labels,
                   mask=arena.typed(1, torch.uint8, (n, S, S)).clone() if with_mask else None)
    still = {k: arena.still_poisoned(k) for k, s in enumerate(slots) if s.role == "out"}
    return results, arena, still


def _observe_case(ctx, entry, first_arg, n, wrapper, call):
    for with_mask in (True, False):
        ctx._observe_work = None
        out = wrapper(with_mask)
        want = dict(obs=out[0].reshape(n, 4, S_OBS, S_OBS), bbox=np.asarray(out[1]).reshape(n, 5),
                    labels=ctx.observe_labels(n, S_OBS), mask=out[2].reshape(n, S_OBS, S_OBS) if with_mask else None)
        assert (want["bbox"][:, 4] > 0).all(), "every observation shows a component"
        runs = [_observe_on_arena(ctx, entry, first_arg, n, with_mask, poison, call) for poison in gc.POISONS]
        gc.unwritten(entry, runs[0][1].slots, runs[0][2], runs[1][2])
        _same(f"{entry}: wrapper against arena, poison A", _freeze(want, []), _freeze(runs[0][0], []))
        _same(f"{entry}: poison A against poison B", _freeze(runs[0][0], []), _freeze(runs[1][0], []))
    REACHED.add(entry)


def test_observe(scenes):
    ctx = scenes[0]
    for env in range(3):
        _observe_case(ctx, "fs_observe", 3, 1, lambda m: ctx.observe(env, S_OBS, want_mask=m),
                      lambda obs, mask, bbox, work: ctx.lib.fs_observe(ctx.h, env, S_OBS, obs, mask, bbox, work))


def test_observe_batch(scenes):
    ctx = scenes[0]
    envs = np.array([2, 0, 1], np.int32)
    _observe_case(ctx, "fs_observe_batch", 4, 3, lambda m: ctx.observe_batch(envs, S_OBS, want_mask=m),
                  lambda obs, mask, bbox, work: ctx.lib.fs_observe_batch(ctx.h, 3, envs.ctypes.data_as(C.POINTER(C.c_int)), S_OBS,
                                                                         obs, mask, bbox, work))


def test_observe_frames(scenes):
    ctx, rgba, depth = scenes
    ptr_c, ptr_d = (C.c_void_p * 2)(*[t.data_ptr() for t in rgba]), (C.c_void_p * 2)(*[t.data_ptr() for t in depth])
    widths, heights = (C.c_int * 2)(*[t.shape[1] for t in rgba]), (C.c_int * 2)(*[t.shape[0] for t in rgba])
    _observe_case(ctx, "fs_observe_frames", 7, 2, lambda m: ctx.observe_frames(rgba, depth, S_OBS, want_mask=m),
                  lambda obs, mask, bbox, work: ctx.lib.fs_observe_frames(ctx.h, 2, ptr_c, ptr_d, widths, heights, S_OBS, obs, mask,
                                                                          bbox, work))


# ---- (d) for the suite as a whole ------------------------------------------------------------------------------------------------
def test_every_entry_point_was_reached(gpu_required):
    """Runs last: the cases above, together, went through every entry of the role table and the three fs_observe* calls."""
    entries, _ = gc.parse_header()
    assert set(entries) == set(gc.ROLES)
    want = set(gc.ROLES) | set(gc.OBSERVE_ENTRIES)
    assert len(want) == 30
    assert REACHED == want, (sorted(want - REACHED), sorted(REACHED - want))
