"""fs_map_list_sweep (csrc/fs_mapsweep.hip) on the GPU: all three outputs against trainops.map_list_sweep_torch in float64 on the
host, column 0 against fs_map_list_loss at every temperature, place independence, isolation of non-finite images,
trainops.fit_temperature on device tensors against the host path, and score_maps / fit_maps end to end.

The bound against the float64 statement is 1e-9 of the value plus 1e-12: the kernel works in double, a 4096-term sum is wrong by
about 4096 * 2^-53 = 5e-13, three orders below the bound, and anything formed through a float32 intermediate would be off by 6e-8,
two orders above it."""
import numpy as np
import pytest
import torch

import mapsweep_reference as sref
from test_maplist_cpu import values
from test_mapsweep_cpu import tiny_files

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = (False, True)
TY = 0.1
EDGES = [1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096]      # the edges of a wave, of the block and of the 16 register slots
STEPS = [257, 512, 513, 1024, 1025, 2048, 2049, 3000]      # where the kernel passes from 1 to 2, 4, 8 and 16 slots per thread
BATCHES = {"edges": EDGES, "steps": STEPS}
_refs = {}


def grid(S):
    return np.array([0.1]) if S == 1 else np.exp(np.linspace(np.log(1e-4), np.log(1e4), S))


def reference(batch, S, per_image):
    """map_list_sweep_torch in float64 on the host, computed once per case."""
    key = (batch, S, per_image)
    if key not in _refs:
        from flingbot_amd import trainops

        pred, label, offsets = values(BATCHES[batch], "replay")
        out = trainops.map_list_sweep_torch(torch.tensor(pred.astype(np.float64)), torch.tensor(label.astype(np.float64)), offsets, grid(S),
                                            TY, per_image)
        _refs[key] = tuple(t.numpy() for t in out)
    return _refs[key]


def _launch(pred, label, offsets, temperatures, per_image, ty=TY):
    from flingbot_amd import trainops

    p = torch.from_numpy(np.ascontiguousarray(pred, np.float32)).to(DEV)
    y = torch.from_numpy(np.ascontiguousarray(label, np.float32)).to(DEV)
    off = torch.from_numpy(np.ascontiguousarray(offsets, np.int32)).to(DEV)
    out = trainops.MapListSweep._launch(p, y, off, np.ascontiguousarray(temperatures, np.float64), ty, per_image)
    torch.cuda.synchronize()
    assert all(t.dtype == torch.float64 for t in out)
    return tuple(t.cpu().numpy() for t in out)


def _bits(*arrays):
    return [np.ascontiguousarray(a, np.float64).view(np.uint64).tolist() for a in arrays]


def _worst(got, want):
    return float((np.abs(got - want) / (1e-9 * np.abs(want) + 1e-12)).max())


@pytest.mark.parametrize("per_image", MODES, ids=["label_mean", "image_mean"])
@pytest.mark.parametrize("S", [1, 2, 33, 64])
@pytest.mark.parametrize("batch", list(BATCHES))
def test_kernels_against_the_torch_statement_in_float64(gpu_required, batch, S, per_image):
    pred, label, offsets = values(BATCHES[batch], "replay")
    got = _launch(pred, label, offsets, grid(S), per_image)
    want = reference(batch, S, per_image)
    for name, a, b in zip(("curve", "rows", "images"), got, want):
        assert a.shape == b.shape and np.isfinite(a).all(), name                 # 1e-4 .. 1e4: finite rows
        print(f"{batch} S={S} per_image={per_image}: {name} largest |got - ref| / (1e-9 |ref| + 1e-12) = {_worst(a, b):.3e}")
        assert _worst(a, b) <= 1.0, name
    curve, rows, images = got
    lengths = np.asarray(BATCHES[batch])
    assert curve[:, 6].tolist() == [float((lengths >= 2).sum())] * S and curve[:, 7].tolist() == [float(lengths[lengths >= 2].sum())] * S
    assert images[:, 0].tolist() == [float(k) if k >= 2 else 0.0 for k in lengths]
    assert not rows[lengths < 2].view(np.uint64).any() and not images[lengths < 2].view(np.uint64).any()   # not listed: +0.0
    assert (rows[:, :, 2] >= 0.0).all() and (curve[:, 0] > 0.0).all()             # no case passes vacuously
    assert _bits(*got) == _bits(*_launch(pred, label, offsets, grid(S), per_image))   # equal inputs: equal bits


@pytest.mark.parametrize("per_image", MODES, ids=["label_mean", "image_mean"])
def test_column_0_is_fs_map_list_loss_at_every_temperature(gpu_required, per_image):
    """rows[b, s, 0], rounded to float32, within one float32 ulp of the table's D_b; curve[s, 0] against stats[1] to 1e-12."""
    from flingbot_amd import trainops

    pred, label, offsets = values(EDGES, "replay")
    temperatures = grid(33)
    curve, rows, _ = _launch(pred, label, offsets, temperatures, per_image)
    p, y = torch.from_numpy(pred).to(DEV), torch.from_numpy(label).to(DEV)
    off = torch.from_numpy(offsets.astype(np.int32)).to(DEV)
    worst = 0.0
    for s, t in enumerate(temperatures):
        _, stats, table = trainops.MapListFunction._launch(p, y, off, 1.0, float(t), TY, per_image)
        stats, D = stats.cpu().numpy(), table.cpu().numpy()[:, 0]
        assert (np.abs(rows[:, s, 0].astype(np.float32) - D) <= np.spacing(np.abs(D))).all(), (s, t)
        worst = max(worst, abs(curve[s, 0] - stats[1]) / abs(stats[1]))
        assert abs(curve[s, 0] - stats[1]) <= 1e-12 * abs(stats[1]), (s, t, curve[s, 0], stats[1])
        assert curve[s, 6] == stats[2] and curve[s, 7] == stats[3]
    print(f"per_image={per_image}: list against fs_map_list_loss' over 33 temperatures, largest relative difference {worst:.3e}")


def test_an_image_does_not_depend_on_its_place_or_on_the_others(gpu_required):
    """Image 7 of the batch (257 labels: two register slots) alone, first, last and between others: the bits of its rows."""
    pred, label, offsets = values(EDGES, "replay")
    temperatures = grid(33)
    _, rows, images = _launch(pred, label, offsets, temperatures, False)
    piece = lambda b: (pred[offsets[b]:offsets[b + 1]], label[offsets[b]:offsets[b + 1]])   # noqa: E731
    for order in ([7], [7, 3, 9], [3, 9, 7], [9, 7, 0, 4]):
        p = np.concatenate([piece(b)[0] for b in order])
        y = np.concatenate([piece(b)[1] for b in order])
        for per_image in MODES:
            _, rows2, images2 = _launch(p, y, sref.offsets_of([EDGES[b] for b in order]), temperatures, per_image)
            assert _bits(rows2, images2) == _bits(rows[order], images[order]), (order, per_image)
    assert rows[7].all() and images[7, 0] == 257.0


def test_a_non_finite_image_stays_alone(gpu_required):
    """A NaN, an infinity or an image of NaNs: every entry of that image's rows and columns 0-5 of the curve are non-finite, the
    other images' rows keep their bits, and the counts stay."""
    pred, label, offsets = values(EDGES, "replay")
    temperatures = grid(33)
    curve, rows, images = _launch(pred, label, offsets, temperatures, False)
    lo, hi = int(offsets[6]), int(offsets[7])                                    # image 6: 256 labels
    others = np.arange(len(EDGES)) != 6
    cases = [("pred", lo + 100, np.nan), ("label", lo + 100, np.nan), ("pred", lo + 3, np.inf), ("pred", lo + 3, -np.inf),
             ("label", lo + 255, np.inf), ("both", slice(lo, hi), np.nan)]
    for which, at, value in cases:
        p, y = pred.copy(), label.copy()
        if which in ("pred", "both"):
            p[at] = value
        if which in ("label", "both"):
            y[at] = value
        curve2, rows2, images2 = _launch(p, y, offsets, temperatures, False)
        assert not np.isfinite(rows2[6]).any() and not np.isfinite(curve2[:, :6]).any(), (which, value)
        assert _bits(rows2[others], images2[others]) == _bits(rows[others], images[others]), (which, value)
        assert curve2[:, 6:].tolist() == curve[:, 6:].tolist() and images2[6, 0] == 256.0
    assert torch.zeros(1, device=DEV).item() == 0.0


@pytest.mark.parametrize("name", ["affine", "noisy"])
def test_fit_temperature_walks_the_host_path(gpu_required, name):
    from flingbot_amd import trainops

    pred, label, offsets = sref.affine_set(0.5) if name == "affine" else sref.noisy_set()
    host = trainops.fit_temperature(torch.from_numpy(pred), torch.from_numpy(label), offsets, TY)
    before = trainops.MapListSweep.n_forward
    fit = trainops.fit_temperature(torch.from_numpy(pred).to(DEV), torch.from_numpy(label).to(DEV), offsets, TY)
    print(name, {k: v for k, v in fit.items() if k != "first_curve"}, "host", host["temperature"], host["chosen"])
    assert trainops.MapListSweep.n_forward == before + fit["sweeps"]                # the kernels, one sweep per round
    assert fit["sweeps"] == host["sweeps"] == 6 and fit["chosen"] == host["chosen"] and fit["at_bound"] is None
    assert abs(fit["temperature"] / host["temperature"] - 1.0) <= 1e-9
    assert abs(fit["list"] - host["list"]) <= 1e-9 * abs(host["list"]) + 1e-12
    assert abs(fit["temperature"] / (0.05 if name == "affine" else 0.13541) - 1.0) < 1e-3
    for a, b in zip(fit["first_curve"], host["first_curve"]):
        assert all(abs(a[k] - b[k]) <= 1e-9 * abs(b[k]) + 1e-12 for k in a), a["temperature"]


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def _policy():
    from flingbot_amd import nets

    torch.manual_seed(31)
    return nets.MaximumValuePolicy(action_primitives=["fling"], num_rotations=12, scale_factors=[1.0], obs_dim=64, pix_grasp_dist=8,
                                   pix_drag_dist=8, pix_place_dist=5, rgb_only=True, depth_only=False, action_expl_prob=0.0,
                                   action_expl_decay=1.0, value_expl_prob=0.0, value_expl_decay=1.0, device=DEV)


def test_score_maps_with_a_fitted_temperature(gpu_required):
    from flingbot_amd import train, trainops
    from flingbot_amd.replay import MapSet

    counts = [17, 1, 40, 5, 0, 9]
    rng = np.random.default_rng(8)
    images = rng.random((6, 4, 64, 64), dtype=np.float32)
    pixels = np.concatenate([np.sort(rng.choice(4096, n, replace=False)) for n in counts]).astype(np.int32)
    labels = (rng.standard_normal(len(pixels)) * 0.1).astype(np.float32)
    maps = MapSet.from_arrays(images, sref.offsets_of(counts), pixels, labels).to_device(DEV)
    policy = _policy()
    before = trainops.MapListSweep.n_forward
    out = train.score_maps(policy, {"fling": maps}, images_per_batch=4, list_temperature=0.1, label_temperature=TY, fit_temperature=True)["fling"]
    fit = out["list_fit"]
    assert trainops.MapListSweep.n_forward == before + fit["sweeps"]                # one fit over both batches
    assert len(fit["curve"]) == 33 and fit["curve"][0]["temperature"] == 1e-3 and fit["curve"][-1]["temperature"] == 1e2
    print({k: v for k, v in fit.items() if k != "curve"}, "list_kl at 0.1:", out["list_kl"])
    assert fit["list_kl"] <= out["list_kl"]                                        # not larger than at 0.1
    at = train.score_maps(policy, {"fling": maps}, list_temperature=fit["temperature"], label_temperature=TY)["fling"]
    assert abs(at["list_kl"] - fit["list_kl"]) <= 1e-9 * abs(fit["list_kl"])
    # the coldest draw is the arg-max: score_maps' regret, which also counts the map of one label (regret 0) -- 5 maps against 4
    assert out["n_maps"] == 5 and abs(4 * fit["curve"][0]["expected_regret"] - 5 * out["regret"]) < 1e-9
    plain = train.score_maps(policy, {"fling": maps}, images_per_batch=4, list_temperature=0.1, label_temperature=TY)["fling"]
    assert "list_fit" not in plain and {k: v for k, v in out.items() if k != "list_fit"} == plain


def test_fit_maps_refits_with_one_sweep_chain_each(gpu_required, tmp_path):
    import json
    import os

    from flingbot_amd import train, trainops

    paths = tiny_files(tmp_path)
    policy = _policy()
    opt = train.make_optimizer(policy, hip=True)
    log = str(tmp_path / "fitted")
    sweeps, lists = trainops.MapListSweep.n_forward, trainops.MapListFunction.n_forward
    out = train.fit_maps(policy, opt, paths, log, 3, images_per_batch=2, seed=5, hip_step=True, map_loss=True, list_weight=0.5,
                         list_temperature="fit", label_temperature=TY, refit_every=2)
    lines = [json.loads(l) for l in open(os.path.join(log, train.TRAIN_LOG))]
    assert [("refit" in l, l["step"]) for l in lines] == [(True, 0), (False, 1), (False, 2), (True, 2), (False, 3)]
    refits = [l for l in lines if l.get("refit")]
    print(refits)
    assert trainops.MapListSweep.n_forward == sweeps + sum(l["sweeps"] for l in refits)   # a chain per refit, none per batch
    assert trainops.MapListFunction.n_forward == lists + 3 and out["steps"] == 3
    assert all(np.isfinite(l["loss"]) for l in lines if l.get("fit")) and all(l["list_kl"] >= 0.0 for l in refits)
    assert out["primitives"]["fling"]["list_temperature"] == refits[-1]["list_temperature"]
