"""The map loss without a GPU: the float64 restatement (maploss_reference.py) against grouploss_reference on the expanded
bounds, trainops.map_loss_torch against the restatement in both normalisations, MapLossFunction on host tensors,
optimize_maps / fit_maps / the command line with map_loss, and the fs_map_loss entry point's header line, export and argument
checks."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import grouploss_reference as gref
import maploss_reference as mref
from test_mapset_cpu import _policy, files  # noqa: F401  (files: the module's fixture of two replay files)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, TAU = 0.5, 0.1
# labels per image: the CPU-sized cases
LAYOUTS = [[1], [2], [5], [64], [65], [257], [0, 3, 0, 0, 7, 0], [12] * 7, [40, 1, 17, 0, 64], [1, 1, 1], [300, 2]]


def _case(lengths, seed=None):
    offsets = mref.offsets_of(lengths)
    pred, label = gref.batch(int(offsets[-1]), seed=sum(lengths) if seed is None else seed)
    return pred, label, offsets


def _torch64(pred, label, offsets, gap, per_image):
    """trainops.map_loss_torch in float64: (stats, table, gradient) as numpy."""
    from flingbot_amd import trainops

    p = torch.tensor(np.asarray(pred, np.float64), requires_grad=True)
    loss, stats, table = trainops.map_loss_torch(p, torch.tensor(np.asarray(label, np.float64)), offsets, W, TAU, gap, per_image)
    (grad,) = torch.autograd.grad(loss, p)
    assert loss.item() == stats[0].item()
    return stats.numpy(), table.numpy(), grad.numpy()


def _same_to_float64(ref, stats, table, grad, scale=1.0):
    for k, name in enumerate(("loss", "mse", "rank")):
        assert abs(stats[k] - ref[name][0]) <= 1e-13 * max(1.0, ref[name][2]), name
    assert stats[3:].tolist() == [ref["pairs"], ref["concordant"], ref["filled"], ref["ranked"], 0.0]
    for b, row in enumerate(ref["table"]):
        assert table[b, 2] == row["pairs"] and table[b, 3] == row["concordant"]
        assert abs(table[b, 0] - row["mse"][0]) <= 1e-13 * max(1.0, row["mse"][2]) and abs(table[b, 1] - row["rank"][0]) <= 1e-13 * max(1.0, row["rank"][2])
    assert np.abs(scale * grad - ref["dpred"][0]).max() <= 1e-13 * max(1.0, ref["dpred"][2].max())


# ---- the restatement, and the torch statement in float64 against it -------------------------------------------------------------
@pytest.mark.parametrize("lengths", LAYOUTS)
@pytest.mark.parametrize("gap", [0.0, 0.05])
def test_label_mean_restatement_is_the_group_restatement_on_expanded_bounds(lengths, gap):
    pred, label, offsets = _case(lengths)
    got = mref.map_loss_f64(pred, label, offsets, W, TAU, gap, False, scale=0.5)
    want = gref.group_loss_f64(pred, label, mref.expanded_bounds(offsets), W, TAU, gap, scale=0.5)
    assert got["pairs"] == want["pairs"] and got["concordant"] == want["concordant"]
    assert got["pairs"] == sum(row["pairs"] for row in got["table"])
    for name in ("loss", "mse", "rank"):
        assert abs(got[name][0] - want[name][0]) <= 1e-14 * abs(want[name][0]), name
        assert got[name][1] == want[name][1] and abs(got[name][2] - want[name][2]) <= 1e-14 * want[name][2], name
    assert np.abs(got["dpred"][0] - want["dpred"][0]).max() <= 1e-14 * np.abs(want["dpred"][0]).max()
    assert np.array_equal(got["dpred"][1], want["dpred"][1])
    assert np.abs(got["dpred"][2] - want["dpred"][2]).max() <= 1e-14 * want["dpred"][2].max()
    for per_image in (False, True):
        _same_to_float64(mref.map_loss_f64(pred, label, offsets, W, TAU, gap, per_image), *_torch64(pred, label, offsets, gap, per_image))


def test_image_mean_restatement_by_hand():
    """Two images; the first has two pairs, the second none."""
    pred, label = np.array([0.3, 0.1, 0.2, 0.5, 0.7]), np.array([1.0, 0.0, 0.0, 2.0, 2.0])
    out = mref.map_loss_f64(pred, label, [0, 3, 5], W, TAU, 0.0, True)
    s = [(0.7 ** 2 + 0.1 ** 2 + 0.2 ** 2) / 3, (1.5 ** 2 + 1.3 ** 2) / 2]
    r = (gref.softplus(-2.0) + gref.softplus(-1.0)) / 2
    assert (out["pairs"], out["concordant"], out["filled"], out["ranked"]) == (2, 2, 2, 1)
    assert abs(out["mse"][0] - (s[0] + s[1]) / 2) < 1e-15 and abs(out["rank"][0] - r) < 1e-15
    assert abs(out["loss"][0] - ((s[0] + s[1]) / 2 + W * r)) < 1e-15
    sig = gref.sigma(np.array([-2.0, -1.0]))
    d = out["dpred"][0]
    assert abs(d[0] - (2 * -0.7 / (2 * 3) - W / (1 * 2 * TAU) * sig.sum())) < 1e-14
    assert abs(d[1] - (2 * 0.1 / (2 * 3) + W / (1 * 2 * TAU) * sig[0])) < 1e-14
    assert d[3] == 2 * -1.5 / (2 * 2) and out["dpred"][1].tolist() == [3, 2, 2, 1, 1]
    assert [row["pairs"] for row in out["table"]] == [2, 0] and out["table"][1]["rank"][0] == 0.0
    assert abs(out["table"][0]["mse"][0] - s[0]) < 1e-15 and abs(out["table"][0]["rank"][0] - r) < 1e-15
    _same_to_float64(out, *_torch64(pred, label, np.array([0, 3, 5]), 0.0, True))


# ---- the torch statement ----------------------------------------------------------------------------------------------------
def _compare(ref, loss, stats, table, grad):
    """The largest |got - ref| / bound over the outputs; the counts exactly."""
    stats, table, worst = np.asarray(stats, np.float64), np.asarray(table, np.float64), 0.0
    assert float(loss) == stats[0]
    assert stats[3:].tolist() == [ref["pairs"], ref["concordant"], ref["filled"], ref["ranked"], 0.0]
    for k, name in enumerate(("loss", "mse", "rank")):
        value, n, A = ref[name]
        assert abs(stats[k] - value) <= gref.bound(n, A), name
        worst = max(worst, abs(stats[k] - value) / gref.bound(n, A)) if A else worst
    for b, row in enumerate(ref["table"]):
        assert table[b, 2] == row["pairs"] and table[b, 3] == row["concordant"], b
        for k, name in enumerate(("mse", "rank")):
            value, n, A = row[name]
            assert abs(table[b, k] - value) <= gref.bound(n, A), (b, name)
    value, n, A = ref["dpred"]
    assert (np.abs(np.asarray(grad, np.float64) - value) <= gref.bound(n, A)).all()
    return worst


@pytest.mark.parametrize("lengths", LAYOUTS)
@pytest.mark.parametrize("per_image", [False, True])
def test_torch_statement_in_float32_is_within_the_bound(lengths, per_image):
    from flingbot_amd import trainops

    pred, label, offsets = _case(lengths)
    ref = mref.map_loss_f64(pred, label, offsets, W, TAU, 0.0, per_image)
    p = torch.tensor(pred, requires_grad=True)
    loss, stats, table = trainops.map_loss_torch(p, torch.tensor(label), offsets, W, TAU, 0.0, per_image)
    (grad,) = torch.autograd.grad(loss, p)
    assert stats.dtype == table.dtype == torch.float32 and tuple(table.shape) == (len(lengths), 4)
    assert not stats.requires_grad and not table.requires_grad
    _compare(ref, loss.item(), stats.numpy(), table.numpy(), grad.numpy())


@pytest.mark.parametrize("lengths", [[5], [12] * 7, [0, 3, 0, 0, 7, 0]])
def test_torch_statement_with_the_label_mean_is_group_loss_torch(lengths):
    from flingbot_amd import trainops

    pred, label, offsets = _case(lengths)
    p, q = torch.tensor(pred, requires_grad=True), torch.tensor(pred, requires_grad=True)
    loss, stats, _ = trainops.map_loss_torch(p, torch.tensor(label), offsets, W, TAU, 0.0, False)
    want, want_stats = trainops.group_loss_torch(q, torch.tensor(label), mref.expanded_bounds(offsets), W, TAU, 0.0)
    assert abs(loss.item() - want.item()) <= 1e-6 * abs(want.item()) and torch.equal(stats[3:5], want_stats[3:5])
    (g,), (h,) = torch.autograd.grad(loss, p), torch.autograd.grad(want, q)
    assert (g - h).abs().max() <= 1e-6 * h.abs().max()


# ---- MapLossFunction on host tensors ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_image", [False, True])
def test_map_loss_function_on_the_host(per_image):
    from flingbot_amd import trainops

    pred, label, offsets = _case([40, 1, 17, 0, 64])
    ref = mref.map_loss_f64(pred, label, offsets, W, TAU, 0.0, per_image)
    before = trainops.MapLossFunction.n_forward
    p = torch.tensor(pred, requires_grad=True)
    loss, stats, table = trainops.MapLossFunction.apply(p, torch.tensor(label), offsets, W, TAU, 0.0, per_image)
    assert trainops.MapLossFunction.n_forward == before                        # (counts kernel calls)
    assert loss.requires_grad and not stats.requires_grad and not table.requires_grad and loss.dtype == torch.float32
    (3.5 * loss).backward()
    scaled = mref.map_loss_f64(pred, label, offsets, W, TAU, 0.0, per_image, scale=3.5)
    _compare(ref, loss.item(), stats.numpy(), table.numpy(), p.grad.numpy() / 3.5)
    assert (np.abs(p.grad.numpy().astype(np.float64) - scaled["dpred"][0]) <= gref.bound(scaled["dpred"][1] + 1, scaled["dpred"][2])).all()
    # offsets as a host tensor are the same call
    loss2, stats2, _ = trainops.MapLossFunction.apply(torch.tensor(pred), torch.tensor(label), torch.from_numpy(offsets), W, TAU, 0.0,
                                                      per_image)
    assert torch.equal(loss2, loss.detach()) and torch.equal(stats2, stats)


def test_map_loss_function_refuses_bad_tables_and_scalars():
    from flingbot_amd import trainops

    z = torch.zeros(6)
    apply = lambda off, p=z, y=z, w=W, tau=TAU, gap=0.0: trainops.MapLossFunction.apply(p, y, off, w, tau, gap, False)   # noqa: E731
    apply(np.array([0, 2, 6]))
    for bad in ([1, 2, 6],                       # offsets[0] != 0
                [0, 4, 2, 6],                    # falling
                [0, -1, 6],                      # negative (falls)
                [0, 2, 5],                       # offsets[G] != len(pred)
                [0, 2, 7],                       # past the labels
                [0.0, 2.0, 6.0],                 # not integers
                [[0, 2, 6]],                     # not [G + 1]
                [6]):                            # no image
        with pytest.raises(ValueError):
            apply(np.array(bad))
    with pytest.raises(ValueError, match="4096"):
        big = torch.zeros(5000)
        apply(np.array([0, 5000]), big, big)
    apply(np.array([0, 4096, 5000]), big, big)                                  # 4096 is served
    with pytest.raises(ValueError, match="at least one label"):
        apply(np.array([0, 0, 0]), torch.zeros(0), torch.zeros(0))
    with pytest.raises(ValueError):
        apply(np.array([0, 2, 6]), z, torch.zeros(5))
    with pytest.raises(ValueError):
        apply(np.array([0, 2, 6]), z, z.double())
    for kw in (dict(w=-0.1), dict(w=float("nan")), dict(tau=0.0), dict(tau=float("inf")), dict(gap=-1e-9), dict(gap=float("nan"))):
        with pytest.raises(ValueError):
            apply(np.array([0, 2, 6]), **kw)


# ---- header and library -------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    from flingbot_amd import build, sim as fsim

    with open(os.path.join(ROOT, "include", "flingsim.h")) as fh:
        header = fh.read()
    assert re.search(r"^int fs_map_loss\(", header, re.M) and re.search(r"^size_t fs_map_loss_work_bytes\(int images, int labels\);", header, re.M)
    assert "begin = clamp(off[b], 0, L)" in header and "min(end, begin + 4096)" in header      # the clamp is stated
    lib = fsim.load_library()
    for name in ("fs_map_loss", "fs_map_loss_work_bytes"):
        assert getattr(lib, name) is not None and name in lib._fs_symbols
    assert "fs_maploss.hip" in build.LIB_SOURCES
    assert lib.fs_map_loss_work_bytes(0, 5) == lib.fs_map_loss_work_bytes(5, 0) == lib.fs_map_loss_work_bytes(-1, -1) == 0
    assert lib.fs_map_loss_work_bytes(3, 1000) >= 4 * 1000 + 3 * 16 * 16
    assert lib.fs_map_loss_work_bytes(1 << 20, (1 << 31) - 1) > 1 << 33                       # sized in size_t


def test_entry_point_refuses_bad_scalars_and_pointers():
    """FS_ERR_ARG before any HIP call: the pointers are host addresses that are never dereferenced."""
    from flingbot_amd import sim as fsim

    lib = fsim.load_library()
    buf = np.zeros(4096, np.float64)
    at = lambda k: C.c_void_p(buf.ctypes.data + 64 * k)   # noqa: E731
    ok = dict(pred=at(0), label=at(1), offsets=at(2), images=2, labels=4, w=0.5, tau=0.1, gap=0.0, per_image=0, s=1.0, dpred=at(3),
              stats=at(4), table=at(5), work=at(6))
    call = lambda **a: lib.fs_map_loss(a["pred"], a["label"], a["offsets"], a["images"], a["labels"], a["w"], a["tau"], a["gap"],   # noqa: E731
                                       a["per_image"], a["s"], a["dpred"], a["stats"], a["table"], a["work"], None)
    nan, inf = float("nan"), float("inf")
    cases = [dict(images=0), dict(images=-3), dict(labels=0), dict(labels=-1), dict(per_image=2), dict(per_image=-1), dict(w=-0.1),
             dict(w=nan), dict(w=inf), dict(tau=0.0), dict(tau=-0.1), dict(tau=nan), dict(tau=inf), dict(tau=5e-324), dict(gap=-1e-9),
             dict(gap=nan), dict(gap=inf), dict(s=nan), dict(s=inf), dict(s=-inf)]
    pointers = ("pred", "label", "offsets", "dpred", "stats", "table", "work")
    cases += [{k: C.c_void_p(None)} for k in pointers]
    cases += [{k: C.c_void_p(buf.ctypes.data + 2)} for k in pointers]
    cases += [{k: C.c_void_p(buf.ctypes.data + 4)} for k in ("stats", "work")]               # 4- but not 8-byte aligned
    for kw in cases:
        assert call(**{**ok, **kw}) == -1, kw                               # FS_ERR_ARG
        assert b"fs_map_loss" in lib.fs_last_error(), kw


# ---- optimize_maps / fit_maps / the command line ------------------------------------------------------------------------------
COUNTS = [1000, 1200, 900, 1100, 1000]


def big_maps(seed=11):
    """A MapSet of 5 images with COUNTS distinct labelled pixels each: 5200 labels, more than fs_group_loss serves."""
    from flingbot_amd.replay import MapSet

    rng = np.random.default_rng(seed)
    images = rng.random((5, 4, 64, 64), dtype=np.float32)
    pixels = np.concatenate([np.sort(rng.choice(4096, n, replace=False)) for n in COUNTS]).astype(np.int32)
    labels = (np.round(rng.standard_normal(len(pixels)) * 0.1 / 0.05) * 0.05).astype(np.float32)      # with ties
    return MapSet.from_arrays(images, mref.offsets_of(COUNTS), pixels, labels)


def host_pairs_of_draw(maps, n_images, seed):
    """P of the batch optimize_maps' first update draws from default_rng(seed), counted on the host."""
    _, offsets, positions, _ = maps.draw_maps(n_images, np.random.default_rng(seed))
    return gref.host_pairs(maps.labels[positions], mref.expanded_bounds(offsets)), int(offsets[-1])


def test_optimize_maps_with_map_loss_takes_what_the_default_path_refuses():
    from flingbot_amd import train

    maps = big_maps()
    want_pairs, want_labels = host_pairs_of_draw(maps, 5, 4)
    ends = []
    for _ in range(2):
        policy, opt = _policy()
        net = policy.value_nets["fling"]
        start = {k: v.clone() for k, v in net.state_dict().items()}
        policy.train()
        rows = []
        losses = train.optimize_maps("fling", net, opt, maps, 1, 5, np.random.default_rng(4), rank_weight=0.5, map_loss=True, stats=rows)
        policy.eval()
        assert len(losses) == 1 and np.isfinite(losses[0]) and int(net.steps) == 1
        assert set(rows[0]) == {"loss", "images", "labels", "mse", "rank", "pairs", "concordant", "images_with_pairs", "map_pair_accuracy"}
        assert rows[0]["loss"] == losses[0] and rows[0]["images"] == 5 and rows[0]["labels"] == want_labels > 4096
        assert rows[0]["pairs"] == want_pairs > 0 and 0 <= rows[0]["concordant"] <= want_pairs and rows[0]["images_with_pairs"] == 5
        assert 0.0 <= rows[0]["map_pair_accuracy"] <= 1.0
        assert any(not torch.equal(v, start[k]) for k, v in net.state_dict().items())
        ends.append((net.state_dict(), rows))
    for k, v in ends[0][0].items():
        assert torch.equal(v, ends[1][0][k]), k
    assert ends[0][1] == ends[1][1]
    # the default path still refuses the same call, and per_image needs map_loss
    policy, opt = _policy()
    net = policy.value_nets["fling"]
    with pytest.raises(ValueError, match="4096"):
        train.optimize_maps("fling", net, opt, maps, 1, 5, np.random.default_rng(4), rank_weight=0.5, map_loss=False)
    with pytest.raises(ValueError, match="map_loss"):
        train.optimize_maps("fling", net, opt, maps, 1, 5, np.random.default_rng(4), per_image=True)
    assert int(net.steps) == 0


def test_optimize_maps_with_map_loss_and_weight_zero_is_the_regression(files):   # noqa: F811
    """rank_weight = 0 with the label mean: the loss is mse_loss' value to rounding, and the rows carry the map statistics."""
    from flingbot_amd import train
    from flingbot_amd.replay import MapSet

    maps = MapSet(list(files), action_primitive="fling")
    got = []
    for extra in (dict(), dict(map_loss=True), dict(map_loss=True, per_image=True)):
        policy, opt = _policy()
        policy.train()
        rows = []
        got.append((train.optimize_maps("fling", policy.value_nets["fling"], opt, maps, 1, 3, np.random.default_rng(0), stats=rows, **extra), rows))
    (plain, plain_rows), (label_mean, rows), (image_mean, image_rows) = got
    assert set(plain_rows[0]) == {"loss", "images", "labels"}
    assert abs(label_mean[0] - plain[0]) <= 1e-6 * plain[0] and rows[0]["rank"] >= 0.0 and rows[0]["mse"] == pytest.approx(plain[0], rel=1e-6)
    assert rows[0]["pairs"] == image_rows[0]["pairs"] and np.isfinite(image_mean[0]) and "map_pair_accuracy" in image_rows[0]


def test_fit_maps_log_lines_with_and_without_the_flag(files, tmp_path):   # noqa: F811
    from flingbot_amd import train

    base = {"fit", "primitive", "step", "loss", "images", "labels"}
    ranked = base | {"mse", "rank", "pairs", "pair_accuracy"}
    full = ranked | {"images_with_pairs", "map_pair_accuracy"}
    for name, kwargs, keys in (("plain", dict(), base), ("ranked", dict(pixels_per_image=2, rank_weight=0.5), ranked),
                               ("map", dict(rank_weight=0.5, map_loss=True), full), ("map0", dict(map_loss=True, per_image=True), full)):
        policy, opt = _policy()
        log = str(tmp_path / name)
        out = train.fit_maps(policy, opt, list(files), log, 1, images_per_batch=3, seed=5, **kwargs)
        assert out["steps"] == 1
        lines = [json.loads(l) for l in open(os.path.join(log, train.TRAIN_LOG))]
        assert len(lines) == 1 and set(lines[0]) == keys, name
        if "map_pair_accuracy" in keys:
            acc = lines[0]["map_pair_accuracy"]
            assert (acc is None) == (lines[0]["images_with_pairs"] == 0) and (acc is None or 0.0 <= acc <= 1.0)
    policy, opt = _policy()
    with pytest.raises(ValueError, match="map_loss"):
        train.fit_maps(policy, opt, list(files), str(tmp_path / "bad"), 1, images_per_batch=3, per_image=True)


def test_command_line_takes_the_flags():
    from flingbot_amd import train

    ap = train.build_parser()
    a = ap.parse_args(["--log", "x", "--fit-maps", "p.npz"])
    assert a.map_loss is False and a.per_image is False
    a = ap.parse_args(["--log", "x", "--fit-maps", "p.npz", "--rank-weight", "0.5", "--map-loss", "--per-image"])
    assert a.map_loss is True and a.per_image is True and a.pixels_per_image is None
    with pytest.raises(SystemExit):
        train.main(["--log", "x", "--fit-maps", "p.npz", "--per-image"])          # refused before anything is loaded
