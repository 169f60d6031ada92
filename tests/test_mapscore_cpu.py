"""Held-out scoring of recorded reward maps, the parts that need no GPU: the float64 restatement (mapscore_reference.py) and
trainops.map_score_host against probe.map_stats, constructed rows, summarize_scores, MapSet.take_maps, fit_maps with a held-out
set against fit_maps without one, the --score-maps command line, and the fs_map_score entry point's header text, export and
argument checks."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import maploss_reference as mref
import mapscore_reference as sref
from test_mapset_cpu import TASKS, _cell, _image, _policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def _one(p, y, gap=0.0):
    """(restatement row, map_score_host row) of one image whose predictions sit at pixels 0 .. n-1 of its map."""
    from flingbot_amd import trainops

    p, y = np.asarray(p, np.float32), np.asarray(y, np.float32)
    value = np.zeros((1, 4096), np.float32)
    value[0, :len(p)] = p
    table, pix = np.array([0, len(p)]), np.arange(len(p))
    ref, _ = sref.score_rows(value, table, pix, y, gap)
    host = trainops.map_score_host(value, table, pix, y, gap)
    return ref[0], host[0]


def _same_row(a, b):
    assert a[:9].tolist() == b[:9].tolist()
    assert sref.same_bits(a[9:11], b[9:11]), (a, b)
    assert abs(a[11] - b[11]) <= (a[0] + 16) * 2.0 ** -53 * max(a[11], b[11])


# ---- against probe.map_stats ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quantised", [False, True], ids=["untied", "quarters"])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 65, 144, 257, 1024])
def test_restatement_and_host_path_are_map_stats(n, quantised):
    from flingbot_amd import probe

    p, y = sref.values(n, 5, quantised)
    if quantised and n >= 64:
        assert sref.has_ties(p) and sref.has_ties(y)                       # the tied cases really hold ties
    if not quantised:
        assert not sref.has_ties(p) and not sref.has_ties(y)
    ref, host = _one(p, y)
    _same_row(ref, host)
    want = probe.map_stats(p, y, (int(ref[1]),), 1.0)
    for row in (ref, host):
        assert (int(row[0]), int(row[3]), int(row[4]), int(row[5])) == (want["n_cells"], want["chosen_rank"], want["pairs"], want["concordant"])
        assert row[1] == int(np.argmax(p)) and row[2] == int(np.argmax(y))
        assert np.float64(row[10]).tobytes() == np.float64(want["lattice_regret"]).tobytes()
        if want["spearman"] is None:
            assert math.isnan(row[9]) and (n < 2 or row[7] == 0 or row[8] == 0)
        else:
            assert np.float64(row[9]).tobytes() == np.float64(want["spearman"]).tobytes()
    if n == 1:
        assert math.isnan(ref[9]) and ref[4] == 0
    if n >= 5:
        assert ref[4] > 0 and not math.isnan(ref[9])


# ---- constructed rows -----------------------------------------------------------------------------------------------------------
def test_equal_predictions_choose_the_lowest_k_and_have_no_spearman():
    for row in _one([0.5] * 6, [0.1, 0.4, 0.2, 0.4, 0.0, 0.3]):
        assert row[:6].tolist() == [6, 0, 1, 4, 14, 0] and row[7] == 0 and row[8] > 0 and math.isnan(row[9])
        assert row[10] == float(np.float32(0.4)) - float(np.float32(0.1))


def test_best_label_tied_with_the_chosen_one():
    for row in _one([0.1, 0.9, 0.3, 0.2], [0.7, 0.7, 0.1, 0.7]):
        assert (row[1], row[2], row[3], row[10]) == (1, 0, 0, 0.0)             # chosen 1, best the lowest k of the tie: no regret


def test_non_finite_predictions_and_labels_are_left_out_of_every_column():
    p = [0.3, NAN, 0.1, INF, 0.2, 0.9, -INF, 0.4]
    y = [0.5, 9.0, NAN, 9.0, 0.1, -INF, 9.0, 0.3]
    clean = _one([0.3, 0.2, 0.4], [0.5, 0.1, 0.3])
    for row, want in zip(_one(p, y), clean):
        assert row[0] == 3 and (row[1], row[2]) == (7, 0) and (want[1], want[2]) == (2, 0)      # k counts every list position
        assert row[3:9].tolist() == want[3:9].tolist() and sref.same_bits(row[9:], want[9:])
    for row in _one([NAN, INF], [0.1, 0.2]) + _one([0.1, 0.2], [INF, NAN]):
        assert row[:9].tolist() == sref.EMPTY[:9] and math.isnan(row[9]) and math.isnan(row[10]) and row[11] == 0.0


def test_a_label_difference_equal_to_min_gap_is_no_pair_and_one_ulp_more_is():
    lo = np.float32(0.25)
    hi = np.float32(0.75)
    gap = float(hi) - float(lo)                                                 # exact in double
    for row in _one([0.1, 0.2], [lo, hi], gap):
        assert (row[4], row[5]) == (0, 0)
    for row in _one([0.1, 0.2], [lo, np.nextafter(hi, np.float32(1))], gap):
        assert (row[4], row[5]) == (1, 1)
    for row in _one([0.1, 0.2], [lo, hi], 0.0):
        assert (row[4], row[5]) == (1, 1)


def test_an_empty_image_writes_its_fixed_row():
    from flingbot_amd import trainops

    value = np.zeros((3, 4096), np.float32)
    value[0, 5], value[2, 9] = 0.5, 0.25
    table, pix, y = np.array([0, 1, 1, 2]), np.array([5, 9]), np.float32([0.1, 0.2])
    ref, _ = sref.score_rows(value, table, pix, y)
    host = trainops.map_score_host(value, table, pix, y)
    for rows in (ref, host, trainops.map_score(torch.from_numpy(value), table, torch.from_numpy(pix), torch.from_numpy(y)).numpy()):
        assert rows.shape == (3, 12) and rows.dtype == np.float64
        assert rows[1, :9].tolist() == sref.EMPTY[:9] and np.isnan(rows[1, 9:11]).all() and rows[1, 11] == 0.0
        assert rows[0, :6].tolist() == [1, 0, 0, 0, 0, 0] and rows[2, :6].tolist() == [1, 0, 0, 0, 0, 0] and rows[2, 10] == 0.0
    assert np.array_equal(trainops.empty_score_rows(1)[0, :9], np.array(sref.EMPTY[:9]))


def test_map_score_on_the_host_validates_before_anything_else():
    from flingbot_amd import trainops

    value = torch.zeros(2, 1, 64, 64)
    pix, y = torch.tensor([0, 4095, 7], dtype=torch.int32), torch.zeros(3)
    rows = trainops.map_score(value, np.array([0, 2, 3]), pix, y)
    assert tuple(rows.shape) == (2, 12) and rows.dtype == torch.float64 and rows[:, 0].tolist() == [2, 1]
    for bad in ([0, 2], [1, 2, 3], [0, 3, 2, 3], [0, 2, 4], [0.0, 2.0, 3.0]):
        with pytest.raises(ValueError):
            trainops.map_score(value, np.array(bad), pix, y)
    same = torch.tensor([5, 5, 7], dtype=torch.int32)
    same.host = same.numpy()
    with pytest.raises(ValueError, match="distinct"):
        trainops.map_score(value, np.array([0, 2, 3]), same, y)
    for gap in (-1e-9, NAN, INF):
        with pytest.raises(ValueError, match="min_gap"):
            trainops.map_score(value, np.array([0, 2, 3]), pix, y, gap)
    with pytest.raises(ValueError):
        trainops.map_score(torch.zeros(2, 64, 64), np.array([0, 2, 3]), pix, y)
    with pytest.raises(ValueError, match="at least one label"):
        trainops.map_score(value, np.array([0, 0, 0]), pix[:0], y[:0])


def test_summary_by_hand_and_whatever_the_batches():
    from flingbot_amd import trainops

    p = [np.float32([0.1, 0.9, 0.3]), np.float32([0.5, 0.5]), np.zeros(0, np.float32), np.float32([0.2])]
    y = [np.float32([0.5, 0.25, 1.0]), np.float32([0.0, 1.0]), np.zeros(0, np.float32), np.float32([0.7])]
    rows = np.array([sref.score_image(a, b)[0] for a, b in zip(p, y)])
    out = trainops.summarize_scores(rows)
    assert (out["n_maps"], out["labels"], out["pairs"], out["concordant"], out["maps_with_spearman"]) == (3, 6, 4, 1, 1)
    assert out["regret"] == (0.75 + 1.0 + 0.0) / 3 and out["chosen_rank"] == (2 + 1 + 0) / 3 and out["top1"] == 1 / 3
    assert out["spearman"] == rows[0, 9] == -0.5 and out["pair_accuracy"] == 0.25 and out["map_pair_accuracy"] == (1 / 3 + 0.0) / 2
    assert out["mse"] == pytest.approx((0.16 + 0.4225 + 0.49 + 0.25 + 0.25 + 0.25) / 6, rel=1e-6)
    assert trainops.summarize_scores(torch.from_numpy(rows)) == out
    nothing = trainops.summarize_scores(rows[2:3])
    assert nothing["n_maps"] == 0 and nothing["labels"] == 0 and nothing["pairs"] == 0
    assert all(nothing[k] is None for k in ("regret", "chosen_rank", "top1", "spearman", "pair_accuracy", "map_pair_accuracy", "mse"))
    json.dumps(out), json.dumps(nothing)


# ---- MapSet.take_maps -----------------------------------------------------------------------------------------------------------
def _maps(seed=3, counts=(5, 0, 3, 7)):
    from flingbot_amd.replay import MapSet

    rng = np.random.default_rng(seed)
    images = rng.random((len(counts), 4, 64, 64), dtype=np.float32)
    pixels = np.concatenate([np.sort(rng.choice(4096, n, replace=False)) for n in counts]).astype(np.int32)
    labels = rng.standard_normal(len(pixels)).astype(np.float32)
    return MapSet.from_arrays(images, mref.offsets_of(counts), pixels, labels)


def test_take_maps_is_deterministic_and_is_the_host_arrays():
    maps = _maps()
    rng = np.random.default_rng(9)
    state = json.dumps(rng.bit_generator.state, sort_keys=True)
    order = [3, 0, 1, 3]
    obs, offsets, pix, labels = maps.take_maps(order)
    again = maps.take_maps(np.array(order))
    assert json.dumps(rng.bit_generator.state, sort_keys=True) == state
    assert obs.dtype == torch.float32 and tuple(obs.shape) == (4, 3, 64, 64) and offsets.tolist() == [0, 7, 12, 12, 19]
    assert torch.equal(obs, again[0]) and np.array_equal(offsets, again[1]) and torch.equal(pix, again[2])
    assert labels.numpy().tobytes() == again[3].numpy().tobytes()
    assert np.array_equal(obs.numpy(), maps.images[order, :3])                 # the recorded floats, rgb: no jitter, no quantisation
    want = np.concatenate([np.arange(maps.offsets[i], maps.offsets[i + 1]) for i in order])
    assert np.array_equal(pix.numpy(), maps.pixels[want]) and np.array_equal(pix.host, maps.pixels[want]) and pix.dtype == torch.int32
    assert labels.numpy().tobytes() == maps.labels[want].tobytes()
    none = maps.take_maps([])
    assert tuple(none[0].shape) == (0, 3, 64, 64) and none[1].tolist() == [0] and len(none[2]) == 0
    with pytest.raises(IndexError):
        maps.take_maps([4])
    # sample_maps still draws what draw_maps says
    a, b = maps.sample_maps(3, np.random.default_rng(1)), maps.sample_maps(3, np.random.default_rng(1))
    assert torch.equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and torch.equal(a[2], b[2])


# ---- score_maps and fit_maps on a host policy -----------------------------------------------------------------------------------
def test_score_maps_on_a_host_policy_is_the_restatement_of_its_own_dense_maps():
    from flingbot_amd import train

    maps = _maps()
    policy, _ = _policy()
    policy.train()
    state = {k: v.clone() for k, v in policy.state_dict().items()}
    seed = torch.random.get_rng_state()
    out = train.score_maps(policy, {"fling": maps}, images_per_batch=3, min_gap=0.05)
    assert policy.training and all(m.training for m in policy.modules())      # the flags it found
    assert torch.equal(torch.random.get_rng_state(), seed)
    assert all(torch.equal(v, state[k]) for k, v in policy.state_dict().items())
    policy.eval()
    with torch.no_grad():
        dense = policy.value_nets["fling"](torch.from_numpy(maps.images[:, :3])).reshape(4, 4096).numpy()
    from flingbot_amd import trainops
    rows, _ = sref.score_rows(dense, maps.offsets, maps.pixels, maps.labels, 0.05)
    want = trainops.summarize_scores(rows)
    assert want["n_maps"] == 3 and want["labels"] == 15 and want["pairs"] > 0
    whole = train.score_maps(policy, {"fling": maps}, images_per_batch=64, min_gap=0.05)
    for k, v in want.items():   # mse to float32 rounding (the host convolutions may round differently per batch size); the rest exactly
        for got in (out["fling"][k], whole["fling"][k]):
            assert got == (pytest.approx(v, rel=1e-5) if k == "mse" else v), k
    assert not policy.training


@pytest.fixture(scope="module")
def fit_files(tmp_path_factory):
    """train.npz: 3 images x 5 pixels; held.npz: 2 images x 5 pixels, the second with the bytes of a training image."""
    from flingbot_amd import lookahead

    pixels = [[(0, 0), (0, 1), (1, 0), (30, 31), (63, 63)], [(0, 0), (0, 1), (1, 0), (17, 5), (40, 63)],
              [(0, 0), (0, 1), (1, 0), (63, 0), (12, 12)]]
    images = [_image(20 + k) for k in range(4)]
    rng = np.random.default_rng(6)
    cells = lambda step, image, rows: [_cell(0, step, r, 1.0, 1.0 + float(rng.uniform(-0.3, 0.6)), rows[r], image) for r in range(5)]   # noqa: E731
    d = tmp_path_factory.mktemp("fit")
    fit, held = str(d / "train.npz"), str(d / "held.npz")
    assert lookahead.save_replay(fit, dict(lane_records=sum((cells(s, images[s], pixels[s]) for s in range(3)), [])), TASKS) == 15
    assert lookahead.save_replay(held, dict(lane_records=cells(0, images[3], pixels[1]) + cells(1, images[0], pixels[2])), TASKS) == 10
    return fit, held


def test_fit_maps_with_a_held_out_set_trains_as_without_one(fit_files, tmp_path):
    from flingbot_amd import train

    fit, held = fit_files
    runs = {}
    for name, extra in (("plain", dict()), ("held", dict(holdout=[held], validate_every=2))):
        policy, opt = _policy()
        log = str(tmp_path / name)
        out = train.fit_maps(policy, opt, [fit], log, 4, images_per_batch=3, seed=5, **extra)
        lines = [json.loads(l) for l in open(os.path.join(log, train.TRAIN_LOG))]
        runs[name] = (out, lines, torch.load(os.path.join(log, train.LATEST)))
        assert out["steps"] == 4 and not policy.training
    (plain, plain_lines, plain_ckpt), (out, lines, ckpt) = runs["plain"], runs["held"]
    assert set(plain) == {"primitives", "steps"} and len(plain_lines) == 4 and all(l.get("fit") for l in plain_lines)
    assert [l for l in lines if l.get("fit")] == plain_lines                      # the same batches, the same losses
    for k, v in plain_ckpt["net"].items():
        assert torch.equal(v, ckpt["net"][k]), k
    assert plain_ckpt["optimizer"]["param_groups"] == ckpt["optimizer"]["param_groups"]
    for i, s in plain_ckpt["optimizer"]["state"].items():
        assert all(torch.equal(torch.as_tensor(v), torch.as_tensor(ckpt["optimizer"]["state"][i][k])) for k, v in s.items()), i
    validate = [l for l in lines if l.get("validate")]
    assert [(l["primitive"], l["step"]) for l in validate] == [("fling", 0), ("fling", 2), ("fling", 4)]
    assert [bool(l.get("validate")) for l in lines] == [True, False, False, True, False, False, True]
    keys = {"n_maps", "labels", "regret", "chosen_rank", "top1", "spearman", "maps_with_spearman", "pairs", "concordant",
            "pair_accuracy", "map_pair_accuracy", "mse"}
    assert all(set(l) == keys | {"validate", "primitive", "step"} and l["n_maps"] == 2 and l["labels"] == 10 and l["pairs"] > 0 for l in validate)
    strip = lambda l: {k: l[k] for k in keys}   # noqa: E731
    assert out["validation"] == {"fling": {"before": strip(validate[0]), "after": strip(validate[2])}}
    assert out["holdout_overlap"] == 1 and out["primitives"] == plain["primitives"]
    assert validate[0]["mse"] != validate[2]["mse"]                                # the weights moved in between


def test_command_line_refuses_score_maps_next_to_fit_maps_or_tasks(tmp_path):
    from flingbot_amd import train

    ap = train.build_parser()
    a = ap.parse_args(["--log", "x", "--score-maps", "a.npz", "b.npz", "--rank-min-gap", "0.05"])
    assert a.score_maps == ["a.npz", "b.npz"] and a.tasks is None and a.fit_maps is None and a.rank_min_gap == 0.05
    a = ap.parse_args(["--log", "x", "--fit-maps", "p.npz", "--holdout-maps", "h.npz", "--validate-every", "50"])
    assert a.holdout_maps == ["h.npz"] and a.validate_every == 50 and a.score_maps is None
    a = ap.parse_args(["--log", "x", "--fit-maps", "p.npz"])
    assert a.holdout_maps is None and a.validate_every == 0
    for bad in (["--score-maps", "a.npz", "--fit-maps", "p.npz"], ["--score-maps", "a.npz", "--tasks", "t.npz"],
                ["--tasks", "t.npz", "--holdout-maps", "h.npz"], ["--fit-maps", "p.npz", "--validate-every", "5"], []):
        with pytest.raises(SystemExit):
            ap.parse_args(["--log", "x"] + bad)
    with pytest.raises(SystemExit):
        train.main(["--log", str(tmp_path / "nothing"), "--score-maps", "a.npz"])   # no checkpoint: refused before a device is touched


# ---- header and library -------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_point():
    from flingbot_amd import build, sim as fsim

    with open(os.path.join(ROOT, "include", "flingsim.h")) as fh:
        header = fh.read()
    assert re.search(r"^int fs_map_score\(const float \*d_value, int value_stride, const int \*d_pix,", header, re.M)
    rule = header[header.index("csrc/fs_mapscore.hip"):header.index("int fs_map_score(")]
    for text in ("chosen_rank", "(double)y_i > (double)y_j + min_gap", "among equals the lowest k", "begin = clamp(off[b], 0, L)",
                 "min(end, begin + 4096)", "[0, value_stride)", "(double)Sab / sqrt((double)Saa * (double)Sbb)", "columns 1-3 = -1"):
        assert text in rule, text
    lib = fsim.load_library()
    assert lib.fs_map_score is not None and "fs_map_score" in lib._fs_symbols
    assert "fs_mapscore.hip" in build.LIB_SOURCES and os.path.exists(os.path.join(build.CSRC, "fs_mapscore.hip"))


def test_entry_point_refuses_bad_scalars_and_pointers():
    """FS_ERR_ARG before any HIP call: the pointers are host addresses that are never dereferenced."""
    from flingbot_amd import sim as fsim

    lib = fsim.load_library()
    buf = np.zeros(4096, np.float64)
    at = lambda k: C.c_void_p(buf.ctypes.data + 64 * k)   # noqa: E731
    ok = dict(value=at(0), stride=4096, pix=at(1), label=at(2), offsets=at(3), images=2, labels=4, gap=0.0, rows=at(4))
    call = lambda **a: lib.fs_map_score(a["value"], a["stride"], a["pix"], a["label"], a["offsets"], a["images"], a["labels"], a["gap"],   # noqa: E731
                                        a["rows"], None)
    cases = [dict(images=0), dict(images=-3), dict(labels=0), dict(labels=-1), dict(stride=0), dict(stride=-4096), dict(gap=-1e-9),
             dict(gap=NAN), dict(gap=INF), dict(gap=-INF)]
    pointers = ("value", "pix", "label", "offsets", "rows")
    cases += [{k: C.c_void_p(None)} for k in pointers]
    cases += [{k: C.c_void_p(buf.ctypes.data + 2)} for k in pointers]
    cases += [dict(rows=C.c_void_p(buf.ctypes.data + 4))]                          # 4- but not 8-byte aligned
    for kw in cases:
        assert call(**{**ok, **kw}) == -1, kw                                     # FS_ERR_ARG
        assert b"fs_map_score" in lib.fs_last_error(), kw
