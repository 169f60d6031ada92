"""The temperature sweep of the listwise map term without a GPU: trainops.map_list_sweep_torch in float64 against the term that
exists (map_list_torch), against central differences and against the direct restatement (mapsweep_reference.py);
trainops.fit_temperature at a known answer, on a noisy set with an interior minimum, at the bound and without a listed image; the
refusals of map_list_sweep and of the fs_map_list_sweep entry point; the command line; and fit_maps / score_maps /
optimize_maps with a fitted temperature on a host policy."""
import ctypes as C
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mapsweep_reference as sref
from test_maplist_cpu import MIXED, values
from test_mapset_cpu import TASKS, _cell, _image, _policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TY = 0.1
MODES = (False, True)
TEMPERATURES = [0.004, 0.02, 0.05, 0.1, 0.3, 1.0, 25.0]


def f64(a):
    return torch.tensor(np.asarray(a, np.float64))


def close(got, want, rel, floor=0.0):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool((np.abs(got - want) <= rel * np.abs(want) + floor).all())


def sweep64(pred, label, offsets, temperatures, per_image, ty=TY):
    from flingbot_amd import trainops

    out = trainops.map_list_sweep_torch(f64(pred), f64(label), offsets, temperatures, ty, per_image)
    assert all(t.dtype == torch.float64 and not t.requires_grad for t in out)
    S, G = len(temperatures), len(offsets) - 1
    assert tuple(out[0].shape) == (S, 8) and tuple(out[1].shape) == (G, S, 4) and tuple(out[2].shape) == (G, 4)
    return tuple(t.numpy() for t in out)


# ---- against the loss that exists --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_image", MODES, ids=["label_mean", "image_mean"])
def test_column_0_is_the_list_term_that_exists(per_image):
    """At every temperature curve[s, 0] is map_list_torch's `list` and rows[b, s, 0] its table's D_b, to 1e-12 (of the value, or
    of 1 where the value is smaller), in float64 on both sides."""
    from flingbot_amd import trainops

    pred, label, offsets = values(MIXED, "replay")
    curve, rows, images = sweep64(pred, label, offsets, TEMPERATURES, per_image)
    for s, t in enumerate(TEMPERATURES):
        _, stats, table = trainops.map_list_torch(f64(pred), f64(label), offsets, 1.0, t, TY, per_image)
        stats, table = stats.numpy(), table.numpy()
        print(f"T={t}: list {curve[s, 0]:.17g} against {stats[1]:.17g}; D_b apart by at most {np.abs(rows[:, s, 0] - table[:, 0]).max():.3e}")
        assert abs(curve[s, 0] - stats[1]) <= 1e-12 * max(1.0, abs(stats[1]))
        assert (np.abs(rows[:, s, 0] - table[:, 0]) <= 1e-12 * np.maximum(1.0, np.abs(table[:, 0]))).all()
        assert curve[s, 6] == stats[2] and curve[s, 7] == stats[3]
    lengths = np.diff(offsets)
    assert images[:, 0].tolist() == [float(k) if k >= 2 else 0.0 for k in lengths]
    assert not rows[lengths < 2].any() and not images[lengths < 2].any()


@pytest.mark.parametrize("per_image", MODES, ids=["label_mean", "image_mean"])
def test_torch_statement_is_the_direct_restatement(per_image):
    """All three outputs against mapsweep_reference (every quantity from its definition, nothing factored), over temperatures
    from 1e-4 to 1e4: 1e-9 of the value plus 1e-12, the GPU test's bound."""
    pred, label, offsets = values(MIXED, "replay")
    temperatures = np.exp(np.linspace(np.log(1e-4), np.log(1e4), 17))
    got = sweep64(pred, label, offsets, temperatures, per_image)
    want = sref.map_list_sweep_f64(pred, label, offsets, temperatures, TY, per_image)
    for name, a, b in zip(("curve", "rows", "images"), got, want):
        assert np.isfinite(a).all(), name
        print(name, "largest |got - ref| / (1e-9 |ref| + 1e-12):", float((np.abs(a - b) / (1e-9 * np.abs(b) + 1e-12)).max()))
        assert close(a, b, 1e-9, 1e-12), name
    curve = got[0]
    assert (curve[:, 2] >= 0.0).all() and (got[1][:, :, 2] >= 0.0).all()                   # a variance
    assert (np.diff(curve[:, 5]) <= 1e-15).all() and curve[0, 5] > 0.99                     # colder: the draw is the arg-max
    assert (curve[:, 3] >= 0.0).all() and ((0.0 <= curve[:, 4:6]) & (curve[:, 4:6] <= 1.0)).all()


def test_sweep_by_hand():
    """One image of three labels at one temperature, every figure by hand; one image that is not listed."""
    p, y = np.array([0.3, 0.1, 0.2, 9.0]), np.array([0.1, 0.0, 0.3, 5.0])
    curve, rows, images = sweep64(p, y, [0, 3, 4], [0.2], False, ty=0.1)
    soft = lambda v: np.exp(v - v.max()) / np.exp(v - v.max()).sum()   # noqa: E731
    q, s = soft(y[:3] / 0.1), soft(p[:3] / 0.2)
    D = float((q * np.log(q / s)).sum())
    mean = float((s * p[:3]).sum())
    want = [D, mean - float((q * p[:3]).sum()), float((s * (p[:3] - mean) ** 2).sum()), float((s * y[:3]).sum())]
    assert close(rows[0, 0], want, 1e-13) and not rows[1].any() and not images[1].any()
    assert close(images[0], [3.0, 0.3, 0.1, float((q * p[:3]).sum())], 1e-14)
    assert close(curve[0], [D, want[1], want[2], 0.3 - want[3], s[2], s[0], 1.0, 3.0], 1e-13)


# ---- derivatives ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_image", MODES, ids=["label_mean", "image_mean"])
def test_columns_1_and_2_are_the_derivatives_in_beta(per_image):
    """Central differences in beta = 1 / T with a step of h = 1e-4 beta, in float64.  Column 1 against (f(b + h) - f(b - h)) / 2h of
    column 0, column 2 against the same difference of column 1: within 1e-6 of the value -- the scheme's truncation term is
    h^2 f''' / 6, some 1e-8 of the value here, two orders below.  Column 2 against the SECOND difference of column 0, (f(b + h) -
    2 f(b) + f(b - h)) / h^2, has the same truncation but divides the rounding of f by h^2, and f is rounded relative to its
    ADDENDS, not to itself: sum q lq and the log-sum are of the size of log K <= log 1000, beta sum q d of at most beta * 0.5 (the
    predictions of this set span less than 0.5).  So: 1e-6 of the value plus 4 * 2^-52 (log 1000 + 0.5 beta) / h^2.  The
    temperatures stay clear of the minimum near 0.135, where column 1 passes through 0 and nothing is relative to it."""
    pred, label, offsets = sref.noisy_set()
    assert np.ptp(pred) < 0.5
    for t in (0.02, 0.05, 0.3, 1.0):
        beta = 1.0 / t
        h = 1e-4 * beta
        (lo, mid, hi), rows, _ = sweep64(pred, label, offsets, [1.0 / (beta - h), t, 1.0 / (beta + h)], per_image)
        first, second = (hi[0] - lo[0]) / (2 * h), (hi[1] - lo[1]) / (2 * h)
        twice = (hi[0] - 2.0 * mid[0] + lo[0]) / (h * h)
        print(f"T={t}: slope {mid[1]:.12g} fd {first:.12g}; curvature {mid[2]:.12g} fd of slope {second:.12g}, second fd {twice:.12g}")
        assert abs(first - mid[1]) <= 1e-6 * abs(mid[1]) and abs(second - mid[2]) <= 1e-6 * abs(mid[2])
        assert abs(twice - mid[2]) <= 1e-6 * abs(mid[2]) + 4 * 2.0 ** -52 * (np.log(1000.0) + 0.5 * beta) / (h * h)
        assert mid[2] > 0.0 and (rows[:, :, 2] >= 0.0).all()
        # per image: relative to the largest entry of the column (an image may sit at its own minimum)
        fd1, fd2 = (rows[:, 2, 0] - rows[:, 0, 0]) / (2 * h), (rows[:, 2, 1] - rows[:, 0, 1]) / (2 * h)
        assert np.abs(fd1 - rows[:, 1, 1]).max() <= 1e-6 * np.abs(rows[:, 1, 1]).max()
        assert np.abs(fd2 - rows[:, 1, 2]).max() <= 1e-6 * np.abs(rows[:, 1, 2]).max()


# ---- fit_temperature -----------------------------------------------------------------------------------------------------------
def _fit(pred, label, offsets, **kw):
    from flingbot_amd import trainops

    return trainops.fit_temperature(torch.from_numpy(np.asarray(pred)), torch.from_numpy(np.asarray(label)), offsets, TY, **kw)


@pytest.mark.parametrize("per_image", MODES, ids=["label_mean", "image_mean"])
def test_fit_finds_the_known_answer(per_image):
    """p = a y + c per image with a = 0.5: softmax(p / T) = softmax(y / T_y) exactly at T = a T_y = 0.05, where the term is 0."""
    pred, label, offsets = sref.affine_set(0.5)
    fit = _fit(pred, label, offsets, per_image=per_image)
    print({k: v for k, v in fit.items() if k != "first_curve"})
    assert abs(fit["temperature"] / 0.05 - 1.0) < 1e-4 and abs(fit["list"]) < 1e-12 and fit["at_bound"] is None
    assert fit["sweeps"] == 6 == len(fit["chosen"]) and len(fit["first_curve"]) == 33
    first = fit["first_curve"]
    assert first[0]["temperature"] == 1e-3 and first[-1]["temperature"] == 1e2
    assert set(first[0]) == {"temperature", "list", "slope", "curvature", "expected_regret", "best_draw", "greedy_draw", "listed_images",
                             "listed_labels"}
    assert first[0]["listed_images"] == 5 and first[0]["listed_labels"] == 438
    k = fit["chosen"][0]
    assert first[k]["list"] == min(c["list"] for c in first) and first[k - 1]["slope"] > 0.0 > first[k + 1]["slope"]   # beta falls with k


def test_fit_on_the_noisy_set_is_interior_and_agrees_with_a_dense_scan():
    pred, label, offsets = sref.noisy_set()
    fit = _fit(pred, label, offsets)
    print({k: v for k, v in fit.items() if k != "first_curve"})
    assert fit["at_bound"] is None and fit["sweeps"] == 6
    dense, ratio = sref.dense_minimum(pred, label, offsets, TY, False, 0.05, 0.5, points=4097)
    assert ratio - 1.0 < 6e-4                                                    # the scan resolves what is asserted
    assert abs(fit["temperature"] / dense - 1.0) <= 1e-3 and abs(fit["temperature"] / 0.13541 - 1.0) <= 1e-3
    assert abs(fit["slope"]) < 1e-6 and fit["list"] <= sref.list_at(pred, label, offsets, dense, TY) + 1e-12
    # float64 inputs walk the same rounds (the host path computes in float64 either way)
    from flingbot_amd import trainops
    again = trainops.fit_temperature(f64(pred), f64(label), offsets, TY)
    assert again["chosen"] == fit["chosen"] and again["temperature"] == fit["temperature"]
    # a narrower range, fewer points and rounds
    short = _fit(pred, label, offsets, lo=0.05, hi=0.5, points=9, rounds=3)
    assert short["sweeps"] == 3 and abs(short["temperature"] / dense - 1.0) < 0.02


def test_fit_at_the_bound():
    """Predictions that rank the labels backwards: the term falls all the way to T = hi."""
    pred, label, offsets = sref.noisy_set(-1.0)
    fit = _fit(pred, label, offsets)
    assert fit["at_bound"] == "high" and fit["temperature"] == 1e2 and fit["slope"] > 0.0 and set(fit["chosen"]) == {32}
    low = _fit(*sref.noisy_set()[:3], lo=1.0, hi=50.0)
    assert low["at_bound"] == "low" and low["temperature"] == 1.0 and low["slope"] < 0.0 and set(low["chosen"]) == {0}


def test_a_set_without_a_listed_image():
    from flingbot_amd import trainops

    p, y, offsets = np.float32([0.3, -0.2, 7.0]), np.float32([0.1, 0.2, 0.0]), np.array([0, 1, 1, 2, 3])
    fit = _fit(p, y, offsets)
    assert fit["temperature"] is None and fit["list"] is None and fit["at_bound"] is None and fit["sweeps"] == 0
    curve, rows, images = trainops.map_list_sweep(torch.from_numpy(p), torch.from_numpy(y), offsets, [0.1, 1.0], TY)
    assert curve.dtype == torch.float64 and not curve.any() and not rows.any() and not images.any()


def test_non_finite_values_stay_in_their_image():
    pred, label, offsets = values([5, 40, 300, 2], "replay", seed=3)
    clean = sweep64(pred, label, offsets, [0.05, 0.5], False)
    for which, value in (("pred", np.nan), ("label", np.nan), ("pred", np.inf), ("label", -np.inf)):
        p, y = pred.astype(np.float64), label.astype(np.float64)
        (p if which == "pred" else y)[int(offsets[2]) + 17] = value
        curve, rows, images = sweep64(p, y, offsets, [0.05, 0.5], False)
        assert not np.isfinite(rows[2]).any() and not np.isfinite(curve[:, :6]).any(), (which, value)
        keep = [0, 1, 3]
        assert np.array_equal(rows[keep], clean[1][keep]) and np.array_equal(images[keep], clean[2][keep])
        assert curve[:, 6:].tolist() == clean[0][:, 6:].tolist()


# ---- map_list_sweep on the host, refusals ---------------------------------------------------------------------------------------------
def test_map_list_sweep_on_host_tensors_and_its_refusals(monkeypatch):
    from flingbot_amd import sim as fsim, trainops

    monkeypatch.setattr(fsim, "load_library", lambda: pytest.fail("refused before anything touches the library"))
    pred, label, offsets = values([40, 1, 17, 0, 64], seed=2)
    before = trainops.MapListSweep.n_forward
    got = trainops.map_list_sweep(torch.from_numpy(pred), torch.from_numpy(label), offsets, [0.05, 0.2], TY, True)
    want = sweep64(pred, label, offsets, [0.05, 0.2], True)
    assert trainops.MapListSweep.n_forward == before                               # (counts kernel calls)
    assert all(g.dtype == torch.float64 and np.array_equal(g.numpy(), w) for g, w in zip(got, want))
    z = torch.zeros(6)
    table = np.array([0, 2, 6])
    sweep = lambda off=table, p=z, y=z, t=(0.1, 1.0), ty=TY: trainops.map_list_sweep(p, y, off, t, ty)   # noqa: E731
    assert not sweep()[0][:, :3].any()                                            # equal predictions and labels: uniform against uniform
    for bad in ([1, 2, 6], [0, 4, 2, 6], [0, -1, 6], [0, 2, 5], [0, 2, 7], [0.0, 2.0, 6.0], [[0, 2, 6]], [6]):
        for fn in (sweep, lambda off: trainops.map_list_sweep_torch(z, z, off, [0.1], TY),   # noqa: E731
                   lambda off: trainops.fit_temperature(z, z, off, TY)):
            with pytest.raises(ValueError):
                fn(np.array(bad))
    big = torch.zeros(5000)
    with pytest.raises(ValueError, match="4096"):
        sweep(np.array([0, 5000]), big, big)
    for p, y in ((z, torch.zeros(5)), (z, z.double()), (z.long(), z.long()), (z.reshape(2, 3), z.reshape(2, 3))):
        with pytest.raises(ValueError):
            sweep(table, p, y)
    nan, inf = float("nan"), float("inf")
    scalars = (0.0, -1.0, inf, nan, 5e-324, 1e-300, 1e300, 1e-46, 1e39, "warm", None)
    for v in scalars:
        for kw in (dict(t=(0.1, v)), dict(ty=v)):
            with pytest.raises(ValueError):
                sweep(**kw)
            with pytest.raises(ValueError):
                trainops.map_list_sweep_torch(z, z, table, kw.get("t", (0.1,)), kw.get("ty", TY))
        with pytest.raises(ValueError):
            trainops.fit_temperature(z, z, table, v)
    for t in ((), [0.1] * 65, [[0.1, 0.2]], 0.1):
        with pytest.raises(ValueError):
            sweep(t=t)
    assert tuple(sweep(t=[0.1] * 64)[0].shape) == (64, 8) and tuple(sweep(t=np.array([0.1]))[1].shape) == (2, 1, 4)
    for kw in (dict(lo=0.0), dict(lo=1.0, hi=1.0), dict(lo=2.0, hi=1.0), dict(hi=inf), dict(hi=nan), dict(points=2), dict(points=65),
               dict(rounds=0), dict(ratio=0.0), dict(ratio=nan), dict(lo="cold")):
        with pytest.raises(ValueError):
            trainops.fit_temperature(z, z, table, TY, **kw)


# ---- header and library -------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    from flingbot_amd import build, sim as fsim

    with open(os.path.join(ROOT, "include", "flingsim.h")) as fh:
        header = fh.read()
    assert re.search(r"^int fs_map_list_sweep\(", header, re.M)
    assert re.search(r"^size_t fs_map_list_sweep_work_bytes\(int images, int labels, int n_temperatures\);", header, re.M)
    assert "E_s[p] - E_q[p]" in header and "Var_s[p]" in header and "expected_regret" in header          # the rule is stated
    lib = fsim.load_library()
    for name in ("fs_map_list_sweep", "fs_map_list_sweep_work_bytes"):
        assert getattr(lib, name) is not None and name in lib._fs_symbols
    assert "fs_mapsweep.hip" in build.LIB_SOURCES and os.path.exists(os.path.join(ROOT, "flingbot_amd", "csrc", "fs_mapsweep.hip"))
    work = lib.fs_map_list_sweep_work_bytes
    assert work(0, 5, 3) == work(5, 0, 3) == work(5, 5, 0) == work(5, 5, 65) == work(-1, -1, -1) == 0
    assert work(3, 1000, 33) >= 3 * 33 * 16 and work(1 << 24, (1 << 31) - 1, 64) >= 1 << 34              # sized in size_t


def test_entry_point_refuses_bad_scalars_and_pointers():
    """FS_ERR_ARG before any HIP call: the device pointers are host addresses that are never dereferenced, so nothing was launched;
    `temperatures` is a host array and is read."""
    from flingbot_amd import sim as fsim

    lib = fsim.load_library()
    buf = np.zeros(4096, np.float64)
    at = lambda k: C.c_void_p(buf.ctypes.data + 64 * k)   # noqa: E731
    temps = np.array([0.1, 1.0, 10.0])
    host = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    ok = dict(pred=at(0), label=at(1), offsets=at(2), images=2, labels=4, temps=host(temps), n=3, ty=0.2, per_image=0, curve=at(3),
              rows=at(4), table=at(5), work=at(6))
    call = lambda **a: lib.fs_map_list_sweep(a["pred"], a["label"], a["offsets"], a["images"], a["labels"], a["temps"], a["n"], a["ty"],   # noqa: E731
                                             a["per_image"], a["curve"], a["rows"], a["table"], a["work"], None)
    nan, inf = float("nan"), float("inf")
    cases = [dict(images=0), dict(images=-3), dict(labels=0), dict(labels=-1), dict(per_image=2), dict(per_image=-1), dict(n=0),
             dict(n=-1), dict(n=65)]
    keep = []
    for v in (0.0, -0.1, nan, inf, 5e-324, 1e-300, 1e300, 1e-46, 1e39):
        cases.append(dict(ty=v))
        for k in range(3):
            keep.append(np.array([v if j == k else 0.5 for j in range(3)]))
            cases.append(dict(temps=host(keep[-1])))
    pointers = ("pred", "label", "offsets", "curve", "rows", "table", "work")
    cases += [{k: C.c_void_p(None)} for k in pointers] + [dict(temps=C.POINTER(C.c_double)())]
    cases += [{k: C.c_void_p(buf.ctypes.data + 2)} for k in pointers]
    cases += [{k: C.c_void_p(buf.ctypes.data + 4)} for k in ("curve", "rows", "table", "work")]           # 4- but not 8-byte aligned
    cases += [dict(temps=C.cast(C.c_void_p(temps.ctypes.data + 4), C.POINTER(C.c_double)))]
    for kw in cases:
        assert call(**{**ok, **kw}) == -1, kw                                     # FS_ERR_ARG
        assert b"fs_map_list_sweep" in lib.fs_last_error(), kw
    assert not buf.any()


# ---- the command line ---------------------------------------------------------------------------------------------------------
def test_command_line(capsys):
    from flingbot_amd import train

    ap = train.build_parser()
    base = ["--log", "x", "--fit-maps", "p.npz", "--map-loss", "--list-weight", "0.5"]
    a = ap.parse_args(base + ["--list-temperature", "0.2"])
    assert a.list_temperature == 0.2 and isinstance(a.list_temperature, float) and a.refit_every == 100 and a.temperature_range is None
    assert not a.fit_temperature and train._list_kwargs(a) == dict(list_weight=0.5, list_temperature=0.2, label_temperature=None)
    a = ap.parse_args(base)
    assert a.list_temperature is None and train._list_kwargs(a) == dict(list_weight=0.5, list_temperature=0.1, label_temperature=None)
    a = ap.parse_args(base + ["--list-temperature", "fit", "--label-temperature", "0.1"])
    assert train._list_kwargs(a) == dict(list_weight=0.5, list_temperature="fit", label_temperature=0.1, refit_every=100)
    a = ap.parse_args(base + ["--list-temperature", "fit", "--label-temperature", "0.1", "--refit-every", "7", "--temperature-range", "0.01", "5"])
    assert train._list_kwargs(a) == dict(list_weight=0.5, list_temperature="fit", label_temperature=0.1, refit_every=7,
                                         temperature_range=(0.01, 5.0))
    a = ap.parse_args(["--log", "x", "--score-maps", "p.npz", "--fit-temperature", "--label-temperature", "0.1"])
    assert a.fit_temperature and a.list_temperature is None and a.label_temperature == 0.1
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--list-temperature", "warm"])
    capsys.readouterr()
    for argv, word in ((base + ["--list-temperature", "fit"], "--label-temperature"),                       # the target would move
                       (["--log", "x", "--tasks", "t.npz", "--list-weight", "0.5", "--list-temperature", "fit", "--label-temperature", "0.1"],
                        "--fit-maps"),
                       (["--log", "x", "--score-maps", "p.npz", "--list-temperature", "fit", "--label-temperature", "0.1"], "--fit-maps"),
                       (["--log", "x", "--fit-maps", "p.npz", "--map-loss", "--list-temperature", "fit", "--label-temperature", "0.1"],
                        "--list-weight"),
                       (["--log", "x", "--fit-maps", "p.npz", "--fit-temperature", "--label-temperature", "0.1"], "--score-maps"),
                       (["--log", "x", "--tasks", "t.npz", "--fit-temperature", "--label-temperature", "0.1"], "--score-maps"),
                       (["--log", "x", "--score-maps", "p.npz", "--fit-temperature"], "--label-temperature"),
                       (base + ["--list-temperature", "fit", "--label-temperature", "0.1", "--refit-every", "0"], "--refit-every"),
                       (base + ["--temperature-range", "0.01", "5"], "--temperature-range"),
                       (base + ["--list-temperature", "fit", "--label-temperature", "0.1", "--temperature-range", "5", "0.01"],
                        "--temperature-range")):
        with pytest.raises(SystemExit):
            train.main(argv)                                                      # refused before anything is loaded
        assert word in capsys.readouterr().err, argv


# ---- fit_maps / score_maps / optimize_maps on a host policy --------------------------------------------------------------------------
def tiny_files(directory):
    """One replay file of 4 maps with 6, 7, 8 and 9 measured cells, each on an image of its own (the GPU test trains on it too)."""
    from flingbot_amd import lookahead

    rng = np.random.default_rng(5)
    records = []
    for m, cells in enumerate((6, 7, 8, 9)):
        image = _image(40 + m)
        pixels = rng.choice(64 * 64, cells, replace=False)
        for r, pixel in enumerate(pixels):
            records.append(_cell(m % 2, m // 2, r, 1.0, 1.0 + float(rng.uniform(-0.3, 0.5)), (int(pixel) // 64, int(pixel) % 64), image))
    path = os.path.join(str(directory), "tiny.npz")
    assert lookahead.save_replay(path, dict(lane_records=records), TASKS) == 30
    return [path]


def _lines(log_dir):
    from flingbot_amd import train

    return [json.loads(l) for l in open(os.path.join(log_dir, train.TRAIN_LOG))]


def test_fit_maps_refits_and_leaves_a_numeric_temperature_alone(tmp_path):
    from flingbot_amd import train
    from flingbot_amd.replay import MapSet

    paths = tiny_files(tmp_path)
    maps = MapSet(paths, action_primitive="fling")
    assert len(maps) == 4 and np.diff(maps.offsets).tolist() == [6, 7, 8, 9]
    common = dict(images_per_batch=2, seed=5, map_loss=True, list_weight=0.5, label_temperature=0.1)
    policy, opt = _policy()
    log = str(tmp_path / "fitted")
    out = train.fit_maps(policy, opt, paths, log, 3, list_temperature="fit", refit_every=2, **common)
    lines = _lines(log)
    assert [("refit" in l, l["step"]) for l in lines] == [(True, 0), (False, 1), (False, 2), (True, 2), (False, 3)]
    refits = [l for l in lines if l.get("refit")]
    keys = ["refit", "primitive", "step", "list_temperature", "previous", "list_kl", "at_bound", "sweeps"]
    assert all(list(l) == keys and l["primitive"] == "fling" and l["sweeps"] >= 1 for l in refits)
    assert refits[0]["previous"] == 0.1 and refits[1]["previous"] == refits[0]["list_temperature"]
    for l in refits:                                                              # kept at a bound, taken inside
        assert l["list_temperature"] == l["previous"] if l["at_bound"] else 1e-3 < l["list_temperature"] < 1e2
    assert out["primitives"]["fling"]["list_temperature"] == refits[-1]["list_temperature"] and out["steps"] == 3
    assert not any("temperature" in name for name in torch.load(os.path.join(log, train.LATEST))["net"])
    # the first refit is the fit over all four maps under the initial weights
    fresh, _ = _policy()
    fit = train._fit_recorded_maps(fresh.value_nets["fling"], maps, 0.1, False, (1e-3, 1e2))
    assert fit["sweeps"] == refits[0]["sweeps"] and fit["list"] == refits[0]["list_kl"] and fit["at_bound"] == refits[0]["at_bound"]
    # a numeric temperature: the log's bytes with and without the new keyword arguments
    texts = []
    for tag, extra in (("absent", dict()), ("passed", dict(refit_every=2, temperature_range=(0.01, 5.0)))):
        policy, opt = _policy()
        log = str(tmp_path / tag)
        train.fit_maps(policy, opt, paths, log, 3, list_temperature=0.2, **common, **extra)
        texts.append(open(os.path.join(log, train.TRAIN_LOG), "rb").read())
    assert texts[0] == texts[1] and b"refit" not in texts[0] and len(texts[0].splitlines()) == 3
    # the fit with the holdout: validate lines at the temperature in force
    policy, opt = _policy()
    log = str(tmp_path / "held")
    out = train.fit_maps(policy, opt, paths, log, 3, list_temperature="fit", refit_every=2, holdout=paths, validate_every=2, **common)
    kinds = ["validate" if l.get("validate") else "refit" if l.get("refit") else "fit" for l in _lines(log)]
    assert kinds == ["validate", "refit", "fit", "fit", "validate", "refit", "fit", "validate"]
    assert "list_kl" in out["validation"]["fling"]["after"]
    # refusals
    policy, opt = _policy()
    for bad in (dict(label_temperature=None), dict(list_weight=0.0), dict(refit_every=0), dict(temperature_range=(1.0, 0.5)),
                dict(temperature_range=(0.0, 1.0)), dict(temperature_range=3.0)):
        with pytest.raises(ValueError):
            train.fit_maps(policy, opt, paths, str(tmp_path / "bad"), 1, list_temperature="fit", **{**common, **bad})
    with pytest.raises(ValueError):
        train.fit_maps(policy, opt, paths, str(tmp_path / "bad"), 1, list_temperature="warm", **common)
    assert int(policy.steps()) == 0


def test_optimize_maps_refits_across_calls_and_the_lane_path_refuses_fit(tmp_path):
    from flingbot_amd import train
    from flingbot_amd.replay import MapSet
    from test_grouploss_cpu import HostGroupSet, _toy_set

    maps = MapSet(tiny_files(tmp_path), action_primitive="fling")
    common = dict(map_loss=True, list_weight=0.5, list_temperature="fit", label_temperature=0.1, refit_every=2)
    policy, opt = _policy()
    net = policy.value_nets["fling"]
    policy.train()
    refits, state, rng = [], {}, np.random.default_rng(0)
    losses = train.optimize_maps("fling", net, opt, maps, 1, 2, rng, refits=refits, fit_state=state, **common)
    losses += train.optimize_maps("fling", net, opt, maps, 3, 2, rng, refits=refits, fit_state=state, **common)
    assert len(losses) == 4 and [r["step"] for r in refits] == [0, 2] and state["updates"] == 4 and net.training
    assert state["temperature"] == refits[-1]["list_temperature"]
    # one call of four updates: the same batches, the same refits, the same weights
    again, opt2 = _policy()
    again.train()
    refits2 = []
    losses2 = train.optimize_maps("fling", again.value_nets["fling"], opt2, maps, 4, 2, np.random.default_rng(0), refits=refits2, **common)
    assert losses2 == losses and refits2 == refits
    assert all(torch.equal(v, again.state_dict()[k]) for k, v in policy.state_dict().items())
    for bad in (dict(label_temperature=None), dict(list_weight=0.0), dict(refit_every=0), dict(temperature_range=(2.0, 1.0))):
        with pytest.raises(ValueError):
            train.optimize_maps("fling", net, opt, maps, 1, 2, rng, **{**common, **bad})
    # the lane path
    from test_train_cpu import _policy as _group_policy
    pol = _group_policy(5)
    with pytest.raises(ValueError, match="fit"):
        train.optimize("fling", pol.value_nets["fling"], train.make_optimizer(pol), HostGroupSet(_toy_set(4, 4, seed=2)), 1, 8,
                       np.random.default_rng(0), list_weight=0.5, list_temperature="fit", label_temperature=0.1)
    with pytest.raises(ValueError, match="fit"):
        train.run(pol, None, SimpleNamespace(record_experience=True), [dict()], str(tmp_path / "run"), 1, 1, 0, list_weight=0.5,
                  list_temperature="fit", label_temperature=0.1)
    assert not os.path.exists(str(tmp_path / "run"))                             # refused before anything is written
    assert "eval-mode BatchNorm" in train.optimize_maps.__doc__ and "eval-mode" in train.fit_maps.__doc__


def test_score_maps_fits_once_over_the_whole_set(tmp_path):
    from flingbot_amd import train, trainops

    paths = tiny_files(tmp_path)
    policy, _ = _policy()
    plain = train.score_maps(policy, paths, list_temperature=0.1, label_temperature=0.1)["fling"]
    assert "list_fit" not in plain
    calls = []
    real = trainops.fit_temperature
    trainops.fit_temperature = lambda *a, **kw: calls.append(a[2]) or real(*a, **kw)
    try:
        got = train.score_maps(policy, paths, images_per_batch=3, list_temperature=0.1, label_temperature=0.1, fit_temperature=True)["fling"]
    finally:
        trainops.fit_temperature = real
    assert len(calls) == 1 and calls[0].tolist() == [0, 6, 13, 21, 30]             # once, over all four maps
    fit = got.pop("list_fit")
    assert got == pytest.approx(plain, rel=1e-5)
    assert list(fit) == ["temperature", "list_kl", "at_bound", "slope", "sweeps", "curve"] and len(fit["curve"]) == 33
    assert all(list(c) == ["temperature", "list_kl", "expected_regret", "best_draw", "greedy_draw"] for c in fit["curve"])
    assert fit["curve"][0]["temperature"] == 1e-3 and fit["curve"][-1]["temperature"] == 1e2
    assert fit["list_kl"] <= min(c["list_kl"] for c in fit["curve"]) and fit["list_kl"] <= plain["list_kl"] * (1 + 1e-6)
    assert abs(fit["curve"][0]["expected_regret"] - plain["regret"]) < 1e-6          # the coldest draw is the arg-max: score_maps' regret
    at = train.score_maps(policy, paths, list_temperature=fit["temperature"], label_temperature=0.1)["fling"]
    assert at["list_kl"] == pytest.approx(fit["list_kl"], rel=1e-4)                # (float32 torch ops on the host)
    alone = train.score_maps(policy, paths, label_temperature=0.1, fit_temperature=True, temperature_range=(0.01, 10.0))["fling"]
    assert "list_kl" not in alone and alone["list_fit"]["curve"][0]["temperature"] == 0.01
    with pytest.raises(ValueError, match="label_temperature"):
        train.score_maps(policy, paths, fit_temperature=True)
    with pytest.raises(ValueError):
        train.score_maps(policy, paths, label_temperature=0.1, fit_temperature=True, temperature_range=(1.0, 1.0))
    json.dumps(alone)
