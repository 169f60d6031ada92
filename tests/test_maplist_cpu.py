"""The listwise map term without a GPU: trainops.map_list_torch in float64 against the float64 restatement (maplist_reference.py) at
the GPU test's shapes and values, against finite differences, and at its minimum; MapListFunction on host tensors and its
refusals; optimize_maps / fit_maps / optimize / the command line with list_weight; and the fs_map_list_loss entry point's header
lines, export and argument checks.

Every output of the float64 torch statement is a double: it lies within maplist_reference.bound64(n, A) of the restatement."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import maplist_reference as lref
from test_grouploss_cpu import HostGroupSet, _toy_set
from test_mapset_cpu import _policy, files  # noqa: F401  (files: the module's fixture of two replay files)
from test_train_cpu import _policy as _group_policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, T = 0.5, 0.1
MIXED = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 4096]    # the wave, slot and cap boundaries in one batch
SMALL = [2, 3, 64, 65, 257]


def values(lengths, kind="replay", seed=0):
    """(pred, label, offsets) float32 / int64 of a layout.  'replay': labels in [-0.11, 0.21] on a grid of 0.01 (ties occur),
    predictions the labels plus N(0, 0.1); 'equal_labels' / 'equal_preds': one constant per batch; 'ties': the maximum of every
    image's labels AND predictions stands at two random indices; 'spread': labels and
    predictions of every image spread evenly over 10^4 T, in two different random orders."""
    offsets = lref.offsets_of(lengths)
    L = int(offsets[-1])
    rng = np.random.default_rng([seed, L, len(lengths)])
    label = (np.round(rng.uniform(-0.11, 0.21, L) / 0.01) * 0.01).astype(np.float32)
    pred = (label + rng.standard_normal(L) * 0.1).astype(np.float32)
    if kind == "equal_labels":
        label[:] = np.float32(0.07)
    elif kind == "equal_preds":
        pred[:] = np.float32(-0.3)
    elif kind in ("ties", "spread"):
        for b in range(len(lengths)):
            lo, hi = int(offsets[b]), int(offsets[b + 1])
            if hi - lo < 2:
                continue
            if kind == "ties":
                for v in (pred, label):
                    at = lo + rng.choice(hi - lo, 2, replace=False)
                    v[at] = v[lo:hi].max() + np.float32(0.05)
            else:
                ramp = np.linspace(0.0, 1e4 * T, hi - lo).astype(np.float32)
                label[lo:hi], pred[lo:hi] = rng.permutation(ramp), rng.permutation(ramp)
    elif kind != "replay":
        raise ValueError(kind)
    return pred, label, offsets


# name -> (lengths, kind, label temperature); every case runs in both normalisations
CASES = {"mixed": (MIXED, "replay", None),
         "mixed_ty": (MIXED, "replay", 0.04),
         "one_image": ([144], "replay", None),
         "300x5": ([5] * 300, "replay", None),
         "equal_labels": (SMALL, "equal_labels", None),
         "equal_preds": (SMALL, "equal_preds", None),
         "ties": (SMALL, "ties", None),
         "spread": (SMALL, "spread", None),
         "spread_ty": (SMALL, "spread", 0.25)}
_refs = {}


def reference(name, per_image, weight=W, scale=1.0):
    """The restatement of a case; its per-image part is computed once and shared (the GPU tests import this)."""
    if name not in _refs:
        lengths, kind, ty = CASES[name]
        pred, label, offsets = values(lengths, kind)
        _refs[name] = lref.image_terms(pred, label, offsets, T, ty)
    return lref.normalise(_refs[name], weight, per_image, scale)


def compare(name, ref, dpred, stats, table, bound_out, bound_table, bound_dpred):
    """Every output against the restatement: the statistics within bound_out, the table within bound_table, dpred within
    bound_dpred (each a function of (n, A)); the integer-valued ones exactly.  Prints and returns the largest |got - ref| / bound."""
    stats, table = np.asarray(stats, np.float64), np.asarray(table, np.float64)
    assert stats[2:5].tolist() == [ref["listed"], ref["labels"], ref["hits"]] and stats[7] == 0.0, name
    worst = 0.0
    for k, out in ((0, "term"), (1, "list"), (5, "chosen_mass"), (6, "best_mass")):
        value, n, A = ref[out]
        err, tol = abs(float(stats[k]) - value), float(bound_out(n, A))
        print(f"{name}: {out} {stats[k]:.17g} ref {value:.17g} err {err:.3e} bound {tol:.3e}")
        assert err <= tol, (name, out, err, tol)
        worst = max(worst, err / tol if tol else 0.0)
    for b, row in enumerate(ref["table"]):
        assert table[b, 2] == row["chosen"] and table[b, 3] == row["best"], (name, b, table[b], row["chosen"], row["best"])
        for k, out in enumerate(("D", "q_chosen")):
            value, n, A = row[out]
            err, tol = abs(float(table[b, k]) - value), float(bound_table(n, A))
            assert err <= tol, (name, b, out, err, tol)
            worst = max(worst, err / tol if tol else 0.0)
    value, n, A = ref["dpred"]
    owned = ~np.isnan(value)
    err, tol = np.abs(np.asarray(dpred, np.float64) - value)[owned], bound_dpred(n, A)[owned]
    ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), 0.0)
    print(f"{name}: dpred largest err / bound {ratio.max() if len(ratio) else 0.0:.3f}; stats and table {worst:.3f}")
    assert (err <= tol).all(), (name, "dpred", int(np.argmax(err - tol)), float(err.max()))
    return max(worst, float(ratio.max()) if len(ratio) else 0.0)


def _torch64(pred, label, offsets, ty, per_image, weight=W):
    from flingbot_amd import trainops

    p = torch.tensor(np.asarray(pred, np.float64), requires_grad=True)
    term, stats, table = trainops.map_list_torch(p, torch.tensor(np.asarray(label, np.float64)), offsets, weight, T, ty, per_image)
    (grad,) = torch.autograd.grad(term, p)
    assert term.item() == stats[0].item() and not stats.requires_grad and not table.requires_grad
    assert stats.dtype == table.dtype == torch.float64 and tuple(table.shape) == (len(offsets) - 1, 4)
    return grad.numpy(), stats.numpy(), table.numpy()


# ---- the torch statement in float64 against the restatement --------------------------------------------------------------------
@pytest.mark.parametrize("per_image", [False, True], ids=["label_mean", "image_mean"])
@pytest.mark.parametrize("name", list(CASES))
def test_torch_statement_in_float64_is_the_restatement(name, per_image):
    lengths, kind, ty = CASES[name]
    pred, label, offsets = values(lengths, kind)
    ref = reference(name, per_image)
    got = _torch64(pred, label, offsets, ty, per_image)
    assert all(np.isfinite(a).all() for a in got), name                     # the spread of 10^4 T included
    compare(f"{name} per_image={per_image}", ref, *got, lref.bound64, lref.bound64, lref.bound64)
    assert ref["listed"] == sum(k >= 2 for k in lengths) and ref["list"][0] >= 0.0
    if kind == "spread":
        assert min(float(r["ls"].min()) for r in _refs[name]["rows"] if r) < -9000.0   # the log-softmax reaches -10^4, finite
        assert any((r["q"] == 0.0).any() for r in _refs[name]["rows"] if r)            # and q underflows to exactly 0


def test_restatement_by_hand():
    """Two listed images and one that is not: softmax by hand."""
    pred, label = np.array([0.3, 0.1, 0.2, 0.5, 0.7, 0.9]), np.array([0.1, 0.0, 0.0, 0.2, 0.2, 0.0])
    out = lref.map_list_f64(pred, label, [0, 3, 5, 6], W, T, None, False, scale=2.0)

    def soft(v):
        e = np.exp(v / T)
        return e / e.sum()
    D = []
    for lo, hi in ((0, 3), (3, 5)):
        s, q = soft(pred[lo:hi]), soft(label[lo:hi])
        D.append(float((q * np.log(q / s)).sum()))
        assert np.abs(out["dpred"][0][lo:hi] - 2.0 * W * ((hi - lo) / 5) * (s - q) / T).max() < 1e-14
    assert (out["listed"], out["labels"], out["hits"]) == (2, 5, 1)           # image 0: arg-max 0 and 0; image 1: 1 against 0 (a tie)
    assert abs(out["list"][0] - (3 * D[0] + 2 * D[1]) / 5) < 1e-14 and abs(out["term"][0] - W * out["list"][0]) < 1e-15
    assert out["dpred"][0][5] == 0.0 and out["table"][2] == {"D": (0.0, 0, 0.0), "q_chosen": (0.0, 0, 0.0), "chosen": -1, "best": -1}
    assert [out["table"][b]["chosen"] for b in (0, 1)] == [0, 1] and [out["table"][b]["best"] for b in (0, 1)] == [0, 0]
    assert abs(out["best_mass"][0] - (soft(label[:3])[0] + 0.5) / 2) < 1e-15 and abs(out["chosen_mass"][0] - out["best_mass"][0]) < 1e-15
    image_mean = lref.map_list_f64(pred, label, [0, 3, 5, 6], W, T, None, True)
    assert abs(image_mean["list"][0] - (D[0] + D[1]) / 2) < 1e-14 and image_mean["coef"].tolist() == [0.5, 0.5, 0.0]
    assert lref.arg_max([np.nan, 1.0, np.nan, 1.0]) == 1 and lref.arg_max([np.nan, np.nan]) == 0


@pytest.mark.parametrize("per_image", [False, True], ids=["label_mean", "image_mean"])
def test_gradient_agrees_with_finite_differences(per_image):
    from flingbot_amd import trainops

    pred, label, offsets = values([3, 5, 1, 0, 2], seed=4)
    p = torch.tensor(pred.astype(np.float64), requires_grad=True)
    y = torch.tensor(label.astype(np.float64))
    for ty in (None, 0.07):
        assert torch.autograd.gradcheck(lambda v: trainops.map_list_torch(v, y, offsets, W, T, ty, per_image)[0], (p,))   # noqa: B023


@pytest.mark.parametrize("per_image", [False, True], ids=["label_mean", "image_mean"])
def test_with_equal_temperatures_the_term_vanishes_where_pred_minus_label_is_constant(per_image):
    """pred = label + a constant per image: list = 0 and a zero gradient, each within its bound -- the term does not pull
    against the regression."""
    lengths = [2, 3, 64, 1, 300]
    _, label, offsets = values(lengths, seed=6)
    label = label.astype(np.float64)
    shift = np.repeat(np.array([0.3, -1.0, 0.05, 2.0, -0.2]), lengths)
    pred = label + shift
    ref = lref.map_list_f64(pred, label, offsets, W, T, None, per_image)
    grad, stats, table = _torch64(pred, label, offsets, None, per_image)
    assert abs(stats[1]) <= lref.bound64(ref["list"][1], ref["list"][2]) and abs(stats[0]) <= lref.bound64(ref["term"][1], ref["term"][2])
    assert (np.abs(grad) <= lref.bound64(ref["dpred"][1], ref["dpred"][2])).all() and ref["dpred"][2].max() > 0.0
    assert stats[4] == ref["listed"] == 4 and stats[5] == stats[6]            # every choice is the best cell
    # and not with unequal temperatures
    assert _torch64(pred, label, offsets, 0.05, per_image)[1][1] > 1e-3


# ---- MapListFunction on host tensors ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_image", [False, True], ids=["label_mean", "image_mean"])
def test_map_list_function_on_the_host(per_image):
    from flingbot_amd import trainops

    pred, label, offsets = values([40, 1, 17, 0, 64], seed=2)
    ref = lref.map_list_f64(pred, label, offsets, W, T, 0.07, per_image, scale=3.5)
    before = trainops.MapListFunction.n_forward
    p = torch.tensor(pred, requires_grad=True)
    term, stats, table = trainops.MapListFunction.apply(p, torch.tensor(label), offsets, W, T, 0.07, per_image)
    assert trainops.MapListFunction.n_forward == before                         # (counts kernel calls)
    assert term.requires_grad and not stats.requires_grad and not table.requires_grad and term.dtype == torch.float32
    (3.5 * term).backward()
    # float32 torch ops: every output a float32 sum, and the gradient scaled once more
    compare("host", ref, p.grad.numpy(), stats.numpy(), table.numpy(), lref.bound32, lref.bound32, lambda n, A: lref.bound32(n + 1, A))
    term2, stats2, _ = trainops.MapListFunction.apply(torch.tensor(pred), torch.tensor(label), torch.from_numpy(offsets), W, T, 0.07, per_image)
    assert torch.equal(term2, term.detach()) and torch.equal(stats2, stats)


def test_map_list_function_refuses_bad_tables_and_scalars(monkeypatch):
    from flingbot_amd import sim as fsim, trainops

    monkeypatch.setattr(fsim, "load_library", lambda: pytest.fail("refused before anything touches the library"))
    z = torch.zeros(6)
    apply = lambda off, p=z, y=z, w=W, tp=T, ty=None: trainops.MapListFunction.apply(p, y, off, w, tp, ty, False)   # noqa: E731
    assert apply(np.array([0, 2, 6]))[0].item() == 0.0                          # equal predictions and labels: KL = 0
    for bad in ([1, 2, 6], [0, 4, 2, 6], [0, -1, 6], [0, 2, 5], [0, 2, 7], [0.0, 2.0, 6.0], [[0, 2, 6]], [6]):
        with pytest.raises(ValueError):
            apply(np.array(bad))
    big = torch.zeros(5000)
    with pytest.raises(ValueError, match="4096"):
        apply(np.array([0, 5000]), big, big)
    with pytest.raises(ValueError):
        apply(np.array([0, 2, 6]), z, torch.zeros(5))
    with pytest.raises(ValueError):
        apply(np.array([0, 2, 6]), z, z.double())
    nan, inf = float("nan"), float("inf")
    for kw in (dict(w=-0.1), dict(w=nan), dict(w=inf), dict(tp=0.0), dict(tp=-1.0), dict(tp=inf), dict(tp=nan), dict(tp=5e-324),
               dict(ty=0.0), dict(ty=-0.1), dict(ty=inf), dict(ty=nan), dict(ty="warm")):
        with pytest.raises(ValueError):
            apply(np.array([0, 2, 6]), **kw)
        with pytest.raises(ValueError):
            trainops.map_list_torch(z, z, np.array([0, 2, 6]), kw.get("w", W), kw.get("tp", T), kw.get("ty"))


# ---- header and library -------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    from flingbot_amd import build, sim as fsim

    with open(os.path.join(ROOT, "include", "flingsim.h")) as fh:
        header = fh.read()
    assert re.search(r"^int fs_map_list_loss\(", header, re.M)
    assert re.search(r"^size_t fs_map_list_work_bytes\(int images, int labels\);", header, re.M)
    assert "KL(q || s)" in header and "g_i = (s_i - q_i) / T_p" in header                       # the rule is stated
    lib = fsim.load_library()
    for name in ("fs_map_list_loss", "fs_map_list_work_bytes"):
        assert getattr(lib, name) is not None and name in lib._fs_symbols
    assert "fs_maplist.hip" in build.LIB_SOURCES
    assert lib.fs_map_list_work_bytes(0, 5) == lib.fs_map_list_work_bytes(5, 0) == lib.fs_map_list_work_bytes(-1, -1) == 0
    assert lib.fs_map_list_work_bytes(3, 1000) >= 8 * 1000 + 3 * 32
    assert lib.fs_map_list_work_bytes(1 << 20, (1 << 31) - 1) > 1 << 34                          # sized in size_t


def test_entry_point_refuses_bad_scalars_and_pointers():
    """FS_ERR_ARG before any HIP call: the pointers are host addresses that are never dereferenced, so nothing was launched."""
    from flingbot_amd import sim as fsim

    lib = fsim.load_library()
    buf = np.zeros(4096, np.float64)
    at = lambda k: C.c_void_p(buf.ctypes.data + 64 * k)   # noqa: E731
    ok = dict(pred=at(0), label=at(1), offsets=at(2), images=2, labels=4, w=0.5, tp=0.1, ty=0.2, per_image=0, s=1.0, dpred=at(3),
              stats=at(4), table=at(5), work=at(6))
    call = lambda **a: lib.fs_map_list_loss(a["pred"], a["label"], a["offsets"], a["images"], a["labels"], a["w"], a["tp"], a["ty"],   # noqa: E731
                                            a["per_image"], a["s"], a["dpred"], a["stats"], a["table"], a["work"], None)
    nan, inf = float("nan"), float("inf")
    cases = [dict(images=0), dict(images=-3), dict(labels=0), dict(labels=-1), dict(per_image=2), dict(per_image=-1), dict(w=-0.1),
             dict(w=nan), dict(w=inf), dict(w=1e300), dict(s=nan), dict(s=inf), dict(s=-inf), dict(s=1e300)]
    for name in ("tp", "ty"):
        cases += [{name: v} for v in (0.0, -0.1, nan, inf, 5e-324, 1e300)]
    pointers = ("pred", "label", "offsets", "dpred", "stats", "table", "work")
    cases += [{k: C.c_void_p(None)} for k in pointers]
    cases += [{k: C.c_void_p(buf.ctypes.data + 2)} for k in pointers]
    cases += [{k: C.c_void_p(buf.ctypes.data + 4)} for k in ("stats", "work")]                 # 4- but not 8-byte aligned
    for kw in cases:
        assert call(**{**ok, **kw}) == -1, kw                                   # FS_ERR_ARG
        assert b"fs_map_list_loss" in lib.fs_last_error(), kw
    assert not buf.any()


# ---- optimize_maps / fit_maps / optimize / the command line ------------------------------------------------------------------------
LIST_KEYS = {"list", "listed_images", "top1_hits", "chosen_mass", "best_mass"}
MAP_KEYS = {"loss", "images", "labels", "mse", "rank", "pairs", "concordant", "images_with_pairs", "map_pair_accuracy"}


def test_optimize_maps_with_the_list_term_on_a_host_policy(files):   # noqa: F811
    from flingbot_amd import train
    from flingbot_amd.replay import MapSet

    maps = MapSet(list(files), action_primitive="fling")
    got = []
    for extra in (dict(), dict(list_weight=0.5), dict(list_weight=0.5, list_temperature=0.2, label_temperature=0.05, per_image=True)):
        policy, opt = _policy()
        policy.train()
        rows = []
        losses = train.optimize_maps("fling", policy.value_nets["fling"], opt, maps, 3, 3, np.random.default_rng(0), rank_weight=0.5,
                                     map_loss=True, stats=rows, **extra)
        policy.eval()
        got.append((losses, rows, policy.value_nets["fling"].state_dict()))
    (plain, plain_rows, plain_state), (listed, rows, state), (_, other_rows, _) = got
    assert set(plain_rows[0]) == MAP_KEYS and set(rows[0]) == set(other_rows[0]) == MAP_KEYS | LIST_KEYS
    first = rows[0]
    assert first["mse"] == pytest.approx(plain_rows[0]["mse"], rel=1e-6) and first["pairs"] == plain_rows[0]["pairs"]   # the same batch
    assert first["loss"] == listed[0] == pytest.approx(plain[0] + 0.5 * first["list"], rel=1e-5)
    rng = np.random.default_rng(0)
    for row in rows:
        _, offsets, _, _ = maps.draw_maps(3, rng)
        assert row["listed_images"] == int((np.diff(offsets) >= 2).sum()) and 0 <= row["top1_hits"] <= row["listed_images"]
        if row["listed_images"]:
            assert row["list"] > 0.0 and 0.0 < row["chosen_mass"] <= row["best_mass"] <= 1.0
        else:
            assert row["list"] == row["chosen_mass"] == row["best_mass"] == 0.0
    assert any(row["listed_images"] for row in rows)                            # no case passes vacuously
    assert any(not torch.equal(state[k], plain_state[k]) for k in state)        # the term reached the weights
    policy, opt = _policy()
    net = policy.value_nets["fling"]
    with pytest.raises(ValueError, match="map_loss"):
        train.optimize_maps("fling", net, opt, maps, 1, 3, np.random.default_rng(0), list_weight=0.5)
    for bad in (dict(list_weight=-1.0), dict(list_weight=float("nan")), dict(list_temperature=0.0), dict(label_temperature=-0.1),
                dict(label_temperature=float("inf"))):
        with pytest.raises(ValueError):
            train.optimize_maps("fling", net, opt, maps, 1, 3, np.random.default_rng(0), map_loss=True, **bad)
    assert int(net.steps) == 0
    for fn in (train.optimize_maps, train.fit_maps, train.optimize, train.run):
        sig = inspect.signature(fn).parameters
        assert (sig["list_weight"].default, sig["list_temperature"].default, sig["label_temperature"].default) == (0.0, 0.1, None)
    assert "guess" in train.optimize_maps.__doc__ and "guess" in train.optimize.__doc__ and "guess" in train.fit_maps.__doc__


def _same_files(a, b):
    from flingbot_amd import train

    assert sorted(os.listdir(a)) == sorted(os.listdir(b))
    assert open(os.path.join(a, train.TRAIN_LOG)).read() == open(os.path.join(b, train.TRAIN_LOG)).read()
    for name in (n for n in os.listdir(a) if n.endswith(".pth")):
        ca, cb = torch.load(os.path.join(a, name)), torch.load(os.path.join(b, name))
        assert set(ca["net"]) == set(cb["net"])
        for k, v in ca["net"].items():
            assert torch.equal(v, cb["net"][k]), k
        sa, sb = ca["optimizer"]["state"], cb["optimizer"]["state"]
        assert set(sa) == set(sb) and ca["optimizer"]["param_groups"] == cb["optimizer"]["param_groups"]
        for k in sa:
            assert all(torch.equal(torch.as_tensor(sa[k][f]), torch.as_tensor(sb[k][f])) for f in sa[k]), k


def test_fit_maps_with_list_weight_zero_writes_what_a_call_without_it_writes(files, tmp_path):   # noqa: F811
    from flingbot_amd import train

    base = {"fit", "primitive", "step", "loss", "images", "labels"}
    for name, kwargs in (("plain", dict()), ("map", dict(rank_weight=0.5, map_loss=True, holdout=list(files)))):
        dirs = []
        for tag, extra in (("absent", dict()), ("zero", dict(list_weight=0, list_temperature=0.3, label_temperature=0.7))):
            policy, opt = _policy()
            dirs.append(str(tmp_path / f"{name}_{tag}"))
            train.fit_maps(policy, opt, list(files), dirs[-1], 2, images_per_batch=3, seed=5, **kwargs, **extra)
        _same_files(*dirs)
        lines = [json.loads(l) for l in open(os.path.join(dirs[0], train.TRAIN_LOG))]
        assert not any(LIST_KEYS & set(l) or "list_kl" in l for l in lines)
        if name == "plain":
            assert all(set(l) == base for l in lines)


def test_fit_maps_with_the_list_term_logs_it_and_scores_the_held_out_maps(files, tmp_path):   # noqa: F811
    from flingbot_amd import train

    policy, opt = _policy()
    log = str(tmp_path / "listed")
    out = train.fit_maps(policy, opt, list(files), log, 2, images_per_batch=3, seed=5, map_loss=True, list_weight=0.5, holdout=list(files),
                         validate_every=1)
    lines = [json.loads(l) for l in open(os.path.join(log, train.TRAIN_LOG))]
    fits, scores = [l for l in lines if l.get("fit")], [l for l in lines if l.get("validate")]
    assert len(fits) == 2 and len(scores) == 3 and all(LIST_KEYS <= set(l) for l in fits)
    for s in scores + [out["validation"]["fling"]["before"], out["validation"]["fling"]["after"]]:
        assert s["list_kl"] >= 0.0 and 0.0 < s["chosen_mass"] <= s["best_mass"] <= 1.0
    # the same figures from score_maps, and none without the temperature
    again = train.score_maps(policy, list(files), list_temperature=0.1)["fling"]
    assert {k: again[k] for k in ("list_kl", "chosen_mass", "best_mass")} == {k: scores[-1][k] for k in ("list_kl", "chosen_mass", "best_mass")}
    split = train.score_maps(policy, list(files), images_per_batch=2, list_temperature=0.1)["fling"]
    assert split["list_kl"] == pytest.approx(again["list_kl"], rel=1e-5) and split["best_mass"] == pytest.approx(again["best_mass"], rel=1e-5)
    assert not {"list_kl", "chosen_mass", "best_mass"} & set(train.score_maps(policy, list(files))["fling"])
    with pytest.raises(ValueError, match="map_loss"):
        train.fit_maps(policy, opt, list(files), str(tmp_path / "bad"), 1, images_per_batch=3, list_weight=0.5)
    with pytest.raises(ValueError):
        train.score_maps(policy, list(files), list_temperature=0.0)


class NestedGroupSet(HostGroupSet):
    """sample_groups whose table passes check_bounds but whose groups are not contiguous rows: one group inside another."""

    def sample_groups(self, batch_size, rng):
        obs, mask, label, bounds = super().sample_groups(batch_size, rng)
        bounds = bounds.clone()
        bounds[:4] = torch.tensor([[0, 3], [1, 2], [0, 3], [3, 4]], dtype=bounds.dtype)
        return obs, mask, label, bounds


def test_optimize_with_the_list_term_over_lane_groups():
    from flingbot_amd import train, trainops

    assert train.group_offsets(np.int32([[0, 2], [0, 2], [2, 3], [3, 6], [3, 6], [3, 6]]), 6).tolist() == [0, 2, 3, 6]
    nested = np.int32([[0, 3], [1, 2], [0, 3], [3, 4]])
    assert trainops.check_bounds(nested, 4) is not None
    with pytest.raises(ValueError, match="contiguous"):
        train.group_offsets(nested, 4)
    raw = _toy_set(4, 4, seed=2)
    data = HostGroupSet(raw)
    for rank_weight in (0.0, 0.5):
        pol, plain = _group_policy(5), _group_policy(5)
        opt, opt_plain = train.make_optimizer(pol), train.make_optimizer(plain)
        pol.train(); plain.train()
        rows = []
        losses = train.optimize("fling", pol.value_nets["fling"], opt, data, 2, 8, np.random.default_rng(4), rank_weight=rank_weight,
                                list_weight=0.5, stats=rows)
        pol.eval()
        keys = {"loss", "mse"} | LIST_KEYS | ({"rank", "pairs", "concordant"} if rank_weight else set())
        assert len(losses) == 2 == len(rows) and np.isfinite(losses).all() and all(set(r) == keys for r in rows)
        rng = np.random.default_rng(4)
        for loss, row in zip(losses, rows):
            idx, bounds, _ = raw.draw_groups(8, rng)                             # grouped batches, also with rank_weight = 0
            offsets = train.group_offsets(bounds, 8)
            assert row["listed_images"] == int((np.diff(offsets) >= 2).sum()) > 0 and row["list"] > 0.0 and row["loss"] == loss
            own = row["mse"] + rank_weight * row.get("rank", 0.0)
            assert loss == pytest.approx(own + 0.5 * row["list"], rel=1e-5) and 0.0 < row["chosen_mass"] <= row["best_mass"] <= 1.0
        # the first update's list term, restated on the same batch and the initial weights
        idx, bounds, params = raw.draw_groups(8, np.random.default_rng(4))
        obs, mask, label = raw.item_host(idx, params)
        with torch.no_grad():
            pred = torch.masked_select(plain.value_nets["fling"](torch.from_numpy(obs)).squeeze(), torch.from_numpy(mask))
        ref = lref.map_list_f64(pred.numpy(), label, train.group_offsets(bounds, 8), 0.5, 0.1, None, False)
        assert rows[0]["list"] == pytest.approx(ref["list"][0], rel=1e-4) and rows[0]["top1_hits"] == ref["hits"]
    # a set without lanes: no listed group, the term is absent and the update is the regression's
    lone = HostGroupSet(_toy_set(16, 1, seed=3))
    ends = []
    for extra in (dict(list_weight=0.5), dict()):
        pol = _group_policy(5)
        opt = train.make_optimizer(pol)
        pol.train()
        rows = []
        losses = train.optimize("fling", pol.value_nets["fling"], opt, lone, 1, 8, np.random.default_rng(1), rank_weight=0.5, stats=rows, **extra)
        pol.eval()
        ends.append((losses, rows, pol.state_dict()))
    assert ends[0][1][0]["listed_images"] == 0 and ends[0][1][0]["list"] == 0.0 and ends[0][1][0]["chosen_mass"] is None
    assert ends[0][0] == ends[1][0] and all(torch.equal(v, ends[1][2][k]) for k, v in ends[0][2].items())
    # groups that are not contiguous rows are refused, before the update
    pol = _group_policy(5)
    opt = train.make_optimizer(pol)
    pol.train()
    with pytest.raises(ValueError, match="contiguous"):
        train.optimize("fling", pol.value_nets["fling"], opt, NestedGroupSet(raw), 1, 8, np.random.default_rng(4), list_weight=0.5)
    assert int(pol.value_nets["fling"].steps) == 0
    for bad in (dict(list_weight=-1.0), dict(list_temperature=0.0), dict(label_temperature=float("nan"))):
        with pytest.raises(ValueError):
            train.optimize("fling", pol.value_nets["fling"], opt, data, 1, 8, np.random.default_rng(0), **bad)


def test_command_line_takes_the_flags(capsys):
    from flingbot_amd import train

    ap = train.build_parser()
    a = ap.parse_args(["--log", "x", "--fit-maps", "p.npz"])
    assert a.list_weight == 0.0 and a.list_temperature is None and a.label_temperature is None and train._list_kwargs(a) == {}
    a = ap.parse_args(["--log", "x", "--fit-maps", "p.npz", "--map-loss", "--list-weight", "0.5"])
    assert train._list_kwargs(a) == dict(list_weight=0.5, list_temperature=0.1, label_temperature=None)
    a = ap.parse_args(["--log", "x", "--tasks", "t.npz", "--lookahead", "4", "--list-weight", "0.25", "--list-temperature", "0.2",
                       "--label-temperature", "0.05"])
    assert train._list_kwargs(a) == dict(list_weight=0.25, list_temperature=0.2, label_temperature=0.05)
    a = ap.parse_args(["--log", "x", "--score-maps", "p.npz", "--list-temperature", "0.2"])
    assert a.list_temperature == 0.2 and train._list_kwargs(a) == {}
    for argv in (["--log", "x", "--fit-maps", "p.npz", "--list-weight", "0.5"],                       # needs --map-loss
                 ["--log", "x", "--fit-maps", "p.npz", "--map-loss", "--list-weight", "-1"],
                 ["--log", "x", "--fit-maps", "p.npz", "--map-loss", "--list-weight", "0.5", "--list-temperature", "0"],
                 ["--log", "x", "--fit-maps", "p.npz", "--map-loss", "--list-weight", "0.5", "--label-temperature", "nan"],
                 ["--log", "x", "--fit-maps", "p.npz", "--label-temperature", "0.1"],                # belongs to the list term
                 ["--log", "x", "--score-maps", "p.npz", "--list-weight", "0.5"]):                   # no updates to weigh
        with pytest.raises(SystemExit):
            train.main(argv)                                                      # refused before anything is loaded
    assert "list" in capsys.readouterr().err
