"""The constructed steering cases (tests/steering_cases.py) without a GPU: the element-by-element float32 restatements equal
the vectorised numpy expressions that tests/fling_helpers.py (OracleBatch, OracleTaskSim) takes from the reference and equal
the same operations in float64; every case's precondition holds, so none passes vacuously; and every mistake the restatements
can be switched to make is noticed by the cases that name it."""
import math

import numpy as np
import pytest

import steering_cases as sc

F = np.float32
READ_ONLY = [c["name"] for c in sc.CASES if c["op"] != "stable"]
STABLE = [c["name"] for c in sc.CASES if c["op"] == "stable"]
# The float32 elementwise displacement of the seeded cloud against the correctly rounded float64 one, in float32 ulps.  The
# float32 expression rounds three differences, three squares, two sums and a square root; the test prints what it measures
# (0 ulp: the cloud's maximum is the same float32 in both precisions).
CLOUD_ULP_MARGIN = 1


def _same(a, b):
    """Equal as values (so +0.0 == -0.0), any NaN equal to any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _ulps(a, b):
    """Distance of two finite float32 of one sign, in units in the last place."""
    return abs(int(F(a).view(np.int32)) - int(F(b).view(np.int32)))


# ---- the vectorised expressions, as OracleBatch states them
def np_stats(pos, vel):
    with np.errstate(invalid="ignore"):
        return pos[:, 1].min(), pos[:, 1].max(), np.abs(vel.ravel()).max()


def np_probe(pos, mid, thr):
    positions = pos[:, :3]
    with np.errstate(invalid="ignore"):
        high_positions = positions[positions[:, 1] > thr, ...]
    single = bool((high_positions[:, 0] < 0).all() or (high_positions[:, 0] > 0).all())
    plist = [p for p in positions]
    plist.sort(key=lambda p: np.linalg.norm(p[[0, 2]] - mid))
    return single, plist[0]


def np_disp(pos, pre):
    with np.errstate(invalid="ignore"):
        return np.linalg.norm(np.abs(pos[:, :3] - pre[:, :3]), axis=1).max()


def expected(case, mut=()):
    """What the case's operation returns under the restatement: a tuple of numpy scalars / Python values."""
    if case["op"] == "stats":
        return sc.stats(case["pos"], case["vel"], mut)
    if case["op"] == "probe":
        single, idx = sc.probe(case["pos"], case["mid"], case["thr"], mut)
        return (single,) + tuple(case["pos"][idx, :3].view(np.uint32).tolist())     # the winner by its position bits
    if case["op"] == "disp":
        return (sc.displacement(case["pos"], case["pre"], mut),)
    return sc.stable(case["vel"], case["tol"], case["max_steps"], mut)


def _differs(a, b):
    return len(a) != len(b) or any(not _same(x, y) for x, y in zip(a, b))


# ---- the table
def test_table_covers_the_issue():
    assert sc.COUNTS == (1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1025) and sc.BIG == 16512
    assert sc.placements(1025) == [0, 63, 64, 255, 256, 511, 767, 1023, 1024] and sc.placements(2) == [0, 1]
    assert sc.placements(513) == [0, 63, 64, 255, 256, 511, 512] and sc.placements(256) == [0, 63, 64, 255]
    for n in sc.COUNTS:
        for at in sc.placements(n):
            for name in (f"stats_min_n{n}_at{at}", f"stats_max_n{n}_at{at}", f"disp_n{n}_at{at}"):
                assert sc.BY_NAME[name]["n"] == n and sc.BY_NAME[name]["at"] == at
    assert sc.BY_NAME[f"disp_n{sc.BIG}_at{sc.BIG - 1}"]["n"] == sc.BIG > 16384
    assert sum(c["n"] == sc.BIG for c in sc.CASES) == 1                  # only one large case
    for case in sc.CASES:
        assert sc.grid_for(case["n"])[0] * sc.grid_for(case["n"])[1] == case["n"]
        assert case["why"] and case["rule"] and case["op"] in ("stats", "probe", "disp", "stable")
        for k in ("pos", "vel", "pre"):
            assert k not in case or case[k].dtype == F
    for at in (0, 257, 512):
        for stem in ("stats_nan_height", "stats_nan_velocity", "disp_nan_snapshot"):
            c = sc.BY_NAME[f"{stem}_at{at}"]
            bad = np.argwhere(np.isnan(c["pre"] if stem.startswith("disp") else c["pos"] if "height" in stem else c["vel"]))
            assert c["n"] == 513 and bad.shape == (1, 2) and bad[0, 0] == at
    assert sorted(sc.BATCH_ORDER) == [0, 1, 2, 3] and all(k != e for k, e in enumerate(sc.BATCH_ORDER))
    assert [sc.BY_NAME[n]["n"] for n in sc.BATCH["probe"]] == list(sc.BATCH_SIZES) == [2, 257, 64, 1025]


# ---- readings agree
@pytest.mark.parametrize("name", [n for n in READ_ONLY if sc.BY_NAME[n]["op"] == "stats"])
def test_stats_restatement_equals_numpy_and_float64(name):
    c = sc.BY_NAME[name]
    got = sc.stats(c["pos"], c["vel"])
    assert all(type(x) is F for x in got)
    assert _same(got, np_stats(c["pos"], c["vel"])), (name, got)
    wide = np_stats(c["pos"].astype(np.float64), c["vel"].astype(np.float64))
    assert wide[0].dtype == np.float64 and _same(got, [F(x) for x in wide]) and _same([float(x) for x in got], wide), (name, got)


@pytest.mark.parametrize("name", [n for n in READ_ONLY if sc.BY_NAME[n]["op"] == "probe"])
def test_probe_restatement_equals_numpy_and_float64(name):
    c = sc.BY_NAME[name]
    single, idx = sc.probe(c["pos"], c["mid"], c["thr"])
    np_single, np_near = np_probe(c["pos"], c["mid"], c["thr"])
    assert single == np_single and np.array_equal(c["pos"][idx, :3].view(np.uint32), np_near.view(np.uint32)), (name, single, idx)
    # one winner under three readings of the distance (a tie is exact in all three: see the preconditions below)
    for reading in ("fused", "f64"):
        assert sc.probe(c["pos"], c["mid"], c["thr"], reading=reading) == (single, idx), (name, reading)
    assert idx == c["at"], (name, idx)


@pytest.mark.parametrize("name", [n for n in READ_ONLY if sc.BY_NAME[n]["op"] == "disp"])
def test_displacement_restatement_equals_numpy_and_float64(name):
    c = sc.BY_NAME[name]
    got = sc.displacement(c["pos"], c["pre"])
    assert type(got) is F and _same(got, np_disp(c["pos"], c["pre"])), (name, got)
    with np.errstate(invalid="ignore"):
        d = c["pos"][:, :3].astype(np.float64) - c["pre"][:, :3].astype(np.float64)
        wide = np.sqrt((d * d).sum(axis=1)).max()
    if "exact" in c:                                            # the float64 result is a float32: correctly rounded, exact
        assert float(got) == wide == c["exact"], (name, got, wide)
    elif math.isnan(wide):
        assert math.isnan(got), (name, got)
    else:
        ulps = _ulps(got, F(wide))
        print(f"{name}: float32 elementwise {got!r}, float64 {wide!r}: {ulps} ulp apart (margin {CLOUD_ULP_MARGIN})")
        assert name == "disp_cloud" and ulps <= CLOUD_ULP_MARGIN


@pytest.mark.parametrize("name", STABLE)
def test_stable_restatement_states_the_double_comparison(name):
    c = sc.BY_NAME[name]
    assert sc.stable(c["vel"], c["tol"], c["max_steps"]) == c["want"], name
    if c["max_steps"]:
        with np.errstate(invalid="ignore"):
            m = np.abs(c["vel"].ravel()).max()
        assert (float(m) < c["tol"]) == c["want"][0]                        # the expression of tests/fling_helpers.py
        assert (np.float64(m) < np.float64(c["tol"])) == c["want"][0]       # the reference under NumPy 1.x: in double


def test_the_tolerance_edge_is_one_value():
    """float32(0.01) lies below 1e-2; compared as float32 the two are equal.  The readings differ there and nowhere else."""
    t = sc.T32
    assert sc.TOL == 1e-2 and float(t) < sc.TOL and not (t < F(sc.TOL))
    edge = {n: np.abs(sc.BY_NAME[n]["vel"]).max() for n in ("stable_one_below", "stable_at_float32_tol", "stable_one_above")}
    assert edge["stable_at_float32_tol"] == t
    assert edge["stable_one_below"] == np.nextafter(t, F(0)) and edge["stable_one_above"] == np.nextafter(t, F(1))
    for name, m in edge.items():
        assert ((float(m) < sc.TOL) != bool(F(m) < F(sc.TOL))) == (name == "stable_at_float32_tol"), name


def test_set_particle_equals_the_whole_array_rewrite():
    """OracleTaskSim.set_particles (the reference's whole-array rewrite, environment/tasks.py:177-224) on the batch's sets."""
    for n, pid, p4 in zip(sc.SET_SIZES, sc.SET_PIDS, sc.SET_POS4):
        assert pid in (0, n - 1)
        pos, vel = sc.base(n)
        for zero in (True, False):
            want_p, want_v = pos.copy(), vel.copy()
            want_p[pid] = np.asarray(p4, F)
            if zero:
                want_v[pid] = 0
            got_p, got_v = sc.set_particle(pos, vel, pid, p4, zero)
            assert np.array_equal(got_p.view(np.uint32), want_p.view(np.uint32))
            assert np.array_equal(got_v.view(np.uint32), want_v.view(np.uint32))
            assert (vel[pid] != 0).any() and not np.array_equal(pos[pid], p4)       # the write is visible
    assert {0} < set(sc.SET_PIDS) and len(set(sc.SET_SIZES)) == 3


# ---- no case passes vacuously
@pytest.mark.parametrize("name", READ_ONLY + STABLE)
def test_preconditions(name):
    c = sc.BY_NAME[name]
    n, at = c["n"], c.get("at")
    if c["rule"] == "placement" or c["rule"] == "regrow":
        assert at in sc.placements(n) or (n == sc.BIG and at == n - 1)
        if c["op"] == "stats":
            y, a = c["pos"][:, 1].astype(np.float64), np.abs(c["vel"].astype(np.float64)).max(axis=1)
            decisive = int(y.argmin()) if "_min_" in name else int(y.argmax())
            assert decisive == at and (np.delete(y, at) != y[at]).all()
            assert int(a.argmax()) == at and (np.delete(a, at) < a[at]).all()
        else:
            d = np.linalg.norm(c["pos"][:, :3].astype(np.float64) - c["pre"][:, :3].astype(np.float64), axis=1)
            assert int(d.argmax()) == at and (np.delete(d, at) < d[at] / 10).all()
    if "beyond_256" in name:
        assert at is not None and np.flatnonzero(c["pos"][:, 1] > c["thr"]).max() >= 256
    if c["op"] == "probe":
        d64 = np.array(sc.distances(c["pos"], c["mid"], reading="f64"))
        if c["tie"]:                                            # exact in float64, and strictly nearer than everything else
            assert at == min(c["tie"]) and len(set(d64[list(c["tie"])].tolist())) == 1
            assert max(c["tie"]) >= 256 and (np.delete(d64, list(c["tie"])) > 2 * d64[at]).all()
            assert len({c["pos"][i, :3].tobytes() for i in c["tie"]}) == len(c["tie"])      # told apart by their positions
        else:
            assert (np.delete(d64, at) > 1.4 * d64[at]).all()   # no near-tie: the winner does not depend on the rounding
        high = np.flatnonzero(c["pos"][:, 1] > c["thr"])
        assert (c["pos"][high, 0] != 0).all() or "zero" in name
        if "threshold" in name:
            y = c["pos"][300, 1]
            assert {"on": y == c["thr"], "below": y == np.nextafter(c["thr"], F(0)), "above": y == np.nextafter(c["thr"], F(9))}[
                name.split("_")[1 if name.startswith("probe_on") else 2]]
        if "dissenter" in name:
            assert (np.sign(c["pos"][high, 0]) > 0).sum() == 1 and c["pos"][high.max(), 0] > 0 and high.max() >= 256
    if c["op"] == "stable" and at is not None and c["max_steps"]:
        a = np.abs(c["vel"])
        assert np.isnan(a[at]).any() or (a.max() == a[at].max() and (np.delete(a, at, 0) < a.max() / 2).all())


# ---- decoys bite
@pytest.mark.parametrize("name", [c["name"] for c in sc.CASES if c["decoy"]])
def test_named_decoys_change_the_expected_output(name):
    c = sc.BY_NAME[name]
    want = expected(c)
    for m in c["decoy"]:
        assert _differs(expected(c, (m,)), want), f"{name} would pass a kernel with the mistake {m}"


def _batch(op, mut=()):
    cases = [sc.BY_NAME[n] for n in sc.BATCH[op]]
    if op == "stats":
        return sc.batch(lambda c: sc.stats(c["pos"], c["vel"]), cases, sc.BATCH_ORDER, [()] * 4, mut)
    if op == "probe":
        rows = sc.batch(lambda c, mid, thr: (sc.probe(c["pos"], mid, thr), c), cases, sc.BATCH_ORDER,
                        [(cases[e]["mid"], cases[e]["thr"]) for e in sc.BATCH_ORDER], mut)
        return [(single,) + tuple(c["pos"][idx, :3].view(np.uint32).tolist()) for (single, idx), c in rows]
    return sc.batch(lambda c, pre: (sc.displacement(c["pos"], pre[:c["n"]]),) if pre.shape[0] >= c["n"] else (F(np.nan),),
                    cases, sc.BATCH_ORDER, [(cases[e]["pre"],) for e in sc.BATCH_ORDER], mut)


@pytest.mark.parametrize("op", ["stats", "probe", "disp"])
def test_batch_rows_are_the_episodes_alone_and_the_batch_decoys_bite(op):
    """Row k of one call over BATCH_ORDER is episode BATCH_ORDER[k] called alone.  With slot 0's parameters for every slot,
    or with the id list ignored, every row but (at most) slot 0's changes.  (A snapshot of fewer particles than the episode
    that is compared with it has no defined answer: NaN here, which differs like any other value.)"""
    rows = _batch(op)
    alone = [expected(sc.BY_NAME[sc.BATCH[op][e]]) for e in sc.BATCH_ORDER]
    assert all(not _differs(tuple(r), tuple(a)) for r, a in zip(rows, alone))
    assert all(_differs(tuple(rows[j]), tuple(rows[k])) for j in range(4) for k in range(j))      # four different answers
    for m in sc.BATCH_DECOYS:
        if (op, m) == ("stats", "other_slot_params"):
            continue                                            # cloth_stats has no per-slot parameter
        changed = [_differs(tuple(r), tuple(w)) for r, w in zip(_batch(op, (m,)), rows)]
        assert changed[1:] == [True] * 3 and (m == "other_slot_params" or changed[0]), (op, m, changed)


def test_every_mutation_is_caught_somewhere():
    named = {m for c in sc.CASES for m in c["decoy"]} | set(sc.BATCH_DECOYS)
    assert named == set(sc.MUTATIONS) - set(sc.EQUIVALENT_MUTATIONS)
    assert sc.EQUIVALENT_MUTATIONS == ("disp_abs_missing",)


@pytest.mark.parametrize("name", [n for n in READ_ONLY if sc.BY_NAME[n]["op"] == "disp" and sc.BY_NAME[n]["n"] <= 1025])
def test_displacement_without_abs_is_the_same_function(name):
    c = sc.BY_NAME[name]
    assert _same(sc.displacement(c["pos"], c["pre"], ("disp_abs_missing",)), sc.displacement(c["pos"], c["pre"]))
    with np.errstate(invalid="ignore"):
        assert _same(np.linalg.norm(c["pos"][:, :3] - c["pre"][:, :3], axis=1).max(), np_disp(c["pos"], c["pre"]))
