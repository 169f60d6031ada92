"""The constructed coverage cases (tests/coverage_cases.py) against tests/golden/coverage_edges_golden.npz, which was recorded
from the reference's own get_current_covered_area (tests/golden/make_golden.py coverage_edges): the table regenerates the
recorded particle sets, oracle/coverage.py and an independent scalar restatement equal the reference bit for bit on them, and
every mistake the restatement can be switched to make is noticed by the cases that name it.  No GPU needed."""
import math
import os

import numpy as np
import pytest

import coverage_cases as cc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coverage_edges_golden.npz")
NAMES = [c["name"] for c in cc.CASES]
I64_MIN = -2 ** 63


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def _same(a, b):
    """Bit for bit as float64, any NaN equal to any NaN."""
    a, b = float(a), float(b)
    return (math.isnan(a) and math.isnan(b)) or np.float64(a).tobytes() == np.float64(b).tobytes()


def scalar_area(pos, mut=()):
    """get_current_covered_area restated one particle and one cell at a time: float32 up to the slot quotients, Python ints and
    float64 from there.  `mut`: names from coverage_cases.MUTATIONS, each a mistake a kernel could make."""
    assert all(m in cc.MUTATIONS for m in mut)
    f32 = np.float32
    xs, zs = [f32(p[0]) for p in pos], [f32(p[2]) for p in pos]

    def extremes(vals):                     # np.min / np.max: a NaN anywhere is the result
        lo = hi = vals[0]
        for v in vals[1:]:
            if v != v or lo != lo:
                lo = hi = f32(np.nan)
            else:
                lo, hi = (v if v < lo else lo), (v if v > hi else hi)
        return lo, hi

    def slot(q):                            # q: a Python float holding the quotient exactly
        if "clip_before_round" in mut and q == q:
            q = min(max(q, 0.0), 100.0)
        if q != q or math.isinf(q):
            return I64_MIN                  # what numpy's cast of a non-finite float to int64 gave when the fixture was made
        if "roundf" in mut:
            return int(math.copysign(math.floor(abs(q) + 0.5), q))
        return round(q)                     # half to even, exact

    with np.errstate(all="ignore"):
        (mnx, mxx), (mnz, mxz) = extremes(xs), extremes(zs)
        span = [f32(mxx - mnx) / f32(100), f32(mxz - mnz) / f32(100)]
        assert all(type(s) is np.float32 for s in span)
        ranges = []
        for x, z in zip(xs, zs):
            r = []
            for o, s in ((f32(x - mnx), span[0]), (f32(z - mnz), span[1])):
                if "f64div" in mut:         # `(o - 0.00625) / s` with a double literal: the whole quotient in float64
                    ql, qh = (float(o) - 0.00625) / float(s) if s != 0 else math.copysign(math.inf, float(o) - 0.00625), \
                             (float(o) + 0.00625) / float(s) if s != 0 else math.inf
                elif "f64quot" in mut and s != 0:   # the float32 operands divided in float64
                    ql, qh = float(f32(o - cc.R32)) / float(s), float(f32(o + cc.R32)) / float(s)
                else:
                    ql, qh = float(f32(o - cc.R32) / s), float(f32(o + cc.R32) / s)
                lo, hi = max(slot(ql), 0), min(slot(qh), 100)
                r += [lo, hi + 1 if "inclusive_end" in mut else hi]
            ranges.append(r)
    nx = max(r[1] - r[0] for r in ranges) + 1
    nz = max(r[3] - r[2] for r in ranges) + 1
    if "swapN" in mut:
        nx, nz = nz, nx
    cells = set()
    for xl, xh, zl, zh in ranges:
        for kx in range(nx):
            ix = math.floor(kx * (xh - xl) / nx + xl)
            for kz in range(nz):
                iz = math.floor(kz * (zh - zl) / nz + zl)
                if "noalias" in mut:
                    ix, iz = min(ix, 99), min(iz, 99)
                idx = iz * 100 + ix if "swap_axes" in mut else ix * 100 + iz
                cells.add(min(max(idx, 0), 9999))
    if "f32_product" in mut:
        with np.errstate(all="ignore"):
            return float(len(cells)) * float(f32(span[0] * span[1]))
    return float(len(cells)) * float(span[0]) * float(span[1])


def test_table_regenerates_the_recorded_particle_sets(gold):
    assert os.path.getsize(GOLD) < 16 * 1024
    assert gold["names"].tolist() == NAMES
    assert gold["area"].dtype == np.float64 and gold["area"].shape == (len(NAMES),)
    for k, case in enumerate(cc.CASES):
        assert int(gold["n"][k]) == case["pos"].shape[0], case["name"]
        assert str(gold["sha256"][k]) == cc.sha256(case["pos"]), case["name"]


def test_table_covers_the_issue():
    ns = sorted({c["pos"].shape[0] for c in cc.CASES})
    assert set(cc.SIZES) <= set(ns) and ns[0] == 1 and cc.SIZES == (2, 63, 64, 65, 1023, 1024, 1025, 2049, 16512)
    assert {c["rule"] for c in cc.CASES} == {"rounding", "flat index", "range ends", "sample count", "zero extent",
                                             "particle counts", "nan"}
    for case in cc.CASES:
        p = case["pos"]
        assert cc.grid_for(p.shape[0])[0] * cc.grid_for(p.shape[0])[1] == p.shape[0]
        assert len(set(p[:, 1].tolist())) > 1 or p.shape[0] <= 2, case["name"]              # y varies
    assert any(c["pos"][:, 0].min() < -1 for c in cc.CASES) and any(c["pos"][:, 2].min() > 10 for c in cc.CASES)
    for n in cc.SIZES:                      # index 0 and index n - 1 own the bounding box
        p = cc.BY_NAME[f"sizes_{n}"]["pos"]
        assert p[0, 0] > p[1:, 0].max() and p[0, 2] < p[1:, 2].min()
        assert p[-1, 0] < p[:-1, 0].min() and p[-1, 2] > p[:-1, 2].max()
    clean = cc.BY_NAME["nan_clean"]["pos"]
    for name, col in (("nan_x", 0), ("nan_z", 2), ("nan_y_only", 1)):
        p = cc.BY_NAME[name]["pos"]
        bad = np.argwhere(np.isnan(p))
        assert bad.shape == (1, 2) and bad[0, 0] > 0 and bad[0, 1] == col
        assert np.array_equal(np.delete(p, bad[0, 0], 0), np.delete(clean, bad[0, 0], 0))


def test_expected_values_the_issue_states(gold):
    area = dict(zip(NAMES, gold["area"].tolist()))
    assert area["alias_x100"] == 0.0007999999642372135 and area["alias_z100"] == 0.0011999999463558203
    for name in ("one", "two_coincident", "line_x", "line_z"):
        assert _same(area[name], 0.0), name
    assert math.isnan(area["nan_x"]) and math.isnan(area["nan_z"]) and area["nan_y_only"] == area["nan_clean"] > 0
    p = cc.BY_NAME["tiny_cluster"]["pos"]
    sx, sz = (p[:, 0].max() - p[:, 0].min()) / np.float32(100), (p[:, 2].max() - p[:, 2].min()) / np.float32(100)
    assert area["tiny_cluster"] == 10000.0 * float(sx) * float(sz)
    assert area["ties_half_even"] != area["ties_one_ulp_below"] != area["ties_one_ulp_above"] != area["ties_half_even"]


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_the_reference(gold, name):
    from oracle.coverage import covered_area

    with np.errstate(divide="ignore", invalid="ignore"):
        got = covered_area(cc.BY_NAME[name]["pos"].ravel().copy())
    assert _same(got, gold["area"][NAMES.index(name)]), (name, got)


@pytest.mark.parametrize("name", NAMES)
def test_scalar_restatement_equals_the_reference(gold, name):
    got = scalar_area(cc.BY_NAME[name]["pos"])
    assert _same(got, gold["area"][NAMES.index(name)]), (name, got)


@pytest.mark.parametrize("name", [c["name"] for c in cc.CASES if c["decoy"]])
def test_named_decoys_change_the_area(gold, name):
    """Non-vacuity, per case: each mistake the case names gives another area than the reference's."""
    want = gold["area"][NAMES.index(name)]
    for m in cc.BY_NAME[name]["decoy"]:
        got = scalar_area(cc.BY_NAME[name]["pos"], (m,))
        assert not _same(got, want), f"{name} would pass a kernel with the mistake {m}"


def test_every_mutation_is_caught_somewhere():
    """Non-vacuity, over the table: every mistake in the list is named by a case (and so, by the test above, caught), except
    the one that is no mistake: clipping the quotient before rounding it gives the reference's area on every case."""
    named = {m for c in cc.CASES for m in c["decoy"]}
    assert named == set(cc.MUTATIONS) - set(cc.EQUIVALENT_MUTATIONS)
    assert cc.EQUIVALENT_MUTATIONS == ("clip_before_round",)


@pytest.mark.parametrize("name", [n for n in NAMES if not n.startswith("sizes_") or n in ("sizes_2", "sizes_65")])
def test_clip_before_round_is_the_same_function(gold, name):
    assert _same(scalar_area(cc.BY_NAME[name]["pos"], ("clip_before_round",)), gold["area"][NAMES.index(name)])
