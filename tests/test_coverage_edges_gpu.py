"""fs_k_coverage (behind fs_coverage) on the constructed particle sets of tests/coverage_cases.py: rounding ties, the flat-index
quirk, range ends, sample counts, zero extent, 1 to 16512 particles, NaN.  The expected areas are
tests/golden/coverage_edges_golden.npz, recorded from the reference's own get_current_covered_area; every comparison is
exact (float64 bits; isnan where the reference gives NaN)."""
import math
import os

import numpy as np
import pytest

import coverage_cases as cc
from scenarios import cloth_params

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coverage_edges_golden.npz")
FINITE = [c["name"] for c in cc.CASES if c["name"] not in cc.NAN_CASES]
_shared = {}


def _gold():
    if "gold" not in _shared:
        with np.load(GOLD) as z:
            _shared["gold"] = dict(zip(z["names"].tolist(), z["area"].tolist()))
            assert z["names"].tolist() == [c["name"] for c in cc.CASES]
    return _shared["gold"]


def _load(ctx, e, name):
    """The case as episode e: a grid cloth of exactly n particles, then the case's positions.  Never stepped."""
    pos = cc.BY_NAME[name]["pos"]
    ctx.set_scene(e, cloth_params(*cc.grid_for(pos.shape[0])))
    assert ctx.n_particles(e) == pos.shape[0]
    ctx.set_positions(e, pos.ravel())


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _first():
    """All finite cases as the episodes of one context, one coverage() call; shared by the tests below and left unchanged."""
    if "first" not in _shared:
        from flingbot_amd import sim as fsim

        ctx = fsim.FlingSim(n_envs=len(FINITE))
        for e, name in enumerate(FINITE):
            _load(ctx, e, name)
        _shared["first"] = (ctx, ctx.coverage())
    return _shared["first"]


def teardown_module(module):
    if "first" in _shared:
        _shared.pop("first")[0].close()


@pytest.mark.parametrize("name", FINITE)
def test_case_equals_the_reference(gpu_required, name):
    _, cov = _first()
    got, want = cov[FINITE.index(name)], _gold()[name]
    print(f"{name}: kernel {got!r} reference {want!r}")
    assert _bits(got) == _bits(want), (name, got, want)


def test_batch_order_and_empty_slots_do_not_matter(gpu_required):
    """The same cases in reversed order in a second context, with a scene-less slot in the middle and one at the end: every
    case gives what it gave in the first context (and so the reference's area), the empty slots 0.0."""
    from flingbot_amd import sim as fsim

    _, cov = _first()
    order = FINITE[::-1]
    mid = len(order) // 2
    slots = order[:mid] + [None] + order[mid:] + [None]
    ctx = fsim.FlingSim(n_envs=len(slots))
    for e, name in enumerate(slots):
        if name is not None:
            _load(ctx, e, name)
    got = ctx.coverage()
    for e, name in enumerate(slots):
        if name is None:
            assert _bits(got[e]) == _bits(0.0), e
        else:
            assert _bits(got[e]) == _bits(cov[FINITE.index(name)]) == _bits(_gold()[name]), (e, name, got[e])
    ctx.close()


def test_coverage_reads_only_and_repeats(gpu_required):
    ctx, cov = _first()
    before = [ctx.get_positions(e).view(np.uint32).copy() for e in range(len(FINITE))]
    again = ctx.coverage()
    assert np.array_equal(_bits(again), _bits(cov))
    for e, name in enumerate(FINITE):
        assert np.array_equal(before[e], cc.BY_NAME[name]["pos"].ravel().view(np.uint32)), name
        assert np.array_equal(ctx.get_positions(e).view(np.uint32), before[e]), name
    assert np.array_equal(_bits(ctx.coverage()), _bits(cov))


def test_slot_reuse_leaves_no_stale_count_or_extent(gpu_required):
    """One slot: 16512 particles, then 2, then 65, then 16512 again.  Each state gives the reference's area."""
    from flingbot_amd import sim as fsim

    ctx = fsim.FlingSim(n_envs=1)
    for name in ("sizes_16512", "sizes_2", "sizes_65", "two_coincident", "sizes_16512"):
        _load(ctx, 0, name)
        got = ctx.coverage()[0]
        assert _bits(got) == _bits(_gold()[name]), (name, got, _gold()[name])
    ctx.close()


def test_nan_coordinates_propagate_like_numpy(gpu_required):
    """np.min / np.max hand a NaN x or z on, and the reference's area is NaN; a NaN height changes nothing.  This context only
    ever sees set_scene, set_positions and coverage: NaN positions never reach the solver."""
    from flingbot_amd import sim as fsim

    gold = _gold()
    assert math.isnan(gold["nan_x"]) and math.isnan(gold["nan_z"]) and gold["nan_y_only"] == gold["nan_clean"]
    ctx = fsim.FlingSim(n_envs=len(cc.NAN_CASES))
    for e, name in enumerate(cc.NAN_CASES):
        _load(ctx, e, name)
    for _ in range(2):
        got = dict(zip(cc.NAN_CASES, ctx.coverage().tolist()))
        print("nan cases:", got)
        assert _bits(got["nan_clean"]) == _bits(gold["nan_clean"])
        assert _bits(got["nan_y_only"]) == _bits(gold["nan_clean"])
        assert math.isnan(got["nan_x"]), got["nan_x"]
        assert math.isnan(got["nan_z"]), got["nan_z"]
    ctx.close()
