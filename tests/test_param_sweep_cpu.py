"""The parameter sweep on the oracle alone (no GPU): the condition under which tests/test_param_sweep_gpu.py means something.

A bit-for-bit comparison of a kernel with the oracle under a changed table proves that the kernel reads a parameter only if
the parameter changes the ORACLE's bits in that scene.  Here: orc_set_params writes what it says it writes, and in the scene
of tests/param_cases.py every slot of the ALL table -- one at a time -- and every EDGES table moves position or velocity bits.
"""
import functools

import numpy as np
import pytest

import param_cases as P
from oracle import OracleSim

SHAPES = [("16x16", 8), ("64x8", 6)]  # cloth, frames: the smallest shapes at which every slot is live
MESH_SHAPES = [("deg16", 6), ("shirt", 6), ("16x16t", 6)]  # the other cloths of the GPU file, at its frame count
_TMP = []


@functools.lru_cache(maxsize=None)
def _run(kind, n_frames, table_items):
    orc = OracleSim()
    P.scene(orc, table=dict(table_items), **P.cloth(kind, _TMP[0]))
    P.frames(orc, n_frames)
    pos = orc.get_positions().reshape(-1, 4)
    assert np.isfinite(pos).all() and np.isfinite(orc.get_velocities()).all()
    return P.bits(orc), float(pos[:, 1].min()), orc.accel_clamps(), np.abs(orc.get_velocities()).reshape(-1, 3)


@pytest.fixture(autouse=True)
def _tmp_dir(tmp_path_factory):
    if not _TMP:
        _TMP.append(tmp_path_factory.mktemp("param_sweep"))


def _key(table):
    return tuple(sorted((k, float(v)) for k, v in table.items()))


def test_set_params_of_get_params_changes_nothing():
    """4a: set_params(get_params()) is a no-op -- the table reads back bit for bit and a run with the call, repeated before
    every frame, equals an untouched oracle."""
    a, b = OracleSim(), OracleSim()
    for o in (a, b):
        P.scene(o, 16, 16)
    t0 = a.get_params()
    for _ in range(8):
        a.set_params(a.get_params())
        P.frames(a, 1)
    P.frames(b, 8)
    assert np.array_equal(a.get_params().view(np.uint32), t0.view(np.uint32))
    assert np.array_equal(P.bits(a), P.bits(b))


def test_set_params_writes_refuses_and_ignores_the_documented_slots():
    """Every table of param_cases round-trips bit for bit; slots 19-21 and 30-31 are ignored; a changed slot 6, 10, 22 or 29 and
    an out-of-range count are refused and change nothing."""
    orc = OracleSim()
    P.scene(orc, 16, 16)
    t0 = orc.get_params()
    for name, table in [("ALL", P.ALL), ("ALL_SHARED", P.ALL_SHARED)] + [(k, v[0]) for k, v in P.EDGES.items()]:
        want = P.apply(orc, table)
        assert np.array_equal(orc.get_params().view(np.uint32), want.view(np.uint32)), name
        orc.set_params(t0)
        assert np.array_equal(orc.get_params().view(np.uint32), t0.view(np.uint32)), name
    t = t0.copy()
    t[[19, 20, 21, 30, 31]] = 0.25
    orc.set_params(t)
    assert np.array_equal(orc.get_params().view(np.uint32), t0.view(np.uint32))
    for slot, value in [(6, 0.01), (10, 0.001), (22, 2), (29, 0), (27, 0), (27, 97), (27, 3.5), (28, -1), (28, 25), (1, 0),
                        (1, 101), (0, -1), (0, 1001), (2, 0.0), (2, -0.01), (2, np.nan)]:
        t = t0.copy()
        t[slot] = value
        t[7] = 0.02  # a valid change next to the refused one: must not be applied either
        with pytest.raises(ValueError):
            orc.set_params(t)
        assert np.array_equal(orc.get_params().view(np.uint32), t0.view(np.uint32)), (slot, value)
    with pytest.raises(ValueError):
        orc.set_params(t0[:31])


@pytest.mark.parametrize("kind,n_frames", SHAPES + MESH_SHAPES)
def test_every_slot_of_the_all_table_is_live(kind, n_frames):
    """4b: under ALL, putting any single slot back to FlingBot's value changes position or velocity bits -- every slot by
    itself, the three components of the plane's normal included (the table then holds a normal that is not a unit vector:
    what is shown is that the step reads that term), and the normal as one.  No slot is exempt, on the two small grids and on
    every other cloth the GPU file steps (16 springs per particle, the shirt, tethers).  The scene's premises: the speed
    clamp binds, the acceleration clamp fires, particles sleep."""
    base, _, clamps, absv = _run(kind, n_frames, _key(P.ALL))
    speed = np.sqrt((absv.astype(np.float64) ** 2).sum(axis=1))
    assert clamps > 100 and abs(speed.max() - 0.45) < 1e-6 and int((speed == 0).sum()) > 1, (clamps, speed.max(), (speed == 0).sum())
    dead = []
    for drop in [(slot,) for slot in sorted(P.ALL)] + [P.PLANE]:
        reverted = {k: v for k, v in P.ALL.items() if k not in drop}
        if np.array_equal(_run(kind, n_frames, _key(reverted))[0], base):
            dead.append(drop)
    assert not dead, f"slots without effect on {kind}: {dead}"


def test_static_friction_branch_is_live():
    """4d: under ALL (static 0.9 > dynamic 0.3) the stick branch decides contacts: static := dynamic changes the bits -- the
    branch FlingBot's table proves dead (test_oracle_cpu.py::test_static_friction_branch_is_redundant)."""
    for kind, n_frames in SHAPES + MESH_SHAPES:
        base = _run(kind, n_frames, _key(P.ALL))[0]
        assert not np.array_equal(_run(kind, n_frames, _key({**P.ALL, 12: P.ALL[11]}))[0], base), kind


@pytest.mark.parametrize("name", [k for k, v in P.EDGES.items() if v[1] != "ramp"])
def test_edges_tables(name):
    """4c: every EDGES table stays finite and differs from FlingBot's table -- except the one that says it is an identity
    (a finite maxSpeed that is never reached: same bits); without shape candidates the sheet falls through the ground."""
    table, note = P.EDGES[name]
    for kind, n_frames in SHAPES:
        base, base_low, _, _ = _run(kind, n_frames, _key(P.DEFAULT))
        got, low, _, _ = _run(kind, n_frames, _key(table))
        assert np.array_equal(got, base) == (note == "same"), (name, kind)
        if note == "below_plane":
            assert low < 0.0 < base_low, (low, base_low)


@pytest.mark.parametrize("cap", P.LIST_CAPS)
def test_list_caps_under_the_ramp(cap):
    """4c, maxNeighbors: under the density ramp some list exceeds the cap before truncation, the capped counts reach the cap
    and no further, and the result differs from the uncapped run's."""
    free, capped = OracleSim(), OracleSim()
    P.ramp_start(free)
    P.ramp_start(capped, {27: P.F(cap)})
    for o in (free, capped):
        o.step(1)
    P.assert_capped(capped, free, cap)
    for o in (free, capped):
        o.step(2)
    assert np.isfinite(capped.get_positions()).all()
    assert not np.array_equal(P.bits(free), P.bits(capped)), cap
