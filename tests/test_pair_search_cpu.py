"""The half-stencil neighbour search of fs_k_fused_grid64 on the CPU: fs_host_pair_search runs the enumeration rule the kernel
includes (csrc/fs_pair_search.h: five runs per particle, every pair found by one owner and appended to both lists) on given
positions.  Checked here against an O(n^2) restatement of the oracle's rule (pair_search_scenes.brute_force) and against
OracleSim.get_last_neighbors, with the shipped 13 bucket bits and with 4 to 6 bits, where nearly every run holds particles of
foreign cells and runs overlap: every pair exactly once per endpoint, ascending, capped like the oracle.

The oracle searches the PREDICTED positions.  Its particles are pinned here (inverse mass 0, velocity 0), so the predicted
positions are the given ones (asserted), and its lists are lists of exactly the positions the host entry gets.
"""
import numpy as np
import pytest

import pair_search_scenes as S
from conftest import cloth_params

LOW = (0.0, -0.005, 0.0)
SCENES = {  # name -> (dimz, edit)
    "flat 64 x 5": (5, S.nothing),
    "flat 64 x 6": (6, S.nothing),
    "64 x 16, 8 rows folded": (16, S.fold(8)),
    "64 x 16 folded and translated (wrapped runs)": (16, S.fold(8, then=S.translate(*S.WRAP_SHIFT_CELLS))),
    "64 x 16, two layers in the same cells": (16, S.fold(8, lift=0.002)),
    "64 x 16, layers shifted by half a pitch": (16, S.fold(8, shift=S.PITCH / 2)),
    "64 x 16, same cells and half a pitch": (16, S.fold(8, lift=0.002, shift=S.PITCH / 2)),
    "64 x 32 folded in half, 4 mm apart (long lists)": (32, S.fold(16, lift=0.004)),
    "64 x 8, two rows in a pile": (8, S.pile),
}
_cache = {}


def _scene(name):
    """(positions, oracle counts, oracle lists, oracle's longest list, brute-force (counts, lists, longest), search radius),
    computed once."""
    if name not in _cache:
        from oracle import OracleSim

        dimz, edit = SCENES[name]
        orc = OracleSim()
        orc.set_scene(cloth_params(64, dimz, pos=LOW))
        xs = orc.get_positions().reshape(-1, 4).copy()
        edit(xs)
        xs[:, 3] = 0.0
        orc.set_positions(xs.ravel())
        orc.set_velocities(np.zeros(3 * xs.shape[0], np.float32))
        orc.step(1)
        assert np.array_equal(orc.get_positions().view(np.uint32), xs.ravel().view(np.uint32)), "pinned particles moved"
        par = orc.get_params()
        radius = np.float32(par[6]) + np.float32(par[10])  # radius + particleCollisionMargin, as the solvers add them
        assert abs(float(radius) - S.RADIUS) < 1e-8
        co, lo = orc.get_last_neighbors()
        _cache[name] = (xs, co, lo, orc.max_neighbor_list(), S.brute_force(xs, radius), radius)
        for a in _cache[name][:3]:
            a.setflags(write=False)
    return _cache[name]


def _same(counts, lists, ref_counts, ref_lists, what):
    assert np.array_equal(counts, ref_counts), f"{what}: counts differ at {np.flatnonzero(counts != ref_counts)[:8]}"
    for i in np.flatnonzero(ref_counts):
        assert np.array_equal(lists[i, :counts[i]], ref_lists[i, :counts[i]]), f"{what}: list of particle {i} differs"


@pytest.mark.parametrize("name", list(SCENES))
def test_brute_force_restates_the_oracle(name):
    """The O(n^2) reference agrees with OracleSim.get_last_neighbors on every scene (counts, lists, longest list)."""
    xs, co, lo, longest, (cb, lb, longest_b), _ = _scene(name)
    _same(cb, lb, co, lo, name)
    assert longest_b == longest


@pytest.mark.parametrize("bits", [13, 4, 5, 6])
@pytest.mark.parametrize("name", list(SCENES))
def test_half_stencil_lists_every_pair_once_per_endpoint(name, bits):
    from flingbot_amd.sim import host_pair_search

    xs, co, lo, longest, _, radius = _scene(name)
    counts, lists, facts = host_pair_search(xs, radius, bucket_bits=bits, ncap=96, dimx=64)
    what = f"{name}, {bits} bucket bits"
    assert facts["longest"] == longest, what  # a pair listed twice, or missed, changes a length before truncation
    _same(counts, lists, co, lo, what)
    for i in range(xs.shape[0]):
        row = lists[i, :counts[i]]
        assert (np.diff(row) > 0).all(), f"{what}: list of particle {i} not strictly ascending"
        assert (lists[i, counts[i]:] == -1).all()
    if bits <= 6 and co.any():  # the premise of the small tables: foreign cells in the runs, taken out by the visit-row test
        assert facts["alias_hits"] > 0, what


def test_premises_of_the_scenes():
    from flingbot_amd.sim import host_pair_search

    for name in ("flat 64 x 5", "flat 64 x 6"):
        assert not _scene(name)[1].any(), name
    co = _scene("64 x 16, 8 rows folded")[1]
    assert co.max() == 1 and int((co > 0).sum()) >= 408
    xs, radius = _scene("64 x 16 folded and translated (wrapped runs)")[0::5]
    assert host_pair_search(xs, radius, 13, 96, 64)[2]["wrapped_runs"] > 0
    # same cells: pairs of one cell, owned through the slot order
    xs, co = _scene("64 x 16, two layers in the same cells")[:2]
    cell = np.floor(xs[:, :3] * (np.float32(1.0) / radius)).astype(np.int64)
    lo = _scene("64 x 16, two layers in the same cells")[2]
    assert any((cell[lo[i, :co[i]]] == cell[i]).all(axis=1).any() for i in np.flatnonzero(co))
    assert _scene("64 x 32 folded in half, 4 mm apart (long lists)")[1].max() > 4
    xs, co, lo, longest, _, _ = _scene("64 x 8, two rows in a pile")
    assert longest > 96 and co.max() == 96
    assert np.unique(xs[:128, :3], axis=0).shape[0] == 128  # distinct, not coincident
    facts = host_pair_search(xs, radius, 13, 96, 64)[2]
    assert facts["over_cap"] >= 100 and facts["longest"] == longest


def test_without_the_stencil_filter_and_bad_arguments():
    """dimx = 0 keeps the grid neighbours: a flat cloth's interior particle lists its 8 neighbours at 6.25 mm pitch."""
    from flingbot_amd.sim import FlingSimError, host_pair_search

    xs, radius = _scene("flat 64 x 6")[0::5]
    counts, lists, _ = host_pair_search(xs, radius, 13, 96, 0)
    i = 64 * 2 + 10
    assert counts[i] == 8 and sorted(lists[i, :8]) == [i - 65, i - 64, i - 63, i - 1, i + 1, i + 63, i + 64, i + 65]
    with pytest.raises(FlingSimError):
        host_pair_search(xs, radius, bucket_bits=1)
    with pytest.raises(FlingSimError):
        host_pair_search(xs, 0.0)
