"""The sort pass of fs_k_fused_grid64's half-stencil neighbour search (find mode 4) bit for bit against the CPU oracle.

The owner of a pair appends it unsorted to both particles' lists: the first four appends of a particle to a table in LDS (in
the w plane and the contact set's accumulators, both idle during the search), later ones to the list's column in global memory.
After a barrier every list is sorted and its column stored: up to four entries straight from LDS, 5 to FS_PAIR_SORT_BOUND = 16
through one batch of loads and a sorting network in registers, longer ones in place; a particle with more than 96 candidates is
searched again behind a second barrier, with queues that cover the planes the heads lay in.

The cases follow test_grid64_pair_search_gpu.py: after EVERY launch neighbour counts AND lists, shape candidates, positions
and velocities are compared with OracleSim, the grid-64 form is asserted to have run, and each case asserts its premise on
the oracle's lists.  The density ramp (list_sort_scenes.ramp) is the smallest shape that holds every path of the sort in one
episode: a pinned line of 128 particles whose spacing grows geometrically, so that list lengths from 0 to dozens occur side
by side -- in neighbouring lanes of the same wavefronts -- and the sheet's own free particles next to the line carry lists
above four, whose order the contact phase turns into position bits.
"""
import numpy as np
import pytest

import list_sort_scenes as L
import pair_search_scenes as S

pytestmark = pytest.mark.gpu

SORT_BOUND = 16  # FS_PAIR_SORT_BOUND (csrc/fs_pair_search.h)
RAMP = (8, L.HIGH, L.ramp(2e-4, 6e-3))
RAMP_TO_THE_CAP = (8, L.HIGH, L.ramp(5e-5, 4e-3))


def _ramp_premise(e, co, orc):
    lengths = set(co.tolist())
    assert set(range(24)) <= lengths, sorted(set(range(24)) - lengths)
    assert co.max() < 96 and orc.max_neighbor_list() < 96
    # every path of the sort, and both sides of each threshold between two of them
    assert {0, 1, 2, 4, 5, SORT_BOUND - 1, SORT_BOUND, SORT_BOUND + 1} <= lengths and co.max() > 2 * SORT_BOUND
    assert int((co[128:] > 4).sum()) >= 100  # free particles whose contacts are evaluated in list order


def test_ramp(gpu_required):
    """Lists of at most 4, of 5 to the bound and above the bound in one episode, every length from 0 to 23 among them."""
    L.run("ramp", [RAMP], _ramp_premise, calls=(1, 1, 1))


def test_ramp_to_the_cap(gpu_required):
    """The denser ramp: its dense end passes the cap of 96, so the one-sided search runs again in the same substep as the
    heads in LDS, over the planes they lay in."""
    def premise(e, co, orc):
        assert co.max() == 96 and orc.max_neighbor_list() > 96
        assert int(((co > 4) & (co <= SORT_BOUND)).sum()) >= 100 and int((co > SORT_BOUND).sum()) >= 100

    L.run("ramp to the cap", [RAMP_TO_THE_CAP], premise, calls=(1, 1, 1))


def test_ramp_carried_state(gpu_required):
    """The ramp as three frames in one launch and one more: heads, append counts and the planes they alias carry across
    substeps, frames and launches."""
    L.run("ramp, 3 + 1 frames", [RAMP], _ramp_premise, calls=(3, 1))


def test_batch(gpu_required):
    """Three episodes in one launch: the ramp, a fold with lists of one, and a flat cloth without lists."""
    def premise(e, co, orc):
        if e == 0:
            _ramp_premise(e, co, orc)
        elif e == 1:
            assert co.max() == 1 and int((co > 0).sum()) >= 408
        else:
            assert not co.any() and orc.max_neighbor_list() == 0

    L.run("batch of three", [RAMP, (16, L.LOW, S.fold(8)), (5, L.HIGH, S.nothing)], premise, calls=(1, 1, 1))


def test_quarter_fold_4mm(gpu_required):
    """The 4 mm quarter fold of test_grid64_pair_search_gpu.test_long_lists as an episode of its own: 64 x 64, a particle of
    the upper layer sees the 3 x 3 block below it in the first substep -- free particles with lists of nine, in the contact
    set, whose order shows in the position bits."""
    def premise(e, co, orc):
        assert orc.max_neighbor_list() == 9

    L.run("quarter fold, 4 mm", [(64, L.LOW, S.fold(16, lift=0.004))], premise, calls=(1, 1))
