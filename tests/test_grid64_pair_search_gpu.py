"""fs_k_fused_grid64's half-stencil neighbour search (find mode 4) bit for bit against the CPU oracle.

Every contact pair is found once, by its owner (csrc/fs_pair_search.h), appended unsorted to both particles' lists, and the
columns are sorted after a barrier; a particle with more than 96 candidates is searched again by the one-sided search, which
keeps the 96 smallest ids.  After EVERY launch the cases compare neighbour counts AND lists, shape candidates, positions and
velocities with OracleSim and assert that the grid-64 form ran.  Each case states its premise on the oracle's lists (or, for
the wrapped runs, through the host restatement of the search) and asserts it.

Fold distances as in test_grid64_finish_phase_gpu.py: a layer FOLD_LIFT = 11 mm above another is inside the search radius
(11.25 mm) with exactly one candidate per particle; 4 mm above, a particle sees the 3 x 3 block below it.
"""
import numpy as np
import pytest

import pair_search_scenes as S
from conftest import cloth_params

pytestmark = pytest.mark.gpu

LOW = (0.0, -0.005, 0.0)  # the sheet within reach of the ground plane's margin
HIGH = (0.0, -0.1, 0.0)


def _compare(ctx, e, orc, what):
    ch, lh = ctx.get_last_neighbors(e)
    co, lo = orc.get_last_neighbors()
    assert np.array_equal(ch, co), f"{what}: neighbour counts differ at {np.flatnonzero(ch != co)[:8]}"
    valid = np.arange(96)[None, :] < co[:, None]
    assert np.array_equal(lh[valid], lo[valid]), \
        f"{what}: neighbour lists differ for particles {np.flatnonzero(((lh != lo) & valid).any(axis=1))[:8]}"
    m = ctx.get_last_shape_candidates(e)
    assert np.array_equal(m, orc.get_last_shape_candidates()), f"{what}: shape candidates differ"
    ph, po = ctx.get_positions(e), orc.get_positions()
    vh, vo = ctx.get_velocities(e), orc.get_velocities()
    assert np.isfinite(po).all(), what
    assert np.array_equal(ph.view(np.uint32), po.view(np.uint32)), \
        f"{what}: positions not bit-exact (max abs diff {np.abs(ph - po).max():.3e})"
    assert np.array_equal(vh.view(np.uint32), vo.view(np.uint32)), \
        f"{what}: velocities not bit-exact (max abs diff {np.abs(vh - vo).max():.3e})"
    return co, m


def _run(what, dimz, pos, edits, premise, calls=(1, 1, 1, 1), start_premise=None):
    """Four frames, in launches of calls[.] frames, one episode per edit; premise(e, counts, masks, orc) on the oracle's
    side and everything compared after every launch."""
    from flingbot_amd import sim as fsim
    from oracle import OracleSim

    ctx = fsim.FlingSim(n_envs=len(edits), solver=fsim.FS_SOLVER_FUSED)
    try:
        orcs = [OracleSim() for _ in edits]
        p = cloth_params(64, dimz, pos=pos)
        for e, edit in enumerate(edits):
            orcs[e].set_scene(p)
            xs = orcs[e].get_positions().reshape(-1, 4).copy()
            edit(xs)
            if start_premise is not None:
                par = orcs[e].get_params()
                start_premise(e, xs, np.float32(par[6]) + np.float32(par[10]))
            ctx.env(e).set_scene(p)
            for s_ in (ctx.env(e), orcs[e]):
                s_.set_positions(xs.ravel())
                s_.set_velocities(np.zeros(3 * xs.shape[0], np.float32))
        frame = 0
        for k in calls:
            ctx.step(k)
            assert ctx.last_kernel_form() == fsim.FS_FORM_FUSED_GRID64, what
            frame += k
            for e, orc in enumerate(orcs):
                orc.step(k)
                co, m = _compare(ctx, e, orc, f"{what}, episode {e}, frame {frame}")
                premise(e, co, m, orc)
    finally:
        ctx.close()


@pytest.mark.parametrize("dimz", [5, 6])
def test_no_candidates(gpu_required, dimz):
    """The smallest cloths the kernel takes, flat: only the grid neighbours are within the radius, every list is empty."""
    def premise(e, co, m, orc):
        assert not co.any() and orc.max_neighbor_list() == 0

    _run(f"flat 64 x {dimz}", dimz, HIGH, [S.nothing], premise)


def test_one_candidate(gpu_required):
    """64 x 16, rows 0..7 folded onto rows 15..8: lists of length one, hundreds of them."""
    def premise(e, co, m, orc):
        assert co.max() == 1 and int((co > 0).sum()) >= 408

    _run("64 x 16, 8 rows folded", 16, LOW, [S.fold(8)], premise)


def test_carried_state(gpu_required):
    """64 x 32 folded in half, three frames in one launch and one more: the queue is in use, and the append counts and the
    planes they alias carry across substeps, frames and launches."""
    def premise(e, co, m, orc):
        assert int((co > 0).sum()) >= 1024

    _run("64 x 32 folded in half", 32, LOW, [S.fold(16)], premise, calls=(3, 1))


def test_long_lists(gpu_required):
    """The quarter fold of test_grid64_natural_order_gpu.py (64 x 64, 16 rows folded; one candidate per particle), and the
    same fold laid 4 mm above the lower layer, where a particle sees the 3 x 3 block below it in the first substep: columns
    longer than the four the sort pass handles in registers.  (The layers part within that frame; lists that stay long are
    test_over_the_cap's.)"""
    def premise(e, co, m, orc):
        if e == 0:
            assert int((co > 0).sum()) > 1024
        else:
            assert orc.max_neighbor_list() == 9

    _run("quarter fold", 64, LOW, [S.fold(16), S.fold(16, lift=0.004)], premise)


def test_over_the_cap(gpu_required):
    """Two rows of a 64 x 8 cloth drawn into 3 mm: more than 96 particles within the radius of one, so the appends pass the
    cap and the one-sided search has to supply the 96 smallest ids.  Episode 0 lets the pile go (lists of up to 13 after the
    first frame), episode 1 pins it, so that the capped lists are there to compare after every frame."""
    def premise(e, co, m, orc):
        assert orc.max_neighbor_list() > 96
        assert (co.max() == 96) if e == 1 else (int((co > 4).sum()) >= 1)

    _run("64 x 8, two rows in a pile", 8, LOW, [S.pile, S.pile_pinned], premise)


def _wrapped(e, xs, radius):
    from flingbot_amd.sim import host_pair_search

    if e == 0:
        assert host_pair_search(xs, radius, 13, 96, 64)[2]["wrapped_runs"] > 0


def test_wrapped_run(gpu_required):
    """The folded 64 x 16 cloth translated so that a row of its cells ends in the last buckets of the hash table: runs that
    continue at bucket 0 (the host restatement of the search reports them)."""
    def premise(e, co, m, orc):
        assert co.max() >= 1

    _run("64 x 16 folded, translated", 16, LOW, [S.fold(8, then=S.translate(*S.WRAP_SHIFT_CELLS))], premise,
         start_premise=_wrapped)


def test_batch(gpu_required):
    """Three episodes in one launch: wrapped runs, two layers sharing cells half a pitch apart, and the plain fold."""
    def premise(e, co, m, orc):
        assert (orc.max_neighbor_list() >= 2) if e == 1 else (co.max() == 1)

    edits = [S.fold(8, then=S.translate(*S.WRAP_SHIFT_CELLS)), S.fold(8, lift=0.002, shift=S.PITCH / 2), S.fold(8)]
    _run("batch of three", 16, LOW, edits, premise, start_premise=_wrapped)
