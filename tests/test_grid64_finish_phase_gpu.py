"""fs_k_fused_grid64's three phases -- spring, contact, finish -- bit for bit against the CPU oracle after EVERY frame.

An iteration parks every particle's spring sums (in the accumulator of its contact-set or overflow-queue slot, or in the
thread's registers), lets set and queue lanes add the particle contacts, and then finishes each particle once -- planes,
spheres, applyDeltas -- in the thread that owns it.  The cases walk through where a particle's sums can come from in the
finish phase and what the finish phase has to add to them, on the smallest cloths that do it; every case asserts its premise
from the neighbour counts and shape candidates of the oracle and of the kernel on every frame it relies on.

Fold distances as in test_grid64_natural_order_gpu.py: a layer laid FOLD_LIFT = 11 mm above another is inside the search
radius and the contact rest distance (both 11.25 mm) and stays there.  Counts below are the CPU oracle's over frames 1..4.
"""
import numpy as np
import pytest

from conftest import cloth_params

pytestmark = pytest.mark.gpu

SET_CAP, QUEUE_CAP, QUEUE_ROUND = 1024, 1536, 960
FOLD_LIFT = 0.011
LOW = (0.0, -0.005, 0.0)  # the sheet within reach of the ground plane's margin
SPHERE_BITS = 8           # get_last_shape_candidates: bit q = plane q, bit 8 + q = sphere q


def _check(ctx, e, orc, what):
    ph, po = ctx.get_positions(e), orc.get_positions()
    vh, vo = ctx.get_velocities(e), orc.get_velocities()
    assert np.isfinite(po).all(), what
    assert np.array_equal(ph.view(np.uint32), po.view(np.uint32)), \
        f"{what}: positions not bit-exact (max abs diff {np.abs(ph - po).max():.3e})"
    assert np.array_equal(vh.view(np.uint32), vo.view(np.uint32)), \
        f"{what}: velocities not bit-exact (max abs diff {np.abs(vh - vo).max():.3e})"


def _lists(ctx, e, orc):
    """(neighbour counts, shape candidates) of the frame's last substep, the same on both sides."""
    ch, _ = ctx.get_last_neighbors(e)
    co, _ = orc.get_last_neighbors()
    assert np.array_equal(ch, co), f"episode {e}: neighbour counts differ from the oracle"
    m = ctx.get_last_shape_candidates(e)
    assert np.array_equal(m, orc.get_last_shape_candidates()), f"episode {e}: shape candidates differ from the oracle"
    return ch, m


def _run(ctx, orcs, what, premise, calls=(1, 1, 1, 1)):
    """Four frames, in launches of calls[.] frames; premise and bits checked after every launch."""
    from flingbot_amd import sim as fsim

    frame = 0
    for k in calls:
        ctx.step(k)
        assert ctx.last_kernel_form() == fsim.FS_FORM_FUSED_GRID64, what
        frame += k
        for e, orc in enumerate(orcs):
            orc.step(k)
            ch, m = _lists(ctx, e, orc)
            premise(e, ch, m)
            _check(ctx, e, orc, f"{what}, episode {e}, frame {frame}")


def _episodes(edits, dimz, pos, spheres=None):
    """One episode per entry of `edits` (callables on the (n, 4) position array), on the HIP batch and on oracles;
    spheres[e] = callable on the edited positions returning [(radius, centre), ...], added to episode e on both."""
    from flingbot_amd import sim as fsim
    from oracle import OracleSim

    ctx = fsim.FlingSim(n_envs=len(edits), solver=fsim.FS_SOLVER_FUSED)
    orcs = [OracleSim() for _ in edits]
    p = cloth_params(64, dimz, pos=pos)
    starts = []
    for e, edit in enumerate(edits):
        orcs[e].set_scene(p)
        xs = orcs[e].get_positions().reshape(-1, 4).copy()
        edit(xs)
        starts.append(xs.copy())
        ctx.env(e).set_scene(p)
        for s_ in (ctx.env(e), orcs[e]):
            s_.set_positions(xs.ravel())
            s_.set_velocities(np.zeros(3 * xs.shape[0], np.float32))
            for radius, centre in (spheres[e](xs) if spheres and e in spheres else ()):
                s_.add_sphere(radius, list(centre), [1, 0, 0, 0])
    return ctx, orcs, starts


def _nothing(xs):
    pass


def _fold(rows, shift=0.0, then=None):
    """Rows 0..rows-1 laid flat onto rows 2 rows - 1..rows, FOLD_LIFT above them (shifted by `shift` in x)."""
    def edit(xs):
        g = xs.reshape(-1, 64, 4)
        for iz in range(rows):
            g[iz, :, 2] = g[2 * rows - 1 - iz, :, 2]
            g[iz, :, 1] = g[2 * rows - 1 - iz, :, 1] + FOLD_LIFT
            g[iz, :, 0] += shift
        if then is not None:
            then(xs)
    return edit


def test_nothing_listed_register_finish(gpu_required):
    """(a) 64 x 8, 10 cm above the ground: no particle has a contact candidate and none lists the plane, so every particle
    is finished from the registers with nothing to add."""
    ctx, orcs, _ = _episodes([_nothing], 8, (0.0, -0.1, 0.0))

    def premise(e, ch, m):
        assert not ch.any() and not m.any()

    try:
        _run(ctx, orcs, "64 x 8, nothing listed", premise)
    finally:
        ctx.close()


def test_plane_on_register_finished_particles(gpu_required):
    """(b) 64 x 16 on the ground: the plane listed for all 1024 particles, no contact candidates."""
    ctx, orcs, _ = _episodes([_nothing], 16, LOW)

    def premise(e, ch, m):
        assert not ch.any() and (m == 1).all()

    try:
        _run(ctx, orcs, "64 x 16 on the ground", premise)
    finally:
        ctx.close()


def _partly_filled_set(e, ch, m):
    k = int((ch > 0).sum())
    # at least one wave of set lanes, and at least one without a set entry; nothing in the queue
    assert 64 <= k <= SET_CAP - 64, f"episode {e}: {k} particles with candidates"


def test_partly_filled_set_small_cloth(gpu_required):
    """(c) 64 x 16, rows 0..7 folded onto rows 15..8: 408-512 particles with one candidate -- a partly filled contact set, an
    empty queue, waves whose threads hold no set entry."""
    ctx, orcs, _ = _episodes([_fold(8)], 16, LOW)

    def premise(e, ch, m):
        _partly_filled_set(e, ch, m)
        assert ch.max() == 1

    try:
        _run(ctx, orcs, "64 x 16, fold of 8 rows", premise)
    finally:
        ctx.close()


def test_partly_filled_set_full_cloth(gpu_required):
    """(d) 64 x 64, rows 0..8 folded onto rows 17..9: 540-736 particles with candidates in a cloth that fills every wave."""
    ctx, orcs, _ = _episodes([_fold(9)], 64, LOW)
    try:
        _run(ctx, orcs, "64 x 64, fold of 9 rows", _partly_filled_set)
    finally:
        ctx.close()


def _set_full_queue_one_round(e, ch, m):
    k = int((ch > 0).sum())
    assert SET_CAP < k <= SET_CAP + QUEUE_ROUND, f"episode {e}: {k} particles with candidates"
    assert ch.max() <= 16


def _quarter_fold(then=None):
    return _fold(16, shift=0.003125, then=then)


@pytest.mark.parametrize("calls", [(1, 1, 1, 1), (3, 1)], ids=["frame-by-frame", "three-frames-one-launch"])
def test_full_set_and_queue(gpu_required, calls):
    """(e), (f) 64 x 32, rows 0..15 folded onto rows 31..16 half a pitch aside: 1502-1658 particles with candidates, lists of
    up to 2 -- the set full, the queue at 478-634 entries (one round).  (f) steps three frames in one launch: the state the
    kernel carries across substeps and frames."""
    ctx, orcs, _ = _episodes([_quarter_fold()], 32, LOW)
    try:
        _run(ctx, orcs, "64 x 32, quarter fold", _set_full_queue_one_round, calls)
    finally:
        ctx.close()


def test_exact_path_counts_reach_set_and_queue(gpu_required):
    """(g) the quarter fold with a particle of inverse mass 0 inside the fold (episode 0), a coincident pair there (episode
    1) and both (episode 2): the waves around them take the exact spring path and park their own spring counts in set and
    queue accumulators; the pinned particle does not move."""
    PIN = 64 * 9 + 40

    def pin(xs):
        xs[PIN, 3] = 0.0

    def coincide(xs):
        xs[64 * 8 + 31, :3] = xs[64 * 8 + 30, :3]

    def both(xs):
        pin(xs)
        coincide(xs)

    ctx, orcs, starts = _episodes([_quarter_fold(pin), _quarter_fold(coincide), _quarter_fold(both)], 32, LOW)

    def premise(e, ch, m):
        _set_full_queue_one_round(e, ch, m)
        if e != 1:
            now = ctx.get_positions(e).reshape(-1, 4)[PIN]
            assert np.array_equal(now.view(np.uint32), starts[e][PIN].view(np.uint32)), f"episode {e}: the pinned particle moved"

    try:
        _run(ctx, orcs, "64 x 32, quarter fold, pinned / coincident", premise)
    finally:
        ctx.close()


def test_sphere_contacts_in_the_finish_phase(gpu_required):
    """(h) the 64 x 16 fold of (c) with a 2 cm sphere pressing 1 mm into the upper layer where the layers have parted (row
    6: after a frame rows 4..11 carry no contact candidates, a single layer as far as contacts go; episode 0), where they
    touch (row 1; episode 1), and both (episode 2): sphere candidates on particles finished from the registers and on
    particles finished from a set accumulator.  On the CPU oracle 103-274 particles without and 137-348 with contact
    candidates list a sphere, in every episode and frame."""
    def over(row, col):
        def centre(xs):
            q = xs.reshape(-1, 64, 4)[row, col]
            return (0.02, (float(q[0]), float(q[1]) + 0.019, float(q[2])))
        return centre

    single, fold = over(6, 8), over(1, 48)
    spheres = {0: lambda xs: [single(xs)], 1: lambda xs: [fold(xs)], 2: lambda xs: [single(xs), fold(xs)]}
    ctx, orcs, _ = _episodes([_fold(8)] * 3, 16, LOW, spheres=spheres)

    def premise(e, ch, m):
        _partly_filled_set(e, ch, m)
        listed = (m >> SPHERE_BITS) != 0
        without, with_ = int((listed & (ch == 0)).sum()), int((listed & (ch > 0)).sum())
        assert without > 0, f"episode {e}: no particle without contact candidates lists a sphere"
        assert with_ > 0, f"episode {e}: no particle with contact candidates lists a sphere"

    try:
        _run(ctx, orcs, "64 x 16, fold of 8 rows, spheres", premise)
    finally:
        ctx.close()
