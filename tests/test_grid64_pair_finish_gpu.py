"""fs_k_fused_grid64 parks and finishes a trip's two particles -- P = row 2 w + 32 trip, Q = the row below it -- in one body,
their sums in registers named per trip: bit for bit against the CPU oracle after EVERY frame, four frames per case.

Wave w owns rows 2 w, 2 w + 1 (trip 0) and 2 w + 32, 2 w + 33 (trip 1); an even row is a P row, an odd row a Q row.  What
pairing can get wrong: a trip without its Q (odd heights) or without both rows, a trip whose particles hold contact-set
slots next to a trip finished from the registers (and the reverse), a pinned particle next to a partner that has to be
finished normally, a sphere that only one of the two particles lists or touches (the sphere ballot is taken once per trip),
and the state carried from iteration to iteration, substep to substep and frame to frame.  Every case asserts its premise
from the neighbour counts and shape candidates of the oracle and the kernel on every frame it relies on; the counts quoted
are the CPU oracle's over frames 1..4.

Fold distances as in test_grid64_finish_phase_gpu.py: a layer laid FOLD_LIFT = 11 mm above another is inside the search
radius and the contact rest distance (both 11.25 mm).  A fold of fewer than 6 rows parts within the first frame (the bend
springs across it are stretched too far) and lists nothing, so the folds at the ends of the 64 x 34 cloth are 8 rows deep.
"""
import numpy as np
import pytest

from conftest import cloth_params

pytestmark = pytest.mark.gpu

SET_CAP, QUEUE_ROUND = 1024, 960
FOLD_LIFT = 0.011
LOW = (0.0, -0.005, 0.0)  # the sheet within reach of the ground plane's margin
SPHERE_BITS = 8           # get_last_shape_candidates: bit q = plane q, bit 8 + q = sphere q
MIN_GRID64_ROWS = 5       # the host offers the grid-64 form from 5 rows on (fs_scene.cpp, build_grid64)
RADIUS, COLLISION_DISTANCE = 0.02, 0.01  # the test sphere; a particle closer than their sum to its centre is in contact


def _check(ctx, e, orc, what):
    ph, po = ctx.get_positions(e), orc.get_positions()
    vh, vo = ctx.get_velocities(e), orc.get_velocities()
    assert np.isfinite(po).all(), what
    assert np.array_equal(ph.view(np.uint32), po.view(np.uint32)), \
        f"{what}: positions not bit-exact (max abs diff {np.abs(ph - po).max():.3e})"
    assert np.array_equal(vh.view(np.uint32), vo.view(np.uint32)), \
        f"{what}: velocities not bit-exact (max abs diff {np.abs(vh - vo).max():.3e})"


def _lists(ctx, e, orc):
    """(neighbour counts, shape candidates) of the frame's last substep as (rows, 64) arrays, the same on both sides."""
    ch, _ = ctx.get_last_neighbors(e)
    co, _ = orc.get_last_neighbors()
    assert np.array_equal(ch, co), f"episode {e}: neighbour counts differ from the oracle"
    m = ctx.get_last_shape_candidates(e)
    assert np.array_equal(m, orc.get_last_shape_candidates()), f"episode {e}: shape candidates differ from the oracle"
    return np.asarray(ch).reshape(-1, 64), np.asarray(m).reshape(-1, 64)


def _run(ctx, orcs, what, premise, calls=(1, 1, 1, 1), grid64=True):
    """Four frames, in launches of calls[.] frames; premise(e, frame, counts, masks, positions before the launch) and bits
    checked after every launch."""
    from flingbot_amd import sim as fsim

    frame = 0
    before = [orc.get_positions().reshape(-1, 4).copy() for orc in orcs]
    for k in calls:
        ctx.step(k)
        assert (ctx.last_kernel_form() == fsim.FS_FORM_FUSED_GRID64) == grid64, what
        frame += k
        for e, orc in enumerate(orcs):
            orc.step(k)
            ch, m = _lists(ctx, e, orc)
            premise(e, frame, ch, m, before[e])
            _check(ctx, e, orc, f"{what}, episode {e}, frame {frame}")
            before[e] = orc.get_positions().reshape(-1, 4).copy()
    assert frame == 4


def _episodes(edits, dimz, pos=LOW, spheres=None):
    """One episode per entry of `edits` (callables on the (n, 4) position array), on the HIP batch and on oracles;
    spheres[e] = callable on the edited positions returning (radius, centre), added to episode e on both."""
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
            if spheres and e in spheres:
                radius, centre = spheres[e](xs)
                s_.add_sphere(radius, list(centre), [1, 0, 0, 0])
    return ctx, orcs, starts


def _nothing(xs):
    pass


def _fold(rows, then=None):
    """Rows 0..rows-1 laid flat onto rows 2 rows - 1..rows, FOLD_LIFT above them."""
    def edit(xs):
        g = xs.reshape(-1, 64, 4)
        for iz in range(rows):
            g[iz, :, 2] = g[2 * rows - 1 - iz, :, 2]
            g[iz, :, 1] = g[2 * rows - 1 - iz, :, 1] + FOLD_LIFT
        if then is not None:
            then(xs)
    return edit


def _fold_last(rows):
    """The mirror image at the other end: the last `rows` rows laid flat onto the `rows` rows before them."""
    def edit(xs):
        g = xs.reshape(-1, 64, 4)
        dimz = g.shape[0]
        for k in range(rows):
            src, dst = dimz - 1 - k, dimz - 2 * rows + k
            g[src, :, 2] = g[dst, :, 2]
            g[src, :, 1] = g[dst, :, 1] + FOLD_LIFT
    return edit


@pytest.mark.parametrize("dimz", [1, 2, 3, 5, 6, 33])
def test_sheet_on_the_ground_smallest_heights(gpu_required, dimz):
    """64 x 1, x 2, x 3, x 5, x 6 and x 33 on the ground: the plane listed for every particle, no contact candidates, so
    every particle is finished from the registers with the plane to add.  64 x 5 and 64 x 6 are the smallest cloths the
    grid-64 kernel takes: trip 0 of waves 0..2 alone, the last of them without and with its Q row.  In 64 x 33 the P row
    without a Q is trip 1 of wave 0 and every other wave's trip 1 is empty.  Cloths of fewer than 5 rows are not offered
    to this kernel by the host (asserted): 64 x 1, x 2 and x 3 pin the same sheets on the kernel that does run them."""
    ctx, orcs, _ = _episodes([_nothing], dimz)

    def premise(e, frame, ch, m, before):
        assert ch.shape[0] == dimz and not ch.any() and (m == 1).all()

    try:
        _run(ctx, orcs, f"64 x {dimz} on the ground", premise, grid64=dimz >= MIN_GRID64_ROWS)
    finally:
        ctx.close()


@pytest.mark.parametrize("end", ["last", "first"])
def test_slots_in_one_trip_registers_in_the_other(gpu_required, end):
    """64 x 34, 8 rows folded at one end.  "last" (rows 33..26 onto rows 18..25): P and Q of wave 0's trip 1 -- rows 32 and
    33 -- hold contact-set slots while its trip 0 -- rows 0 and 1 -- is finished from the registers; 408-512 particles with
    one candidate, row 32 on every frame, row 33 from frame 2 on.  "first" (rows 0..7 onto rows 15..8) is the reverse: rows
    0 and 1 hold slots (row 1 on every frame, row 0 from frame 2 on), rows 32 and 33 do not."""
    ctx, orcs, _ = _episodes([_fold_last(8) if end == "last" else _fold(8)], 34)
    slots, registers = ((32, 33), (0, 1)) if end == "last" else ((0, 1), (32, 33))
    seen = set()

    def premise(e, frame, ch, m, before):
        k = int((ch > 0).sum())
        assert 64 <= k <= SET_CAP - 64 and ch.max() == 1, f"frame {frame}: {k} particles with candidates"
        assert not ch[list(registers)].any(), f"frame {frame}: rows {registers} list candidates"
        assert ch[list(slots)].any(), f"frame {frame}: rows {slots} list no candidate"
        seen.update(r for r in slots if ch[r].any())

    try:
        _run(ctx, orcs, f"64 x 34, fold of the {end} 8 rows", premise)
        assert seen == set(slots), f"rows with slots over the four frames: {sorted(seen)}"
    finally:
        ctx.close()


def test_pinned_particle_in_a_p_row_a_q_row_and_both(gpu_required):
    """64 x 16, rows 0..7 folded onto rows 15..8 (408-524 particles with one candidate), with a particle of inverse mass 0
    inside the fold in a P row (row 2; episode 0), in a Q row (row 3; episode 1) and in both rows of one thread (episode
    2): the pinned particle's bits stay what they were and its partner in the trip is finished normally."""
    COL = 40

    def pin(*rows):
        def then(xs):
            for r in rows:
                xs[64 * r + COL, 3] = 0.0
        return then

    pinned = [(2,), (3,), (2, 3)]
    ctx, orcs, starts = _episodes([_fold(8, pin(*rows)) for rows in pinned], 16)

    def premise(e, frame, ch, m, before):
        k = int((ch > 0).sum())
        assert 64 <= k <= SET_CAP - 64 and ch.max() == 1, f"episode {e}: {k} particles with candidates"
        now = ctx.get_positions(e).reshape(-1, 4)
        for r in pinned[e]:
            i = 64 * r + COL
            assert np.array_equal(now[i].view(np.uint32), starts[e][i].view(np.uint32)), f"episode {e}: the pinned particle of row {r} moved"
            assert ch[r, COL] == 0  # (a pinned particle takes no slot)
        # the partner of a lone pinned particle, and the particles around, keep their candidates and slots
        assert ch[2:4, COL - 1:COL + 2].any()

    try:
        _run(ctx, orcs, "64 x 16, fold of 8 rows, pinned particles", premise)
    finally:
        ctx.close()


def test_sphere_touching_one_row_of_a_pair(gpu_required):
    """The 64 x 16 fold with a 2 cm sphere whose surface is 1 mm inside the contact distance of: the upper layer's edge row
    0 alone, from beside the folded sheet (a P row; episode 0); the lower layer's edge row 15 alone (a Q row; episode 1);
    rows 2 and 3 from above, centred between lanes 30 and 31 (a P and a Q row of wave 1, two lanes; episode 2).  The
    particles in contact at the start of every frame are those rows' and no others (episode 2: rows 2 and 3 on every
    frame, rows 4 and 5 as well from frame 3 on), while the sphere is LISTED for rows of both parities in every episode --
    rows 0..5 and 10..15 in episodes 0 and 1: lanes whose P lists it and whose Q does not, and the reverse, in one wave."""
    def beside(row):
        def centre(xs):
            q = xs.reshape(-1, 64, 4)[row, 30]
            return RADIUS, (float(q[0]), float(q[1]), float(q[2]) + 0.029)
        return centre

    def above(xs):
        g = xs.reshape(-1, 64, 4)
        a, b = g[2, 30], g[3, 31]
        return RADIUS, (0.5 * float(a[0] + b[0]), float(a[1]) + 0.029, 0.5 * float(a[2] + b[2]))

    spheres = {0: beside(0), 1: beside(15), 2: above}
    ctx, orcs, starts = _episodes([_fold(8)] * 3, 16, spheres=spheres)
    centres = [np.array(spheres[e](starts[e])[1], np.float64) for e in range(3)]
    allowed = [{0}, {15}, {2, 3, 4, 5}]

    def premise(e, frame, ch, m, before):
        listed = (m >> SPHERE_BITS) != 0
        assert listed[0::2].any() and listed[1::2].any()
        dist = np.linalg.norm(before[:, :3].astype(np.float64) - centres[e], axis=1).reshape(-1, 64)
        touched = dist < RADIUS + COLLISION_DISTANCE
        rows = {int(r) for r in np.flatnonzero(touched.any(axis=1))}
        assert rows and rows <= allowed[e], f"episode {e}, frame {frame}: rows in contact {sorted(rows)}"
        assert (listed | ~touched).all(), f"episode {e}, frame {frame}: a particle in contact does not list the sphere"
        if e == 2:  # one lane's P and another lane's Q of wave 1
            assert touched[2, 30] and touched[3, 31]
        with_, without = int((touched & (ch > 0)).sum()), int((touched & (ch == 0)).sum())
        assert with_ + without > 0

    try:
        _run(ctx, orcs, "64 x 16, fold of 8 rows, sphere on one row of a pair", premise)
    finally:
        ctx.close()


def test_half_fold_three_frames_in_one_launch_then_one(gpu_required):
    """64 x 32 folded in half (rows 0..15 onto rows 31..16) as step(3) in one launch, then step(1): 1536 and 1416
    particles with one candidate -- the set full, the queue at 512 and 392 entries -- rows 12..19 finished from the
    registers, and after the last frame 120 threads one of whose two particles has a slot and the other has not: what the
    kernel carries across iterations, substeps and frames, with set, queue and register particles side by side."""
    ctx, orcs, _ = _episodes([_fold(16)], 32)

    def premise(e, frame, ch, m, before):
        k = int((ch > 0).sum())
        assert SET_CAP < k <= SET_CAP + QUEUE_ROUND and ch.max() <= 16, f"frame {frame}: {k} particles with candidates"
        assert not ch[12:20].any()
        if frame == 4:
            assert ((ch[0::2] > 0) != (ch[1::2] > 0)).any()

    try:
        _run(ctx, orcs, "64 x 32, half fold", premise, calls=(3, 1))
    finally:
        ctx.close()
