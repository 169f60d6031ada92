"""fs_k_fused_grid64's substep boundary bit for bit against the CPU oracle after EVERY launch.

Between the iterations of one substep and those of the next, the kernel finalizes the thread's particles t + 1024 k and
predicts them again in one pass over registers (velocity loaded once, substep-start position handed over, not written to LDS
and read back), parks the substep-start positions in global memory across the search, reads the predicted positions back from
the bucket-ordered copy after it, and builds the contact set from count words fetched in one batch.  The cases are the
inputs on which such a pass can go wrong: batches of four with absent particles, state carried across substeps, frames and
launches, the exits of finalize, the contact set partly filled / full with a queue / fed by the over-the-cap search, a sphere
that moves with the substep index, several episodes in one launch.

Every case compares positions and velocities with OracleSim after every launch, and the neighbour counts, lists and shape
candidates of the last substep; each states its premise on the CPU oracle alone and asserts it.  Fold distances as in
test_grid64_finish_phase_gpu.py.
"""
import numpy as np
import pytest

import pair_search_scenes as S
from conftest import cloth_params

pytestmark = pytest.mark.gpu

LOW = (0.0, -0.005, 0.0)   # the sheet within reach of the ground plane's margin
HIGH = (0.0, -0.1, 0.0)    # 10 cm above the ground: free fall
SET_CAP = 1024
SPHERE_BITS = 8            # get_last_shape_candidates: bit q = plane q, bit 8 + q = sphere q
P_SUBSTEPS, P_DT, P_SLEEP, P_MAXACC, P_MAXSPEED = 1, 2, 15, 17, 18  # get_params


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
    assert np.isfinite(po).all() and np.isfinite(vo).all(), what
    assert np.array_equal(ph.view(np.uint32), po.view(np.uint32)), \
        f"{what}: positions not bit-exact (max abs diff {np.abs(ph - po).max():.3e})"
    assert np.array_equal(vh.view(np.uint32), vo.view(np.uint32)), \
        f"{what}: velocities not bit-exact (max abs diff {np.abs(vh - vo).max():.3e})"
    return co, m


class _Episode:
    """One episode's start: cloth rows, placement, an edit of the (n, 4) positions, start velocities ((n, 3) array or a
    callable on the positions), spheres [(radius, centre)] and an edit of the (shapes, 14) shape states."""
    def __init__(self, dimz, pos=LOW, edit=S.nothing, vel=None, spheres=(), shape_edit=None):
        self.dimz, self.pos, self.edit, self.vel, self.spheres, self.shape_edit = dimz, pos, edit, vel, spheres, shape_edit


def _run(what, episodes, premise, calls):
    """Launches of calls[.] frames; after each, premise(e, launch, before, orc, counts, masks) on the oracle's side
    (before = the oracle's (positions, velocities) in front of the launch) and everything compared."""
    from flingbot_amd import sim as fsim
    from oracle import OracleSim

    ctx = fsim.FlingSim(n_envs=len(episodes), solver=fsim.FS_SOLVER_FUSED)
    try:
        orcs = [OracleSim() for _ in episodes]
        for e, ep in enumerate(episodes):
            p = cloth_params(64, ep.dimz, pos=ep.pos)
            orcs[e].set_scene(p)
            xs = orcs[e].get_positions().reshape(-1, 4).copy()
            ep.edit(xs)
            v = np.zeros((xs.shape[0], 3), np.float32) if ep.vel is None else np.asarray(
                ep.vel(xs) if callable(ep.vel) else ep.vel, np.float32)
            ctx.env(e).set_scene(p)
            for s_ in (ctx.env(e), orcs[e]):
                s_.set_positions(xs.ravel())
                s_.set_velocities(v.ravel())
                for radius, centre in ep.spheres:
                    s_.add_sphere(radius, list(centre), [1, 0, 0, 0])
            if ep.shape_edit is not None:
                st = np.array(orcs[e].get_shape_states(), np.float32).reshape(-1, 14)
                ep.shape_edit(st)
                for s_ in (ctx.env(e), orcs[e]):
                    s_.set_shape_states(st.ravel())
        frame = 0
        for launch, k in enumerate(calls):
            before = [(o.get_positions().reshape(-1, 4).copy(), o.get_velocities().reshape(-1, 3).copy()) for o in orcs]
            ctx.step(k)
            assert ctx.last_kernel_form() == fsim.FS_FORM_FUSED_GRID64, what
            frame += k
            for e, orc in enumerate(orcs):
                orc.step(k)
                co, m = _compare(ctx, e, orc, f"{what}, episode {e}, frame {frame}")
                premise(e, launch, before[e], orc, co, m)
    finally:
        ctx.close()


@pytest.mark.parametrize("dimz", [5, 17, 64])
def test_partial_slots(gpu_required, dimz):
    """Free fall, two frames.  64 x 5: 320 particles, threads 320..1023 own nothing and the slots k >= 1 are empty; 64 x 17:
    1088, slot 1 holds 64 threads only; 64 x 64: every slot full.  Premise: nothing is listed, every particle moves."""
    def premise(e, launch, before, orc, co, m):
        assert not co.any() and not m.any()
        assert (orc.get_positions().reshape(-1, 4)[:, 1] < before[0][:, 1]).all()
        assert (orc.get_velocities().reshape(-1, 3)[:, 1] < 0.0).all()

    _run(f"64 x {dimz} in free fall", [_Episode(dimz, HIGH)], premise, calls=(1, 1))


def test_carried_state(gpu_required):
    """64 x 32 folded in half, three frames in one launch and then one more: velocity and substep-start position handed
    from finalize to predict across substeps, across the frame boundaries inside a launch and across launches (through
    global memory, which has to hold the final velocity when a launch ends).  Premise: the velocities are not zero when
    the second launch starts and the fold keeps candidates."""
    def premise(e, launch, before, orc, co, m):
        assert int((co > 0).sum()) >= 1024
        if launch == 1:
            assert np.abs(before[1]).max() > 0.0

    _run("64 x 32 folded in half", [_Episode(32, LOW, S.fold(16))], premise, calls=(3, 1))


def test_pinned_particle_with_stored_velocity(gpu_required):
    """64 x 16 in free fall, inverse mass 0 at particle 64 * 7 + 20, which carries a stored velocity: finalize zeroes it
    and predict leaves the position alone, in a pass whose other lanes -- and, in the finish phase, the same thread's
    partner row -- are finished normally.  Premise on the oracle: the particle stays, its velocity reads 0 after the
    first frame, everything else falls."""
    PIN = 64 * 7 + 20

    def pin(xs):
        xs[PIN, 3] = 0.0

    def vel(xs):
        v = np.zeros((xs.shape[0], 3), np.float32)
        v[PIN] = (0.3, -0.2, 0.1)
        return v

    def premise(e, launch, before, orc, co, m):
        po, vo = orc.get_positions().reshape(-1, 4), orc.get_velocities().reshape(-1, 3)
        assert np.array_equal(po[PIN].view(np.uint32), before[0][PIN].view(np.uint32))
        assert not vo[PIN].any()
        others = np.arange(po.shape[0]) != PIN
        assert np.abs(vo[others]).max(axis=1).min() > 0.0

    _run("64 x 16, one pinned particle", [_Episode(16, HIGH, pin, vel)], premise, calls=(1, 1))


def _params(orc):
    par = orc.get_params()
    h = np.float32(par[P_DT]) / np.float32(par[P_SUBSTEPS])
    return int(par[P_SUBSTEPS]), np.float32(par[P_DT]), np.float32(par[P_SLEEP]), np.float32(par[P_MAXACC]) * h, par[P_MAXSPEED]


def test_finalize_at_rest(gpu_required):
    """64 x 16 lying on the ground, rows 0..7 still and rows 8..15 started at 0.2 m/s along x: particles whose speed comes
    out below the sleep threshold keep their position and get velocity 0 (the asleep exit), next to particles that move
    (the plain exit).  (A sheet that lies still everywhere falls asleep everywhere on the oracle, hence the push.)  Premise on the oracle: finalize
    never stores a speed in (0, threshold) -- |v|^2 < thr^2 restated -- and after the first frame there are particles
    with velocity exactly 0 whose position did not change over the launch, and in some frame particles that moved.
    The maxSpeed exit cannot be reached: the cloth scene leaves maxSpeed at FLT_MAX, for which the kernel (like the
    oracle) skips the test."""
    moved = []

    def vel(xs):
        v = np.zeros((xs.shape[0], 3), np.float32)
        v.reshape(-1, 64, 3)[8:, :, 0] = 0.2
        return v

    def premise(e, launch, before, orc, co, m):
        _, _, thr, _, max_speed = _params(orc)
        assert thr > 0.0 and max_speed >= np.float32(3.0e38)
        po, vo = orc.get_positions().reshape(-1, 4), orc.get_velocities().reshape(-1, 3)
        v2 = vo[:, 0] * vo[:, 0] + vo[:, 1] * vo[:, 1] + vo[:, 2] * vo[:, 2]
        assert not ((v2 > 0.0) & (v2 < thr * thr)).any()
        still = (v2 == 0.0) & (po[:, :3] == before[0][:, :3]).all(axis=1)
        moved.append(int((v2 > 0.0).sum()))
        if launch == 0:
            assert still.sum() > 0

    _run("64 x 16 at rest on the ground", [_Episode(16, LOW, vel=vel)], premise, calls=(1, 1))
    assert min(moved) > 0, "a frame in which no particle took the plain exit"


def test_finalize_acceleration_clamp(gpu_required):
    """64 x 16 thrown at the ground at 3 m/s from within the contact margin: the ground stops the particles within a
    substep, a velocity change far above maxAcceleration * h, so the clamp acts in the first frame.  Premise on the oracle,
    from the velocities before and the state after the launch: without a clamp (and with the sleep rule, which changes a
    velocity by less than the threshold) every substep changes a velocity by at most maxdv + thr, so the mean velocity of
    the frame, displacement / dt, stays within S * (maxdv + thr) of the start velocity; particles beyond that bound have
    been clamped (dv2 > maxdv2 restated on the frame).  The oracle's own clamp counter agrees."""
    def vel(xs):
        v = np.zeros((xs.shape[0], 3), np.float32)
        v[:, 1] = -3.0
        return v

    def premise(e, launch, before, orc, co, m):
        if launch != 0:
            return
        S_, dt, thr, maxdv, _ = _params(orc)
        po = orc.get_positions().reshape(-1, 4)
        dv = (po[:, :3] - before[0][:, :3]) / dt - before[1]
        dv2 = (dv * dv).sum(axis=1)
        bound = np.float32(S_) * (maxdv + thr)
        assert int((dv2 > bound * bound).sum()) > 0
        assert orc.accel_clamps() > 0

    _run("64 x 16 thrown at the ground", [_Episode(16, LOW, vel=vel)], premise, calls=(1, 1))


def test_counts_partly_filled_set(gpu_required):
    """64 x 16 with 8 rows folded: one candidate for some hundred particles -- the set partly filled, the queue empty."""
    def premise(e, launch, before, orc, co, m):
        k = int((co > 0).sum())
        assert 64 <= k <= SET_CAP - 64 and co.max() == 1

    _run("64 x 16, 8 rows folded", [_Episode(16, LOW, S.fold(8))], premise, calls=(1, 1, 1, 1))


def test_counts_full_set_and_queue(gpu_required):
    """64 x 32 folded in half, half a pitch aside: the set full and 478..634 particles in the overflow queue, whose words
    carry the first candidate."""
    def premise(e, launch, before, orc, co, m):
        k = int((co > 0).sum())
        assert SET_CAP + 478 <= k <= SET_CAP + 634 and co.max() <= 16

    _run("64 x 32 folded half a pitch aside", [_Episode(32, LOW, S.fold(16, shift=S.PITCH / 2))], premise,
         calls=(1, 1, 1, 1))


def test_counts_over_the_cap(gpu_required):
    """The over-the-cap pile of pair_search_scenes.py (64 x 8, two rows drawn into 3 mm; episode 1 pins it): a count above
    96, so the one-sided search runs with its queue over all four position planes, and whatever the kernel keeps across
    the search has to survive it."""
    def premise(e, launch, before, orc, co, m):
        assert orc.max_neighbor_list() > 96
        assert (co.max() == 96) if e == 1 else (int((co > 4).sum()) >= 1)

    _run("64 x 8, two rows in a pile", [_Episode(8, LOW, S.pile), _Episode(8, LOW, S.pile_pinned)], premise,
         calls=(1, 1, 1, 1))


def test_moving_sphere(gpu_required):
    """64 x 16 on the ground with a 2 cm picker sphere that sweeps 3 cm along x over the frame, 1 mm into the sheet, in a
    launch of two frames: the sweep and collideShapes take the substep index, and every substep but the launch's first
    starts right behind a fused boundary.  Premise: the sphere's previous and current positions differ, and particles
    list it in the last substep."""
    centre = []

    def edit(xs):
        q = xs.reshape(-1, 64, 4)[8, 20]
        centre[:] = [float(q[0]), float(q[1]) + 0.019, float(q[2])]

    def move(st):
        assert st.shape[0] == 1
        st[0, 0] = st[0, 3] + np.float32(0.03)   # pos.x = prev.x + 3 cm

    def premise(e, launch, before, orc, co, m):
        st = orc.get_shape_states().reshape(-1, 14)
        assert st[0, 0] != st[0, 3]
        assert int(((m >> SPHERE_BITS) != 0).sum()) > 0

    # (the sphere's centre is known only once the positions are: the episode's edit records it)
    p = cloth_params(64, 16, pos=LOW)
    from oracle import OracleSim
    probe = OracleSim()
    probe.set_scene(p)
    edit(probe.get_positions().reshape(-1, 4).copy())
    _run("64 x 16, moving sphere", [_Episode(16, LOW, spheres=[(0.02, tuple(centre))], shape_edit=move)], premise,
         calls=(2, 1))


def test_batch_of_different_cloths(gpu_required):
    """Three episodes in one launch: 64 x 16 folded on the ground, 64 x 17 in free fall, 64 x 64 with 16 rows folded -- cloths
    of different heights, so the workgroups differ in how many slots a thread owns.  Two frames in one launch, then one."""
    def premise(e, launch, before, orc, co, m):
        if e == 1:
            assert not co.any()
        else:
            assert int((co > 0).sum()) >= 64

    eps = [_Episode(16, LOW, S.fold(8)), _Episode(17, HIGH), _Episode(64, LOW, S.fold(16))]
    _run("batch of three cloths", eps, premise, calls=(2, 1))
