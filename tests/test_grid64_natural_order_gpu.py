"""fs_k_fused_grid64 with every in-wave spring evaluated at the endpoint whose slot comes first in the canonical order, bit
for bit against the CPU oracle after EVERY frame.

A trip owns rows P (even) and Q = P + 1.  s0 / s1 of both rows and Q's s2, s3, s8 are evaluated in place; s4 / s5 take the
scale from the lanes to the right (+0 arrives at columns 63 / 62, 63), P's s6 takes Q's s2 from the left, P's s7 Q's s3
from the right, P's s10 Q's s8 from the same thread.  The cases put coincident particles (squared length 0, which only the
evaluating endpoint can see) where those takers sit at the edge of the grid, on a middle trip and on the first and the last
rows of the cloth; put neighbours 1e-20 apart (a denormal squared length: the fast form's root has no clamp in front and
leaves such a pair to the exact path); run cloths whose last P row has no Q; and drive the three places a particle's contacts are finished in
-- contact set, overflow queue, inline fallback -- with a premise asserted from the neighbour counts of the first frame.

Fold distances: the search radius and the contact rest distance are both 1.8 pitches = 11.25 mm.  A layer laid closer than
~10.5 mm is pushed beyond the radius within one frame (the lists are empty again at the frame's last substep); at 11 mm it
is in contact and stays there.  On the CPU oracle alone: rows 0..15 folded onto rows 31..16 at 11 mm give 1632 particles
with a candidate after the first frame (> 1024 = contact set, < 2560 = set + queue), the sheet folded in half 3680.
"""
import numpy as np
import pytest

from conftest import cloth_params

pytestmark = pytest.mark.gpu

SET_CAP, QUEUE_CAP = 1024, 1536
FOLD_LIFT = 0.011


def _check(ctx, e, orc, what):
    ph, po = ctx.get_positions(e), orc.get_positions()
    vh, vo = ctx.get_velocities(e), orc.get_velocities()
    assert np.isfinite(po).all(), what
    assert np.array_equal(ph.view(np.uint32), po.view(np.uint32)), \
        f"{what}: positions not bit-exact (max abs diff {np.abs(ph - po).max():.3e})"
    assert np.array_equal(vh.view(np.uint32), vo.view(np.uint32)), \
        f"{what}: velocities not bit-exact (max abs diff {np.abs(vh - vo).max():.3e})"


def _run(ctx, orcs, frames, what, premise=None):
    from flingbot_amd import sim as fsim

    for f in range(frames):
        ctx.step(1)
        assert ctx.last_kernel_form() == fsim.FS_FORM_FUSED_GRID64, what
        for e, orc in enumerate(orcs):
            orc.step(1)
            if f == 0 and premise is not None:
                premise(ctx, e, orc)
            _check(ctx, e, orc, f"{what}, episode {e}, frame {f + 1}")


def _episodes(edits, dimz=64, jitter_seed=None, pos=(0.0, -0.1, 0.0), spheres=None):
    """One episode per entry of `edits` (callables on the (n, 4) position array), on the HIP batch and on oracles;
    spheres[e] = callable on the edited positions returning [(radius, centre), ...], added to episode e on both."""
    from flingbot_amd import sim as fsim
    from oracle import OracleSim

    ctx = fsim.FlingSim(n_envs=len(edits), solver=fsim.FS_SOLVER_FUSED)
    orcs = [OracleSim() for _ in edits]
    p = cloth_params(64, dimz, pos=pos)
    for e, edit in enumerate(edits):
        orcs[e].set_scene(p)
        xs = orcs[e].get_positions().reshape(-1, 4).copy()
        if jitter_seed is not None:
            rng = np.random.RandomState(jitter_seed + e)
            xs[:, :3] += (rng.rand(xs.shape[0], 3).astype(np.float32) - 0.5) * 0.004
        edit(xs)
        ctx.env(e).set_scene(p)
        for s_ in (ctx.env(e), orcs[e]):
            s_.set_positions(xs.ravel())
            s_.set_velocities(np.zeros(3 * xs.shape[0], np.float32))
            for radius, centre in (spheres[e](xs) if spheres and e in spheres else ()):
                s_.add_sphere(radius, list(centre), [1, 0, 0, 0])
    return ctx, orcs


def _coincide(r0, c0, r1, c1):
    def edit(xs):
        xs[64 * r1 + c1, :3] = xs[64 * r0 + c0, :3]
    return edit


def _horizontal(P, Q):
    return [(f"({r}, {a}) = ({r}, {b})", _coincide(r, a, r, b))
            for a, b in ((62, 63), (61, 63), (0, 1), (0, 2)) for r in (P, Q)]


def _between(P, Q):
    return [(f"({P}, {a}) = ({Q}, {b})", _coincide(P, a, Q, b))
            for a, b in ((0, 1), (1, 0), (63, 62), (62, 63), (0, 0), (31, 31), (63, 63))]


@pytest.mark.parametrize("P", [40, 0, 62])
@pytest.mark.parametrize("kind", ["horizontal", "between"])
def test_coincident_particles_where_the_takers_sit_at_the_edge(gpu_required, P, kind):
    """Squared length 0 on the springs whose taker is an edge lane -- horizontal ones at columns 62 / 63 and 61 / 63 (and
    0 / 1, 0 / 2, where the evaluator now sits), the two P-Q diagonals touching columns 0 and 63 in both directions, the P-Q
    vertical -- on a middle trip (rows 40, 41), the first rows of the cloth (0, 1) and the last (62, 63)."""
    cases = _horizontal(P, P + 1) if kind == "horizontal" else _between(P, P + 1)
    assert len(cases) <= 8
    ctx, orcs = _episodes([c[1] for c in cases])
    try:
        _run(ctx, orcs, 4, "coincident particles: " + ", ".join(c[0] for c in cases))
    finally:
        ctx.close()


def _nearly_coincide(r0, c0, r1, c1):
    """(r1, c1) 1e-20 beside (r0, c0), which is put at x = 0 (column 0 is there already) so that the difference survives:
    squared length 1e-40."""
    def edit(xs):
        xs[64 * r0 + c0, 0] = 0.0
        xs[64 * r1 + c1, :3] = xs[64 * r0 + c0, :3]
        xs[64 * r1 + c1, 0] = 1e-20
    return edit


def test_denormal_squared_length_bit_exact(gpu_required):
    """Two neighbours 1e-20 apart: the spring's squared length is a denormal, below the FLT_MIN that fs_rsqrt clamps to.  The
    fast form takes the root without the clamp and must hand such a pair to the exact path (which clamps): on an in-wave
    horizontal spring of a P and of a Q row, the P-Q vertical and diagonal, and a cross-wave vertical."""
    cases = [_nearly_coincide(40, 0, 40, 1), _nearly_coincide(41, 0, 41, 1), _nearly_coincide(40, 0, 41, 0),
             _nearly_coincide(40, 0, 41, 1), _nearly_coincide(41, 0, 42, 0), _nearly_coincide(40, 0, 40, 2)]
    ctx, orcs = _episodes(cases)
    try:
        _run(ctx, orcs, 4, "neighbours 1e-20 apart")
    finally:
        ctx.close()


@pytest.mark.parametrize("dimz", [5, 33])
def test_last_p_row_without_q_bit_exact(gpu_required, dimz):
    """64 x 5 and 64 x 33 cloths, jittered: the last row is a P row without its Q and takes the exact path, the Q row
    above it evaluates its s10 / s11 towards it across the trip boundary."""
    ctx, orcs = _episodes([lambda xs: None, lambda xs: None], dimz=dimz, jitter_seed=110)
    try:
        _run(ctx, orcs, 4, f"64 x {dimz} cloth")
    finally:
        ctx.close()


def _fold(rows, shift=0.0, then=None):
    """Rows 0..rows-1 laid flat onto rows 2 rows - 1..rows, FOLD_LIFT above them (shifted by `shift` in x)."""
    def edit(xs):
        g = xs.reshape(64, 64, 4)
        for iz in range(rows):
            g[iz, :, 2] = g[2 * rows - 1 - iz, :, 2]
            g[iz, :, 1] = g[2 * rows - 1 - iz, :, 1] + FOLD_LIFT
            g[iz, :, 0] += shift
        if then is not None:
            then(xs)
    return edit


def _with_candidates(ctx, e, orc):
    ch, _ = ctx.get_last_neighbors(e)
    co, _ = orc.get_last_neighbors()
    assert np.array_equal(ch, co), f"episode {e}: neighbour counts differ from the oracle"
    return ch, int((ch > 0).sum())


def test_overflow_queue_in_use_bit_exact(gpu_required):
    """The first 16 rows folded flat onto the next 16: more particles with a candidate than the contact set holds, fewer
    than set + queue, so the rest is finished from the queue and nothing inline.  Episode 1 has a particle of inverse mass
    0 in the folded region, episode 2 a coincident pair there (its wave takes the exact path and writes queue entries with
    its own spring counts), episode 3 two spheres, one resting on the folded region (shape candidates on queued particles)."""
    def pin(xs):
        xs[64 * 9 + 40, 3] = 0.0

    def spheres(xs):  # one 2 cm sphere pressing 1 mm into the upper layer of the fold, one parked far away
        q = xs.reshape(64, 64, 4)[8, 20]
        return [(0.02, (float(q[0]), float(q[1]) + 0.019, float(q[2]))), (0.02, (0.5, 0.5, -0.5))]

    edits = [_fold(16), _fold(16, then=pin), _fold(16, then=_coincide(8, 30, 8, 31)), _fold(16)]
    ctx, orcs = _episodes(edits, pos=(0.0, -0.005, 0.0), spheres={3: spheres})

    def premise(ctx, e, orc):
        ch, k = _with_candidates(ctx, e, orc)
        assert SET_CAP < k < SET_CAP + QUEUE_CAP, f"episode {e}: {k} particles with candidates: the queue is not the path taken"
        assert ch.max() <= 16
        if e == 3:
            m = ctx.get_last_shape_candidates(e)
            assert np.array_equal(m, orc.get_last_shape_candidates())
            both = int(((m >> 8 != 0) & (ch > 0)).sum())
            assert both > 200, f"only {both} particles with a contact candidate have a sphere candidate"

    try:
        _run(ctx, orcs, 4, "quarter fold (overflow queue)", premise)
    finally:
        ctx.close()


def test_inline_fallback_in_use_bit_exact(gpu_required):
    """The sheet folded in half onto itself (episode 1: shifted half a pitch, two candidates each): more particles with
    candidates than contact set and queue hold together, so the rest is finished inline in the main loop."""
    ctx, orcs = _episodes([_fold(32), _fold(32, shift=0.003125)], pos=(0.0, -0.005, 0.0))

    def premise(ctx, e, orc):
        _, k = _with_candidates(ctx, e, orc)
        assert k > SET_CAP + QUEUE_CAP, f"episode {e}: {k} particles with candidates: set and queue do not overflow"

    try:
        _run(ctx, orcs, 4, "half fold (inline fallback)", premise)
    finally:
        ctx.close()
