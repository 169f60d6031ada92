"""fs_k_fused_grid64 with the edge stiffness of its spring block as LDS TABLES, its shear rest lengths per slot and the clamp in
front of the contact roots: bit for bit against the CPU oracle after EVERY frame.

The kernel reads `stiffness / 2, or +0 outside the grid` of an evaluated slot from LDS tables -- per column for the shear
slots 2, 3, 6, 7 (a trip whose ROW lacks the slot reads rows of zeros instead), per row for the z-direction slots 8..11 --
and the six shear rest lengths of a pair per particle and slot (Q's slots 2, 3, 6, 7, P's 2, 3).  A mix-up of rows, slots or
halves changes bits only when the values differ, so the scenes here give every spring family its own stiffness (premise
asserted from the springs the scene reports) and sit at an offset where the four shear rest lengths of a particle differ
(premise asserted likewise).  Cloth heights: 5 rows (the last P row has no Q and takes the exact path), 6 (every row-edge
condition within three trips), 33 and 64.  Pinned particles at the corners of the grid send their own pair down the exact
path while the fast pairs around them read the tables at the grid's edge.  The clamp of fs_rsqrt in front of the contact
roots is driven by squared lengths of 0 (coincident particles that share no spring), a denormal (1e-20 apart) and the
near-zero tangential displacement of a sheet at rest on the ground.
"""
import numpy as np
import pytest

from conftest import cloth_params

pytestmark = pytest.mark.gpu

STIFF = (0.9, 0.6, 0.3)
OFFSETS = {"default": (0.0, -0.1, 0.0), "shifted": (0.37, -0.1, -0.21)}


def _check(ctx, e, orc, what):
    ph, po = ctx.get_positions(e), orc.get_positions()
    vh, vo = ctx.get_velocities(e), orc.get_velocities()
    assert np.isfinite(po).all(), what
    assert np.array_equal(ph.view(np.uint32), po.view(np.uint32)), \
        f"{what}: positions not bit-exact (max abs diff {np.abs(ph - po).max():.3e})"
    assert np.array_equal(vh.view(np.uint32), vo.view(np.uint32)), \
        f"{what}: velocities not bit-exact (max abs diff {np.abs(vh - vo).max():.3e})"


def _run(ctx, orcs, frames, what):
    from flingbot_amd import sim as fsim

    for f in range(frames):
        ctx.step(1)
        assert ctx.last_kernel_form() == fsim.FS_FORM_FUSED_GRID64, what
        for e, orc in enumerate(orcs):
            orc.step(1)
            _check(ctx, e, orc, f"{what}, episode {e}, frame {f + 1}")


def _episodes(edits, dimz=64, jitter_seed=None, pos=OFFSETS["default"], stiff=STIFF):
    """One episode per entry of `edits` (callables on the (n, 4) position array), on the HIP batch and on oracles."""
    from flingbot_amd import sim as fsim
    from oracle import OracleSim

    assert len(edits) <= 8
    ctx = fsim.FlingSim(n_envs=len(edits), solver=fsim.FS_SOLVER_FUSED)
    orcs = [OracleSim() for _ in edits]
    p = cloth_params(64, dimz, pos=pos, stiff=stiff)
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
    return ctx, orcs


def _springs(sim_like, *env):
    """(dx, dz) >= per spring, rest lengths, stiffness, endpoints -- from what the scene itself reports."""
    ed = np.asarray(sim_like.get_edges(*env)).reshape(-1, 2)
    L = np.asarray(sim_like.get_spring_lengths(*env), np.float32)
    k = np.asarray(sim_like.get_spring_stiffness(*env), np.float32)
    dx = np.abs(ed[:, 1] % 64 - ed[:, 0] % 64)
    dz = np.abs(ed[:, 1] // 64 - ed[:, 0] // 64)
    return ed, dx, dz, L, k


def _assert_premises(ctx, orc, dimz):
    for sim_like, env in ((ctx, (0,)), (orc, ())):
        ed, dx, dz, L, k = _springs(sim_like, *env)
        fam = {"stretch": (dx + dz) == 1, "shear": (dx == 1) & (dz == 1), "bend": ((dx == 2) & (dz == 0)) | ((dx == 0) & (dz == 2))}
        assert sum(int(m.sum()) for m in fam.values()) == len(k), "a spring outside the three families"
        bits = {}
        for name, m in fam.items():
            u = np.unique(k[m].view(np.uint32))
            assert len(u) == 1, f"{name}: {len(u)} stiffness values"
            bits[name] = int(u[0])
        assert len(set(bits.values())) == 3, f"the three families' stiffness bits do not differ: {bits}"
        # the four shear rest lengths of an interior particle: not bit-equal for at least one particle
        n = 64 * dimz
        shear = fam["shear"]
        per = [[] for _ in range(n)]
        for (i, j), l in zip(ed[shear], L[shear].view(np.uint32)):
            per[i].append(int(l))
            per[j].append(int(l))
        differing = sum(1 for i in range(n) if len(per[i]) == 4 and len(set(per[i])) > 1)
        assert differing >= 1, "every interior particle has four bit-equal shear rest lengths: an interleave mix-up would not show"


@pytest.mark.parametrize("offset", sorted(OFFSETS))
@pytest.mark.parametrize("dimz", [5, 6, 33, 64])
def test_distinct_stiffness_and_shear_lengths_bit_exact(gpu_required, dimz, offset):
    """Stiffness (0.9, 0.6, 0.3) per family and per-slot shear rest lengths on jittered cloths of 5, 6, 33 and 64 rows, at
    the default offset and at (0.37, -0.1, -0.21)."""
    ctx, orcs = _episodes([lambda xs: None, lambda xs: None], dimz=dimz, jitter_seed=130, pos=OFFSETS[offset])
    try:
        _assert_premises(ctx, orcs[0], dimz)
        _run(ctx, orcs, 4, f"64 x {dimz} cloth, stiffness {STIFF}, offset {offset}")
    finally:
        ctx.close()


def _pin(r, c):
    def edit(xs):
        xs[64 * r + c, 3] = 0.0
    return edit


PIN_DIMZ = 64
PIN_CASES = {
    "first rows": [(r, c) for r in (0, 1) for c in (0, 1, 62, 63)],
    "last rows": [(r, c) for r in (PIN_DIMZ - 2, PIN_DIMZ - 1) for c in (0, 1, 62, 63)],
    "middle": [(31, 30)],
}


@pytest.mark.parametrize("where", sorted(PIN_CASES))
def test_pinned_particle_at_the_edges_bit_exact(gpu_required, where):
    """One particle of inverse mass 0 per episode, at columns 0, 1, 62, 63 of the first two and the last two rows and in the
    middle of the cloth: its pair (and every pair that holds a neighbour of it) takes the exact path, the fast pairs around
    read the stiffness tables at the grid's edge."""
    cells = PIN_CASES[where]
    ctx, orcs = _episodes([_pin(r, c) for r, c in cells], dimz=PIN_DIMZ, jitter_seed=140, pos=OFFSETS["shifted"])
    try:
        for e, (r, c) in enumerate(cells):
            assert ctx.get_positions(e).reshape(-1, 4)[64 * r + c, 3] == 0.0
        _run(ctx, orcs, 4, f"pinned particle, {where}: {cells}")
    finally:
        ctx.close()


# pairs of particles that share no spring (three rows or three columns apart) and are no rest-pose neighbours
FAR_PAIRS = [((10, 10), (13, 10)), ((0, 0), (3, 0)), ((40, 5), (40, 8)), ((63, 63), (60, 63))]


def _onto(a, b, gap):
    """particle b put `gap` beside particle a in x (a moved to x = 0 first, so that a tiny gap survives the subtraction)"""
    def edit(xs):
        ia, ib = 64 * a[0] + a[1], 64 * b[0] + b[1]
        if gap != 0.0:
            xs[ia, 0] = 0.0
        xs[ib, :3] = xs[ia, :3]
        xs[ib, 0] += np.float32(gap)
    return edit


@pytest.mark.parametrize("gap", [0.0, 1e-20])
def test_contact_root_of_a_zero_or_denormal_squared_length_bit_exact(gpu_required, gap):
    """Two particles without a common spring at the same place (squared length 0) or 1e-20 apart (a denormal squared
    length): the particle contact takes its root through the clamp of fs_rsqrt."""
    for a, b in FAR_PAIRS:
        assert max(abs(a[0] - b[0]), abs(a[1] - b[1])) > 2, "the pair shares a spring"
    ctx, orcs = _episodes([_onto(a, b, gap) for a, b in FAR_PAIRS])
    try:
        for e, (a, b) in enumerate(FAR_PAIRS):  # premise: the squared length the contact sees
            x = ctx.get_positions(e).reshape(-1, 4)
            d = x[64 * a[0] + a[1], :3] - x[64 * b[0] + b[1], :3]
            l2 = np.float32(d[0] * d[0]) + np.float32(d[1] * d[1]) + np.float32(d[2] * d[2])
            assert (l2 == 0.0) if gap == 0.0 else (0.0 < float(np.abs(d).max()) < 1e-19 and float(d[0]) ** 2 < 1.17549435e-38)
        _run(ctx, orcs, 4, f"particles without a common spring {gap} apart")
    finally:
        ctx.close()


def test_sheet_at_rest_on_the_ground_bit_exact(gpu_required):
    """A flat sheet lying on the ground plane with zero velocity (exactly flat; 2 mm up; jittered by a micrometre): the
    plane contact's friction takes the root of a tangential displacement that is zero or next to it."""
    def flat(y, wobble=0.0):
        def edit(xs):
            xs[:, 1] = np.float32(y)
            if wobble:
                rng = np.random.RandomState(150)
                xs[:, :3] += (rng.rand(xs.shape[0], 3).astype(np.float32) - 0.5) * np.float32(wobble)
        return edit

    ctx, orcs = _episodes([flat(0.0), flat(0.002), flat(0.002, 1e-6)])
    try:
        _run(ctx, orcs, 4, "sheet at rest on the ground")
    finally:
        ctx.close()
