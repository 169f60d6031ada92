"""fs_k_fused_grid64 with springs shared inside the wavefront, bit for bit against the CPU oracle after EVERY frame.

A trip of the kernel owns two adjacent rows (P even, Q = P + 1).  The horizontal springs of both rows and the vertical and
diagonal springs between P and Q are evaluated once, at one endpoint, and the other endpoint takes the scale through
registers (DPP lane shift or the same thread); springs to other wavefronts are evaluated at both ends.  The cases below
put coincident particles (squared length 0: the pair must leave the fast form) on every kind of shared spring and on a
cross-wave one, inverse mass 0 on a P row and on a Q row, and run cloths with fewer than 64 rows (odd heights leave a
last P row without its Q) and a few frames of bench.py's 256-episode workload.
"""
import numpy as np
import pytest

import bench
from conftest import cloth_params

pytestmark = pytest.mark.gpu


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


def _episodes(edits, dimz=64, jitter_seed=None):
    """One episode per entry of `edits` (callables on the (n, 4) position array), on the HIP batch and on oracles."""
    from flingbot_amd import sim as fsim
    from oracle import OracleSim

    ctx = fsim.FlingSim(n_envs=len(edits), solver=fsim.FS_SOLVER_FUSED)
    orcs = [OracleSim() for _ in edits]
    p = cloth_params(64, dimz, pos=(0.0, -0.1, 0.0))
    for e, edit in enumerate(edits):
        orcs[e].set_scene(p)
        pos = orcs[e].get_positions().reshape(-1, 4).copy()
        if jitter_seed is not None:
            rng = np.random.RandomState(jitter_seed + e)
            pos[:, :3] += (rng.rand(pos.shape[0], 3).astype(np.float32) - 0.5) * 0.004
        edit(pos)
        ctx.env(e).set_scene(p)
        for s_ in (ctx.env(e), orcs[e]):
            s_.set_positions(pos.ravel())
    return ctx, orcs


def _coincide(r0, c0, r1, c1):
    def edit(pos):
        pos[64 * r1 + c1, :3] = pos[64 * r0 + c0, :3]
    return edit


def test_coincident_particles_on_shared_springs_bit_exact(gpu_required):
    """Squared length 0 on each kind of shared spring (P row 20, Q row 21 / 41) and on a cross-wave one (Q row 21 -> P row
    22): the fast form must see it even though only one endpoint evaluates the spring."""
    cases = [
        ("horizontal, columns 0/1, P row", _coincide(20, 0, 20, 1)),
        ("horizontal, columns 62/63, Q row", _coincide(41, 62, 41, 63)),
        ("horizontal distance 2, columns 0/2, Q row", _coincide(21, 0, 21, 2)),
        ("P-Q vertical", _coincide(20, 31, 21, 31)),
        ("P-Q diagonal (-1, +1)", _coincide(20, 31, 21, 30)),
        ("P-Q diagonal (+1, +1)", _coincide(20, 31, 21, 32)),
        ("cross-wave vertical", _coincide(21, 31, 22, 31)),
    ]
    ctx, orcs = _episodes([c[1] for c in cases])
    try:
        _run(ctx, orcs, 4, "coincident particles: " + ", ".join(c[0] for c in cases))
    finally:
        ctx.close()


def test_pinned_particle_on_p_and_q_rows_bit_exact(gpu_required):
    """Inverse mass 0 (what a picker gives the particle it holds) on a P row and on a Q row: the waves around it take the
    general path, their neighbours in the other row of the trip still the shared fast one."""
    def pin(r, c):
        def edit(pos):
            pos[64 * r + c, 3] = 0.0
        return edit

    ctx, orcs = _episodes([pin(30, 10), pin(31, 50), pin(0, 0), pin(63, 63)], jitter_seed=7)
    try:
        _run(ctx, orcs, 4, "pinned particle")
    finally:
        ctx.close()


@pytest.mark.parametrize("dimz", [39, 33, 5])
def test_fewer_rows_bit_exact(gpu_required, dimz):
    """Cloths of 39, 33 and 5 rows: trips past the cloth, and an odd height's last row, whose trip has no Q row."""
    ctx, orcs = _episodes([lambda pos: None, lambda pos: None], dimz=dimz, jitter_seed=40)
    try:
        _run(ctx, orcs, 4, f"64 x {dimz} cloth")
    finally:
        ctx.close()


def test_bench_workload_frames_bit_exact(gpu_required):
    """Three frames of bench.py's 256-episode launch, sampled episodes compared after every frame."""
    from flingbot_amd import sim as fsim
    from oracle import OracleSim

    ctx = fsim.FlingSim(n_envs=256, solver=fsim.FS_SOLVER_FUSED)
    for e in range(256):
        bench.setup_episode(ctx.env(e), seed=e)
    sample = (0, 97, 255)
    orcs = []
    for s in sample:
        o = OracleSim()
        bench.setup_episode(o, seed=s)
        orcs.append(o)
    try:
        for f in range(3):
            ctx.step(1)
            assert ctx.last_kernel_form() == fsim.FS_FORM_FUSED_GRID64
            for s, o in zip(sample, orcs):
                o.step(1)
                _check(ctx, s, o, f"bench workload, episode {s}, frame {f + 1}")
    finally:
        ctx.close()
