"""Start states and the launch-by-launch comparison of tests/test_grid64_list_sort_gpu.py (the sort pass of the half-stencil
neighbour search of fs_k_fused_grid64)."""
import numpy as np

from conftest import cloth_params

HIGH = (0.0, -0.1, 0.0)
LOW = (0.0, -0.005, 0.0)  # the sheet within reach of the ground plane's margin


def ramp(lo, hi):
    """Density ramp on a 64 x dimz cloth: rows 0 and 1 (128 particles) pinned (inverse mass 0) on one line of x whose
    spacing grows geometrically from `lo` to `hi`, the two rows 1 mm apart in y and 3 mm above the sheet.  Where the spacing
    is small a particle has dozens of the 127 others within the search radius, where it is large none: one episode holds
    lists of every length from 0 up to the dense end's."""
    def edit(xs):
        g = xs.reshape(-1, 64, 4)
        steps = np.geomspace(lo, hi, 64)
        x = (g[0, 32, 0] + np.cumsum(steps) - steps.sum() / 2).astype(np.float32)
        z, y = g[0, :, 2].copy(), g[0, :, 1].copy()
        for iz in range(2):
            g[iz, :, 0] = x
            g[iz, :, 2] = z
            g[iz, :, 1] = y + np.float32(0.003 + 0.001 * iz)
        xs[:128, 3] = 0.0
    return edit


def compare(ctx, e, orc, what):
    """Counts, lists, shape candidates, positions and velocities of episode e against the oracle, bit for bit."""
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
    return co


def start(sim, dimz, pos, edit):
    """Scene and edited start state on `sim` (an episode of the device context, or the oracle)."""
    sim.set_scene(cloth_params(64, dimz, pos=pos))
    xs = sim.get_positions().reshape(-1, 4).copy()
    edit(xs)
    sim.set_positions(xs.ravel())
    sim.set_velocities(np.zeros(3 * xs.shape[0], np.float32))


def run(what, episodes, premise, calls):
    """episodes: (dimz, pos, edit) each, all in one context; launches of calls[.] frames; after every launch everything is
    compared and premise(e, counts, orc) asserted on the oracle's side."""
    from flingbot_amd import sim as fsim
    from oracle import OracleSim

    ctx = fsim.FlingSim(n_envs=len(episodes), solver=fsim.FS_SOLVER_FUSED)
    try:
        orcs = [OracleSim() for _ in episodes]
        for e, (dimz, pos, edit) in enumerate(episodes):
            start(orcs[e], dimz, pos, edit)
            ctx.env(e).set_scene(cloth_params(64, dimz, pos=pos))
            ctx.env(e).set_positions(orcs[e].get_positions())
            ctx.env(e).set_velocities(np.zeros(3 * 64 * dimz, np.float32))
        frame = 0
        for k in calls:
            ctx.step(k)
            assert ctx.last_kernel_form() == fsim.FS_FORM_FUSED_GRID64, what
            frame += k
            for e, orc in enumerate(orcs):
                orc.step(k)
                premise(e, compare(ctx, e, orc, f"{what}, episode {e}, frame {frame}"), orc)
    finally:
        ctx.close()
