"""The per-episode iterate forms of the streaming back-end: fs_k_iterate_mesh (cloths without one-byte spring codes, packed
mesh words) and fs_k_iterate_mixed (every workgroup runs the body its slot's cloth allows), reached through
FS_SOLVER_STREAM_MESH at small shapes and by FS_SOLVER_AUTO above the latency threshold.

Reference of every comparison: the same cloth, perturbed the same way, stepped ALONE under FS_SOLVER_STREAM -- the latency
form (the grid-L form for a grid), which the parity suite pins to the oracle.  Comparisons are on the bits of positions and
velocities."""
import os

import numpy as np
import pytest

import shirt_meshes

pytestmark = pytest.mark.gpu

STIFF = (0.9, 0.7, 0.5)
_CLOTHS, _ALONE = {}, {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _sp(dimx=-1, dimz=-1):
    return np.array([0, 0.15, 0, dimx, dimz, *STIFF, 2, 0, 2, 0, np.pi / 2, -np.pi / 2, 0, 720, 720, 0.5, 0], np.float32)


def _cloth(kind, tmp_dir):
    """kind -> (scene_params, mesh arrays (empty for a grid), indices of the particles that get inverse mass 0)."""
    from flingbot_amd import tasks as ftasks

    if kind not in _CLOTHS:
        grids = {"grid24x27": (24, 27, ()), "grid32x32pin": (32, 32, (0,)), "grid60x64": (60, 64, ())}
        if kind in grids:
            dx, dz, pinned = grids[kind]
            _CLOTHS[kind] = (_sp(dx, dz), (), pinned)
        else:
            if kind == "sheet":   # the parity suite's small irregular mesh: it HAS stream codes
                g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "task_golden.npz"), allow_pickle=True)
                text, pinned = str(g["obj_text"]), ()
            elif kind == "shirt_big":
                text, pinned = shirt_meshes.shirt_a(body_w=33, body_h=44, sleeve_w=14, sleeve_h=14, neck=11), ()
            else:
                text, pinned = getattr(shirt_meshes, kind)(), (3, 200)
            path = tmp_dir / (kind + "_processed.obj")
            path.write_text(text)
            verts, faces, stretch, bend, shear = ftasks.load_cloth(str(path))
            arrays = (verts.reshape(-1), stretch.reshape(-1), bend.reshape(-1), shear.reshape(-1), faces.reshape(-1))
            _CLOTHS[kind] = (_sp(), arrays, pinned)
    return _CLOTHS[kind]


def _host_scene(kind, tmp_dir):
    from flingbot_amd import sim as fsim

    sp, arrays, _ = _cloth(kind, tmp_dir)
    return fsim.host_scene(sp, *arrays)


def _place(ctx, e, kind, seed, tmp_dir):
    """Scene `kind` in slot e, perturbed by seeded noise of 2 mm, its pinned particles given inverse mass 0."""
    sp, arrays, pinned = _cloth(kind, tmp_dir)
    ctx.set_scene(e, sp, *arrays)
    pos = ctx.get_positions(e).reshape(-1, 4).copy()
    pos[:, :3] += (np.random.RandomState(seed).randn(len(pos), 3) * 0.002).astype(np.float32)
    for k in pinned:
        pos[k, 3] = 0.0
    ctx.set_positions(e, pos.ravel())


def _alone(kind, seed, steps, tmp_dir):
    """(positions, velocities) of the cloth stepped alone under FS_SOLVER_STREAM; computed once per (kind, seed, steps)."""
    from flingbot_amd import sim as fsim

    key = (kind, seed, steps)
    if key not in _ALONE:
        ctx = fsim.FlingSim(n_envs=1, solver=fsim.FS_SOLVER_STREAM)
        _place(ctx, 0, kind, seed, tmp_dir)
        ctx.step(steps)
        assert ctx.last_kernel_form() in (fsim.FS_FORM_STREAM_EAGER, fsim.FS_FORM_STREAM_GRIDL), ctx.last_kernel_form()
        _ALONE[key] = (ctx.get_positions(0), ctx.get_velocities(0))
        ctx.close()
        assert np.isfinite(_ALONE[key][0]).all()
    return _ALONE[key]


def _assert_equals_alone(ctx, e, kind, seed, steps, tmp_dir):
    want_p, want_v = _alone(kind, seed, steps, tmp_dir)
    got_p, got_v = ctx.get_positions(e), ctx.get_velocities(e)
    bad_p, bad_v = int((_bits(got_p) != _bits(want_p)).sum()), int((_bits(got_v) != _bits(want_v)).sum())
    assert bad_p == 0 and bad_v == 0, (e, kind, bad_p, bad_v)


# ---- T1: the mesh form
@pytest.mark.parametrize("copies", [1, 9])
@pytest.mark.parametrize("shirt", ["shirt_a", "shirt_b"])
def test_mesh_form_equals_cloth_stepped_alone(gpu_required, tmp_path, shirt, copies):
    """shirt_a (514 particles = 2 tiles + 2 lanes, max_deg 18) and shirt_b (281) as 1 and as 9 episodes (16 slot rows, 7 of them
    empty), two particles pinned, five steps under FS_SOLVER_STREAM_MESH: fs_k_iterate_mesh in every slot, every episode
    equal to the cloth stepped alone."""
    from flingbot_amd import sim as fsim

    h = _host_scene(shirt, tmp_path)
    assert h["mesh_ok"] == 1 and not (h["stream_dict"] != 0xffffffff).any() and h["n"] == {"shirt_a": 514, "shirt_b": 281}[shirt]
    ctx = fsim.FlingSim(n_envs=copies, solver=fsim.FS_SOLVER_STREAM_MESH)
    for e in range(copies):
        _place(ctx, e, shirt, e % 2, tmp_path)
    ctx.step(5)
    assert ctx.last_kernel_form() == fsim.FS_FORM_STREAM_MESH
    assert ctx.last_slot_forms() == [fsim.FS_FORM_STREAM_MESH] * copies
    for e in range(copies):
        _assert_equals_alone(ctx, e, shirt, e % 2, 5, tmp_path)
    ctx.close()


# ---- T2 / T3: the mixed form
PATTERN = ["shirt_a", "grid24x27", "shirt_b", "grid32x32pin", "sheet"]
N_MIXED = 17


def _pattern_forms(fsim):
    per_kind = {"shirt_a": fsim.FS_FORM_STREAM_MESH, "shirt_b": fsim.FS_FORM_STREAM_MESH, "sheet": fsim.FS_FORM_STREAM_CODED,
                "grid24x27": fsim.FS_FORM_STREAM_GRIDL_TP, "grid32x32pin": fsim.FS_FORM_STREAM_GRIDL_TP}
    return [per_kind[PATTERN[e % len(PATTERN)]] for e in range(N_MIXED)]


def test_mixed_form_equals_each_cloth_stepped_alone(gpu_required, tmp_path):
    """17 episodes in two chains (the second starts at slot 8; both hold mixed forms): shirts, grids (one with a pinned corner)
    and a small mesh that has stream codes, five steps under FS_SOLVER_STREAM_MESH.  fs_k_iterate_mixed with the slot forms
    MESH, GRIDL_TP, MESH, GRIDL_TP, CODED, ...; every episode equal to itself stepped alone."""
    from flingbot_amd import sim as fsim

    sheet = _host_scene("sheet", tmp_path)
    assert (sheet["stream_dict"] != 0xffffffff).any() and sheet["mesh_ok"] == 0 and sheet["flags"]["gp_L_ok"] == 0
    ctx = fsim.FlingSim(n_envs=N_MIXED, solver=fsim.FS_SOLVER_STREAM_MESH)
    ctx.set_stream_groups(2)
    for e in range(N_MIXED):
        _place(ctx, e, PATTERN[e % len(PATTERN)], e, tmp_path)
    ctx.step(5)
    assert ctx.last_kernel_form() == fsim.FS_FORM_STREAM_MIXED and ctx.last_stream_groups() == 2
    assert ctx.last_slot_forms() == _pattern_forms(fsim)
    for e in range(N_MIXED):
        _assert_equals_alone(ctx, e, PATTERN[e % len(PATTERN)], e, 5, tmp_path)
    ctx.close()


def _movep_run(fsim, solver, episodes, tmp_dir):
    """For each listed (kind, seed, lift): place the cloth, put picker sphere 0 on particle 5 and picker 1 half a metre above
    the scene, then ONE movep that grasps the particle and lifts it by `lift` (5 mm per step).  Returns (iterations, picked
    ids, positions, velocities)."""
    n = len(episodes)
    ctx = fsim.FlingSim(n_envs=n, solver=solver)
    if n > 8:
        ctx.set_stream_groups(2)
    up = []
    for e, (kind, seed, lift) in enumerate(episodes):
        _place(ctx, e, kind, seed, tmp_dir)
        p5 = ctx.get_positions(e).reshape(-1, 4)[5, :3].astype(np.float64)
        centres = [p5, np.array([0.0, 0.5, 0.0])]
        for c in centres:
            ctx.env(e).add_sphere(0.02, c, [1, 0, 0, 0])
        st = np.array(ctx.env(e).get_shape_states()).reshape(-1, 14)
        for i, c in enumerate(centres):
            st[i] = np.hstack([c, c, [1, 0, 0, 0], [1, 0, 0, 0]])
        ctx.env(e).set_shape_states(st)
        ctx.picker_reset(e, picker_radius=0.02)
        up.append([p5 + [0.01, lift, 0.0], centres[1]])
    ids = list(range(n))
    iters = ctx.movep(ids, np.array(up), [[1, 0]] * n, speed=5e-3)
    out = (np.asarray(iters).tolist(), [int(ctx.picked(e)[0]) for e in ids], [ctx.get_positions(e) for e in ids],
           [ctx.get_velocities(e) for e in ids])
    ctx.close()
    return out


def test_mixed_form_through_movep_device_lists(gpu_required, tmp_path):
    """The mixed set through movep (fs_advance's device id lists): one grasped particle per episode, lifted by a different
    distance in every episode, so the picker spheres move and the slots retire at different frames.  Every episode equals the
    same movep run alone."""
    from flingbot_amd import sim as fsim

    episodes = [(PATTERN[e % len(PATTERN)], e, 0.03 + 0.004 * e) for e in range(N_MIXED)]
    iters, picked, pos, vel = _movep_run(fsim, fsim.FS_SOLVER_STREAM_MESH, episodes, tmp_path)
    assert all(p == 5 for p in picked), picked
    assert len(set(iters)) >= 8, iters                                   # the slots retire at different frames
    for e, ep in enumerate(episodes):
        it1, picked1, pos1, vel1 = _movep_run(fsim, fsim.FS_SOLVER_STREAM, [ep], tmp_path)
        assert it1[0] == iters[e] and picked1 == [5], (e, it1, iters[e])
        bad_p, bad_v = int((_bits(pos[e]) != _bits(pos1[0])).sum()), int((_bits(vel[e]) != _bits(vel1[0])).sum())
        assert bad_p == 0 and bad_v == 0 and np.isfinite(pos[e]).all(), (e, ep[0], bad_p, bad_v)


# ---- T4: FS_SOLVER_AUTO at the real threshold (one test per launch class that passed its measurement, EXPERIMENTS R29.1: both)
def test_auto_takes_the_mesh_form_above_the_latency_threshold(gpu_required, tmp_path):
    """36 shirts of 3764 particles (135 504 > 32 x 4096: two chains, 15 tiles per slot), two steps under FS_SOLVER_AUTO:
    fs_k_iterate_mesh; three episodes equal the cloth stepped alone.  FS_SOLVER_STREAM on the same launch keeps the
    uncompressed adjacency."""
    from flingbot_amd import sim as fsim

    copies = 36
    ctx = fsim.FlingSim(n_envs=copies, solver=fsim.FS_SOLVER_AUTO)
    for e in range(copies):
        _place(ctx, e, "shirt_big", 3, tmp_path)
    assert ctx.n_particles(0) * copies == 135504
    ctx.step(2)
    assert ctx.last_kernel_form() == fsim.FS_FORM_STREAM_MESH
    assert ctx.last_slot_forms() == [fsim.FS_FORM_STREAM_MESH] * copies
    for e in (0, 17, 35):
        _assert_equals_alone(ctx, e, "shirt_big", 3, 2, tmp_path)
    ctx.set_solver(fsim.FS_SOLVER_STREAM)
    ctx.step(1)
    assert ctx.last_kernel_form() == fsim.FS_FORM_STREAM_ELL
    assert ctx.last_slot_forms() == [fsim.FS_FORM_STREAM_ELL] * copies
    ctx.close()


def test_auto_takes_the_mixed_form_above_the_latency_threshold(gpu_required, tmp_path):
    """24 shirts of 3764 particles and 12 grids of 60 x 64 (136 416 particles), two steps under FS_SOLVER_AUTO:
    fs_k_iterate_mixed with the grids' slots on the grid-L throughput body; three episodes equal themselves stepped alone."""
    from flingbot_amd import sim as fsim

    kinds = ["shirt_big", "shirt_big", "grid60x64"] * 12
    ctx = fsim.FlingSim(n_envs=len(kinds), solver=fsim.FS_SOLVER_AUTO)
    for e, kind in enumerate(kinds):
        _place(ctx, e, kind, 3, tmp_path)
    assert sum(ctx.n_particles(e) for e in range(len(kinds))) == 136416
    ctx.step(2)
    assert ctx.last_kernel_form() == fsim.FS_FORM_STREAM_MIXED
    want = {"shirt_big": fsim.FS_FORM_STREAM_MESH, "grid60x64": fsim.FS_FORM_STREAM_GRIDL_TP}
    assert ctx.last_slot_forms() == [want[k] for k in kinds]
    for e in (0, 2, 34):
        _assert_equals_alone(ctx, e, kinds[e], 3, 2, tmp_path)
    ctx.close()
