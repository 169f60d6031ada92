"""fs_fork (FlingSim.fork): an episode copied into other slots on the device must be indistinguishable from its source --
the same calls on both leave identical bits, under every solver form the launches take, and equal to a context that ran the
same sequence and never forked; stepping one copy leaves the others alone.  Three sources in one context: a 24 x 20 grid
(480 particles: one full and one partial tile of 256), a 64 x 64 grid (the fused grid-64 form's cloth) and the smallest
shirt of tests/shirt_meshes.py (no grid pattern: the ELL / coded adjacency), each crumpled by a few frames of a movep that
is cut off at its step limit -- one picker still holds a particle, the spheres are in mid-motion."""
import numpy as np
import pytest

from scenarios import cloth_params

pytestmark = pytest.mark.gpu

SRC = [0, 1, 2]
PAIRS_SRC, PAIRS_DST = [0, 0, 1, 1, 2, 2], [3, 4, 5, 6, 7, 8]
FAMILY = {0: [0, 3, 4], 1: [1, 5, 6], 2: [2, 7, 8]}


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _shirt(tmp_path):
    import shirt_meshes
    from flingbot_amd import tasks as ftasks

    text = min((shirt_meshes.shirt_a(), shirt_meshes.shirt_b()), key=lambda t: len(shirt_meshes.parse(t)[0]))
    path = tmp_path / "s_processed.obj"
    path.write_text(text)
    verts, faces, stretch, bend, shear = ftasks.load_cloth(str(path))
    sp = np.array([0, 0.15, 0, -1, -1, 0.9, 0.9, 0.9, 2, 0, 2, 0, np.pi / 2, -np.pi / 2, 0, 720, 720, 0.5, 0], np.float32)
    return sp, (verts.reshape(-1), stretch.reshape(-1), bend.reshape(-1), shear.reshape(-1), faces.reshape(-1))


def _prepare_sources(sim, shirt):
    """Slots 0 .. 2: the three cloths, two pickers each, picker 0 on a particle; six frames of a grasping movep that runs
    into its limit.  Returns the targets of the movep (it is continued later)."""
    from flingbot_amd.sim import MoveLimitError

    sim.set_scene(0, cloth_params(24, 20))
    sim.set_scene(1, cloth_params(64, 64))
    sim.set_scene(2, shirt[0], *shirt[1])
    sim.step_list(SRC, 3)
    targets = []
    for e in SRC:
        pos = sim.get_positions(e).reshape(-1, 4)
        p = pos[len(pos) // 3, :3].astype(np.float64)
        centres = [p + [0.0, 0.01, 0.0], np.array([0.5, 0.5, -0.5])]
        for c in centres:
            sim.add_sphere(e, 0.02, c, [1, 0, 0, 0])
        sim.set_shape_states(e, np.array([np.hstack([c, c, [1, 0, 0, 0], [1, 0, 0, 0]]) for c in centres]))
        sim.picker_reset(e, 0.005, 0.00625, picker_radius=0.02)
        targets.append([p + [0.06, 0.3, 0.05], [0.3, 0.4, -0.3]])
    with pytest.raises(MoveLimitError):
        sim.movep(SRC, targets, [[1, 0]] * 3, speed=0.01, limit=6)
    return targets


def _continue(sim, families, targets):
    """The same continued movep (cut off again) for every listed episode, then 10 frames per cloth, the copies of a cloth
    together."""
    from flingbot_amd.sim import MoveLimitError

    envs = [e for f in families for e in f]
    tg = [targets[k] for k, f in enumerate(families) for _ in f]
    with pytest.raises(MoveLimitError):
        sim.movep(envs, tg, [[1, 0]] * len(envs), speed=0.01, limit=6)
    forms = []
    for f in families:
        sim.step_list(f, 10)
        forms.append(sim.last_kernel_form())
    return forms


def _state(sim, e):
    return dict(pos=_bits(sim.get_positions(e)), vel=_bits(sim.get_velocities(e)), phase=sim.get_phases(e).copy(),
                shapes=_bits(sim.get_shape_states(e)), picked=sim.picked(e).copy(),
                coverage=np.array([sim.coverage()[e]]).view(np.uint64), params=_bits(sim.get_params(e)),
                camera=_bits(sim.get_camera_params(e)))


def _assert_same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("solver", ["auto", "stream", "cotenant"])
def test_fork_is_bit_exact_and_independent(gpu_required, tmp_path, solver):
    from flingbot_amd import sim as fsim

    code = {"auto": fsim.FS_SOLVER_AUTO, "stream": fsim.FS_SOLVER_STREAM, "cotenant": fsim.FS_SOLVER_COTENANT}[solver]
    shirt = _shirt(tmp_path)
    sim, control = fsim.FlingSim(n_envs=9, solver=code), fsim.FlingSim(n_envs=3, solver=code)
    try:
        targets = _prepare_sources(sim, shirt)
        assert _prepare_sources(control, shirt) is not None
        for e in SRC:
            assert sim.picked(e)[0] >= 0 and sim.picked(e)[1] < 0, "picker 0 must hold a particle"
            st = sim.get_shape_states(e).reshape(-1, 14)
            assert not np.array_equal(st[0, :3], st[0, 3:6]), "the sphere must be in mid-motion"
            assert (sim.get_positions(e).reshape(-1, 4)[:, 3] == 0).sum() == 1, "one pinned particle"
            _assert_same(_state(sim, e), _state(control, e), ("before the fork", e))
        for e in (3, 5, 7):   # one destination of every source held a cloth of another size before
            sim.set_scene(e, cloth_params(16, 16))
        sim.step_list([3, 5, 7], 1)
        sim.fork(PAIRS_SRC, PAIRS_DST)
        for s, d in zip(PAIRS_SRC, PAIRS_DST):
            assert sim.n_particles(d) == sim.n_particles(s) and sim.n_shapes(d) == 2
            _assert_same(_state(sim, s), _state(sim, d), ("right after the fork", s, d))
        forms = _continue(sim, [FAMILY[k] for k in SRC], targets)
        _continue(control, [[k] for k in SRC], targets)
        if solver == "cotenant":
            assert forms[1] == fsim.FS_FORM_FUSED_GRID64, forms
        for k in SRC:
            want = _state(control, k)
            assert np.isfinite(sim.get_positions(k)).all()
            for e in FAMILY[k]:
                _assert_same(want, _state(sim, e), ("continued", solver, k, e))
        # stepping one copy leaves its source and its sibling alone
        before = {e: _state(sim, e) for e in range(9)}
        sim.step_list([4, 6, 8], 5)
        for e in (0, 1, 2, 3, 5, 7):
            _assert_same(before[e], _state(sim, e), ("untouched", e))
        for e in (4, 6, 8):
            assert not np.array_equal(before[e]["pos"], _state(sim, e)["pos"])
        # a fork forgets the snapshot of fs_snapshot_positions: the destination has none
        sim.snapshot_positions([0])
        sim.fork(0, 4)
        with pytest.raises(fsim.FlingSimError):
            sim.max_displacement([4])
        assert sim.max_displacement([0])[0] == 0.0
    finally:
        sim.close()
        control.close()


def test_fork_refusals_leave_the_context_usable(gpu_required):
    """Every refusal is an error return before anything is launched; afterwards the context forks and steps as usual."""
    from flingbot_amd import sim as fsim

    sim = fsim.FlingSim(n_envs=4, solver=0)
    try:
        sim.set_scene(0, cloth_params(24, 20))
        sim.set_scene(1, cloth_params(16, 16))
        sim.step_list([0, 1], 2)
        p0 = _bits(sim.get_positions(0)).copy()
        p1 = _bits(sim.get_positions(1)).copy()
        for src, dst in (([2], [3]),          # a source without a scene
                         ([0], [0]),          # into its own slot
                         ([0, 1], [1, 2]),    # slot 1 is a source and a destination
                         ([0, 2], [2, 3]),    # the same, the destination first
                         ([0, 1], [2, 2]),    # a destination listed twice
                         ([0], [4]), ([-1], [2]), ([], [])):
            with pytest.raises(fsim.FlingSimError):
                sim.fork(src, dst)
        with pytest.raises(ValueError):
            sim.fork([0, 1], [2])
        assert np.array_equal(_bits(sim.get_positions(0)), p0) and np.array_equal(_bits(sim.get_positions(1)), p1)
        for e in (2, 3):   # nothing was created
            with pytest.raises(fsim.FlingSimError):
                sim.get_positions(e)
        sim.fork([0, 1], [2, 3])
        sim.step_list([0, 1, 2, 3], 3)
        assert np.array_equal(_bits(sim.get_positions(0)), _bits(sim.get_positions(2)))
        assert np.array_equal(_bits(sim.get_positions(1)), _bits(sim.get_positions(3)))
        assert not np.array_equal(_bits(sim.get_positions(0)), p0)
    finally:
        sim.close()
