"""fs_state_gather / fs_state_scatter (csrc/fs_state.hip) through FlingSim.state_tensors / set_state_tensors on the GPU.

The standing context holds the smallest shapes at which a tile bound, a padded tail or a per-row count can go wrong: grid
cloths 3 x 5, 8 x 8, 9 x 7 and 17 x 16 (272 particles: one full tile of 256 and a partial one), the smaller shirt of
tests/shirt_meshes.py, one 64 x 64 (16 full tiles), and a slot without a scene.  Every cloth has two pickers; the 17 x 16 one
is grasped and moved for a few frames (a zero inverse mass), all have fallen for a few frames (non-zero velocities).  The
reference is the per-episode getters, read once, packed by tests/state_tensor_reference.py and compared as uint32."""
import ctypes as C

import numpy as np
import pytest

import state_tensor_reference as ref
from scenarios import cloth_params

pytestmark = pytest.mark.gpu

GRIDS = {0: (3, 5), 1: (8, 8), 2: (9, 7), 3: (17, 16), 5: (64, 64)}
SHIRT, EMPTY, GRASPED = 4, 6, 3
FULL = [0, 1, 2, 3, 4, 5]
PERMUTED = [5, 0, 3, 4, 3, 1, 2]   # any order, one repeat
STREAM_FORMS = (4, 5, 6, 7, 9, 10, 11, 12)   # FS_FORM_STREAM_* (include/flingsim.h)


def _prepare(sim, shirt, slots=FULL, grasp=(GRASPED,)):
    """The listed slots of the standing layout: scenes, two frames, two pickers each, `grasp` moved by a movep that is cut off
    at its step limit (picker 0 keeps its particle), two more frames."""
    from flingbot_amd.sim import MoveLimitError

    for e in slots:
        if e == SHIRT:
            sim.set_scene(e, shirt[0], *shirt[1])
        else:
            sim.set_scene(e, cloth_params(*GRIDS[e]))
    sim.step_list(slots, 2)
    targets = {}
    for e in slots:
        pos = sim.get_positions(e).reshape(-1, 4)
        p = pos[len(pos) // 3, :3].astype(np.float64)
        centres = [p + [0.0, 0.01, 0.0], np.array([0.5, 0.5, -0.5])]
        for c in centres:
            sim.add_sphere(e, 0.02, c, [1, 0, 0, 0])
        sim.set_shape_states(e, np.array([np.hstack([c, c, [1, 0, 0, 0], [1, 0, 0, 0]]) for c in centres]))
        sim.picker_reset(e, 0.005, 0.00625, picker_radius=0.02)
        targets[e] = [p + [0.06, 0.3, 0.05], [0.3, 0.4, -0.3]]
    held = [e for e in slots if e in grasp]
    if held:
        with pytest.raises(MoveLimitError):
            sim.movep(held, [targets[e] for e in held], [[1, 0]] * len(held), speed=0.01, limit=4)
    sim.step_list(slots, 2)


@pytest.fixture(scope="module")
def shirt(tmp_path_factory):
    from test_fork_gpu import _shirt

    return _shirt(tmp_path_factory.mktemp("shirt"))


@pytest.fixture(scope="module")
def standing(gpu_required, shirt):
    """(context, reference): the reference is read through the getters ONCE; no test that takes this fixture changes the state."""
    from flingbot_amd import sim as fsim

    sim = fsim.FlingSim(n_envs=7, solver=fsim.FS_SOLVER_AUTO)
    _prepare(sim, shirt)
    want = {e: dict(pos4=sim.get_positions(e).reshape(-1, 4).copy(), vel3=sim.get_velocities(e).reshape(-1, 3).copy(),
                    phase=sim.get_phases(e).copy()) for e in FULL}
    assert (want[GRASPED]["pos4"][:, 3] == 0).sum() == 1, "one pinned particle"
    assert all(np.abs(w["vel3"]).max() > 0 for w in want.values()), "non-zero velocities"
    counts = [w["pos4"].shape[0] for w in want.values()]
    assert {15, 63, 64, 272, 4096} <= set(counts) and max(counts) == 4096
    yield sim, want
    sim.close()


def _packed(want, envs, n_max):
    return dict(pos4=ref.pack_rows([want[e]["pos4"] for e in envs], n_max)[0],
                vel3=ref.pack_rows([want[e]["vel3"] for e in envs], n_max)[0],
                phase=ref.pack_rows([want[e]["phase"] for e in envs], n_max, np.int32)[0],
                counts=np.array([want[e]["pos4"].shape[0] for e in envs], np.int32))


def _assert_state(st, exp, what):
    """Whatever fields `st` holds against the packed reference, bit for bit; the padded rows are zeros in every lane."""
    assert np.array_equal(st.counts, exp["counts"]) and st.counts.dtype == np.int32, what
    live = ref.mask(exp["counts"], exp["pos4"].shape[1])
    if st.pos4 is not None:
        assert np.array_equal(ref.bits(st.pos4.cpu().numpy()), ref.bits(exp["pos4"])), (what, "pos4")
    if st.vel4 is not None:
        v = st.vel4.cpu().numpy()
        assert np.array_equal(ref.bits(v[..., :3]), ref.bits(exp["vel3"])), (what, "vel4")
        assert not ref.bits(v)[~live].any(), (what, "vel4 tail")
    if st.phase is not None:
        assert np.array_equal(st.phase.cpu().numpy(), exp["phase"]), (what, "phase")
    assert np.array_equal(st.mask.cpu().numpy(), live), (what, "mask")


# ---- gather ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, 37], ids=["n_max = largest count", "n_max larger"])
def test_gather_equals_the_getters_inside_a_guarded_arena(standing, extra):
    """Test 1: permuted list with a repeat; outputs carved out of a poisoned allocation with guard bands; under both poisons no
    guard byte changes and every output byte is written (none keeps the poison in both runs)."""
    import torch
    from guarded_calls import Arena, Slot, unwritten

    sim, want = standing
    n, n_max = len(PERMUTED), 4096 + extra
    exp = _packed(want, PERMUTED, n_max)
    still, slots = {}, None
    for poison in ("A", "B"):
        slots = [Slot("d_pos4", 16 * n * n_max, "out"), Slot("d_vel4", 16 * n * n_max, "out"), Slot("d_phase", 4 * n * n_max, "out")]
        arena = Arena(torch.device("cuda", sim.device), slots, poison=poison, entry="fs_state_gather", seed=3)
        out = (arena.typed(0, torch.float32, (n, n_max, 4)), arena.typed(1, torch.float32, (n, n_max, 4)),
               arena.typed(2, torch.int32, (n, n_max)))
        st = sim.state_tensors(PERMUTED, phases=True, n_max=n_max, out=out)
        assert st.pos4.data_ptr() == arena.ptr(0) and st.vel4.data_ptr() == arena.ptr(1) and st.phase.data_ptr() == arena.ptr(2)
        arena.check_guards()
        _assert_state(st, exp, ("poison", poison, extra))
        pinned = ((st.inv_mass == 0) & st.mask).sum(1).tolist()
        assert pinned == [0, 0, 1, 0, 1, 0, 0], pinned   # the grasped cloth, listed twice
        still[poison] = {k: arena.still_poisoned(k).clone() for k in range(3)}
    unwritten("fs_state_gather", slots, still["A"], still["B"])
    fresh = sim.state_tensors(PERMUTED, phases=True) if extra == 0 else sim.state_tensors(PERMUTED, phases=True, n_max=n_max)
    _assert_state(fresh, exp, "fresh tensors")


def test_gather_right_after_step_list_sees_the_stepped_state(gpu_required):
    """Test 2: the launch is ordered behind the frames queued on the context's stream."""
    from flingbot_amd import sim as fsim

    sim = fsim.FlingSim(n_envs=3, solver=fsim.FS_SOLVER_AUTO)
    try:
        slots = [1, 3, 5]
        for k, e in enumerate(slots):
            sim.set_scene(k, cloth_params(*GRIDS[e]))
        sim.step_list([0, 1, 2], 2)
        sim.sync()
        sim.step_list([0, 1, 2], 6)
        queued = sim.state_tensors([2, 0, 1], phases=True)   # no sync in between
        sim.sync()
        settled = sim.state_tensors([2, 0, 1], phases=True)
        for a, b in zip(queued[:3], settled[:3]):
            assert np.array_equal(ref.bits(a.cpu().numpy()), ref.bits(b.cpu().numpy()))
        exp = ref.pack_from_getters(sim, [2, 0, 1])
        _assert_state(queued, exp, "against the getters")
    finally:
        sim.close()


@pytest.mark.parametrize("fields", [("pos4",), ("vel4",), ("phase",), ("pos4", "vel4"), ("pos4", "phase"), ("vel4", "phase")],
                         ids=lambda f: "+".join(f))
def test_gather_of_single_fields_and_pairs(standing, fields):
    """Test 3."""
    sim, want = standing
    st = sim.state_tensors(PERMUTED, positions="pos4" in fields, velocities="vel4" in fields, phases="phase" in fields)
    for name in ("pos4", "vel4", "phase"):
        assert (getattr(st, name) is not None) == (name in fields), name
    _assert_state(st, _packed(want, PERMUTED, 4096), fields)


def test_gathered_tensors_agree_with_the_device_reductions(standing):
    """Test 7: min / max of y and the largest |velocity component| over an episode's rows are exact operations, so they equal
    fs_cloth_stats bit for bit."""
    import torch

    sim, _ = standing
    st = sim.state_tensors(FULL)
    inf = torch.tensor(float("inf"), device=st.pos4.device)
    y = st.positions[..., 1]
    lo = torch.where(st.mask, y, inf).min(dim=1).values
    hi = torch.where(st.mask, y, -inf).max(dim=1).values
    vm = torch.where(st.mask[..., None], st.velocities.abs(), torch.zeros_like(inf)).amax(dim=(1, 2))
    got = torch.stack([lo, hi, vm], dim=1).cpu().numpy()
    assert np.array_equal(ref.bits(got), ref.bits(sim.cloth_stats(FULL)))


def test_topology_tensors_are_the_getters(standing):
    import torch

    sim, _ = standing
    for e in (GRASPED, SHIRT):
        t = sim.topology_tensors(e)
        assert all(x.is_cuda for x in t) and t.springs.dtype == torch.int64 and t.faces.dtype == torch.int64
        assert np.array_equal(t.springs.cpu().numpy(), sim.get_edges(e).reshape(-1, 2))
        assert np.array_equal(t.faces.cpu().numpy(), sim.get_faces(e).reshape(-1, 3))
        assert np.array_equal(t.rest_lengths.cpu().numpy(), sim.get_spring_lengths(e))
        assert np.array_equal(t.stiffness.cpu().numpy(), sim.get_spring_stiffness(e))
        assert np.array_equal(t.rest_positions.cpu().numpy(), sim.get_restPositions(e).reshape(-1, 4))
        assert t.springs.shape[0] == sim.n_springs(e) and t.rest_positions.shape[0] == sim.n_particles(e)


# ---- scatter ---------------------------------------------------------------------------------------------------------------------
def _new_state(sim, envs, seed):
    """Numbers to write into the listed episodes: their own state moved a little (the inverse masses, a grasp's zero among them,
    stay), per episode {pos4 [N, 4], vel3 [N, 3]} float32."""
    rng = np.random.RandomState(seed)
    out = {}
    for e in envs:
        p = sim.get_positions(e).reshape(-1, 4).copy()
        p[:, :3] += rng.uniform(-2e-4, 2e-4, (p.shape[0], 3)).astype(np.float32)
        out[e] = dict(pos4=p, vel3=rng.uniform(-0.05, 0.05, (p.shape[0], 3)).astype(np.float32))
    return out


def _tensors(new, envs, n_max, device):
    """The scatter's input for `new`: the fourth velocity lane holds 7 (it must be stored as 0), the rows beyond a count NaN
    (they must not be read)."""
    import torch

    pos, counts = ref.pack_rows([new[e]["pos4"] for e in envs], n_max)
    vel = np.full((len(envs), n_max, 4), 7.0, np.float32)
    vel[..., :3] = ref.pack_rows([new[e]["vel3"] for e in envs], n_max)[0]
    tail = ~ref.mask(counts, n_max)
    pos[tail], vel[tail] = np.nan, np.nan
    return torch.from_numpy(pos).to(device), torch.from_numpy(vel).to(device)


@pytest.mark.parametrize("path", ["fused grid-64", "streams"])
def test_scatter_equals_the_per_episode_setters(gpu_required, shirt, path):
    """Test 4: two identically prepared contexts; A takes the new state through set_positions / set_velocities per episode, B
    through one set_state_tensors; three frames later positions and velocities are equal bit for bit.  Once with a launch in
    the fused grid-64 form (the 64 x 64 cloth alone, under the co-tenant rule), once with a streaming launch of all cloths."""
    import torch
    from flingbot_amd import sim as fsim

    solver, listed = {"fused grid-64": (fsim.FS_SOLVER_COTENANT, [5]), "streams": (fsim.FS_SOLVER_STREAM, [3, 5, 0, 4, 2, 1])}[path]
    a, b = fsim.FlingSim(n_envs=7, solver=solver), fsim.FlingSim(n_envs=7, solver=solver)
    try:
        _prepare(a, shirt)
        _prepare(b, shirt)
        new = _new_state(a, listed, seed=11)
        for e in listed:
            a.set_positions(e, new[e]["pos4"])
            a.set_velocities(e, new[e]["vel3"])
        pos4, vel4 = _tensors(new, listed, 4096 + 5, torch.device("cuda", b.device))
        b.set_state_tensors(listed, pos4=pos4, vel4=vel4)
        back = b.state_tensors(listed, n_max=4096 + 5)
        _assert_state(back, ref.pack_from_getters(a, listed, 4096 + 5), "right after the scatter")
        assert not back.vel4[..., 3].any(), "the fourth velocity lane is stored as 0"
        a.step_list(listed, 3)
        b.step_list(listed, 3)
        form = b.last_kernel_form()
        assert a.last_kernel_form() == form
        if path == "fused grid-64":
            assert form == fsim.FS_FORM_FUSED_GRID64, form
        else:
            assert form in STREAM_FORMS, form
        for e in FULL:   # the listed ones stepped, the others as prepared: equal either way
            assert np.array_equal(ref.bits(a.get_positions(e)), ref.bits(b.get_positions(e))), (path, e, "positions")
            assert np.array_equal(ref.bits(a.get_velocities(e)), ref.bits(b.get_velocities(e))), (path, e, "velocities")
            assert np.isfinite(b.get_positions(e)).all()
        # one field at a time: the other one stays
        before = b.state_tensors(listed)
        b.set_state_tensors(listed, vel4=torch.zeros_like(before.vel4))
        after = b.state_tensors(listed)
        assert torch.equal(after.pos4, before.pos4) and not after.vel4.any()
        b.set_state_tensors(listed, pos4=before.pos4)
        assert torch.equal(b.state_tensors(listed, velocities=False).pos4, before.pos4)
    finally:
        a.close()
        b.close()


def test_scatter_into_forks_that_were_stepped_apart(gpu_required):
    """Test 5: the fork's own contract reached through tensors -- gather from the sources, scatter into their forks after those
    ran ahead, step both: identical bits."""
    from flingbot_amd import sim as fsim

    sim = fsim.FlingSim(n_envs=4, solver=fsim.FS_SOLVER_AUTO)
    try:
        src, dst = [0, 1], [2, 3]
        sim.set_scene(0, cloth_params(17, 16))
        sim.set_scene(1, cloth_params(64, 64))
        sim.step_list(src, 3)
        sim.fork(src, dst)
        sim.step_list(dst, 4)
        assert not np.array_equal(ref.bits(sim.get_positions(0)), ref.bits(sim.get_positions(2)))
        st = sim.state_tensors(src)
        sim.set_state_tensors(dst, pos4=st.pos4, vel4=st.vel4)
        sim.step_list(src + dst, 3)
        for s, d in zip(src, dst):
            assert np.array_equal(ref.bits(sim.get_positions(s)), ref.bits(sim.get_positions(d))), (s, d)
            assert np.array_equal(ref.bits(sim.get_velocities(s)), ref.bits(sim.get_velocities(d))), (s, d)
    finally:
        sim.close()


def test_scatter_of_a_tensor_produced_on_another_torch_stream(gpu_required):
    """Test 6: the tensor is still being produced on a non-default torch stream when the call is made."""
    import torch
    from flingbot_amd import sim as fsim

    def produce(base):   # a queue of exact copies in front of the result
        t = base.clone()
        for _ in range(200):
            t = t.roll(1, 1).roll(-1, 1)
        return t + 0.0

    def run(stream):
        sim = fsim.FlingSim(n_envs=2, solver=fsim.FS_SOLVER_AUTO)
        try:
            sim.set_scene(0, cloth_params(17, 16))
            sim.set_scene(1, cloth_params(64, 64))
            sim.step_list([0, 1], 2)
            new = _new_state(sim, [0, 1], seed=23)
            pos4, vel4 = _tensors(new, [0, 1], 4096, torch.device("cuda", sim.device))
            torch.cuda.synchronize()
            if stream is None:
                sim.set_state_tensors([0, 1], pos4=produce(pos4), vel4=produce(vel4))
            else:
                with torch.cuda.stream(stream):
                    sim.set_state_tensors([0, 1], pos4=produce(pos4), vel4=produce(vel4))
            sim.step_list([0, 1], 2)
            return [ref.bits(sim.get_positions(e)).copy() for e in (0, 1)] + [ref.bits(sim.get_velocities(e)).copy() for e in (0, 1)]
        finally:
            sim.close()

    want = run(None)
    got = run(torch.cuda.Stream())
    for w, g in zip(want, got):
        assert np.array_equal(w, g)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _c_gather(sim, envs, n_max, pos4=None, vel4=None, phase=None):
    """Straight to the C entry: FlingSimError with fs_last_error on a refusal."""
    ids, counts = np.asarray(envs, np.int32), np.zeros(len(envs), np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))   # noqa: E731
    sim._ck(sim.lib.fs_state_gather(sim.h, ids.size, ip(ids), int(n_max), _ptr(pos4), _ptr(vel4), _ptr(phase), ip(counts)))
    return counts


def _c_scatter(sim, envs, n_max, pos4=None, vel4=None):
    ids = np.asarray(envs, np.int32)
    sim._ck(sim.lib.fs_state_scatter(sim.h, ids.size, ids.ctypes.data_as(C.POINTER(C.c_int)), int(n_max), _ptr(pos4), _ptr(vel4)))


def test_refusals_name_their_reason_and_change_nothing(standing):
    """Test 8 (argument checks on the host; nothing here launches a kernel on bad input)."""
    import torch
    from flingbot_amd import sim as fsim

    sim, want = standing
    exp = _packed(want, FULL, 4096)
    dev = torch.device("cuda", sim.device)
    canary = 123.0
    p = torch.full((3, 4096, 4), canary, device=dev)
    v = torch.full((3, 4096, 4), canary, device=dev)

    def unchanged(what):
        _assert_state(sim.state_tensors(FULL, phases=True), exp, what)
        assert bool((p == canary).all()) and bool((v == canary).all()), what

    refusals = [
        ("no scene", lambda: sim.state_tensors([0, EMPTY])),
        ("no scene", lambda: _c_gather(sim, [0, EMPTY, 1], 4096, p, v)),
        ("no scene", lambda: _c_scatter(sim, [0, EMPTY, 1], 4096, p, v)),
        ("out of range", lambda: sim.state_tensors([0, 7])),
        ("out of range", lambda: _c_gather(sim, [0, 7, 1], 4096, p, v)),
        ("out of range", lambda: _c_gather(sim, [0, -1, 1], 4096, p, v)),
        ("out of range", lambda: _c_scatter(sim, [0, 1, 7], 4096, p, v)),
        ("n_max 4095 is below the 4096 particles of episode 5", lambda: _c_gather(sim, [0, 5, 1], 4095, p, v)),
        ("n_max 271 is below the 272 particles of episode 3", lambda: _c_gather(sim, [3, 3, 3], 271, p, v)),
        ("n_max 4095 is below the 4096 particles of episode 5", lambda: _c_scatter(sim, [0, 5, 1], 4095, p, v)),
        ("destination 3 is listed twice", lambda: _c_scatter(sim, [3, 1, 3], 4096, p, v)),
        ("all null", lambda: _c_gather(sim, [0, 1, 2], 4096)),
        ("both null", lambda: _c_scatter(sim, [0, 1, 2], 4096)),
    ]
    for reason, call in refusals:
        with pytest.raises(fsim.FlingSimError, match=reason):
            call()
        unchanged(reason)
    with pytest.raises(ValueError, match="listed twice"):
        sim.set_state_tensors([3, 1, 3], pos4=p, vel4=v)
    with pytest.raises(ValueError, match="n_max 4095"):
        sim.set_state_tensors([0, 5, 1], pos4=p[:, :4095].contiguous())
    unchanged("python-side refusals")
    assert _c_gather(sim, [0, 5, 1], 4096, p, v).tolist() == [15, 4096, 64]   # the same calls are taken once they fit


def test_scatter_is_refused_while_an_advance_ticket_is_open_on_a_listed_episode(gpu_required):
    """Test 8, the lane guard of fs_set_positions / fs_set_velocities: between advance_begin and advance_end a call on the
    service lane must not rewrite an episode of the chunk in flight; its neighbour is free, and a gather is always allowed."""
    import torch
    from flingbot_amd import sim as fsim

    def make():
        s = fsim.FlingSim(n_envs=2, solver=fsim.FS_SOLVER_AUTO)
        for e in (0, 1):
            s.set_scene(e, cloth_params(17, 16))
        s.step_list([0, 1], 2)
        for e in (0, 1):
            for c in ([0.5, 0.5, -0.5], [-0.5, 0.5, -0.5]):
                s.add_sphere(e, 0.02, c, [1, 0, 0, 0])
            s.picker_reset(e)
        return s

    sim, control = make(), make()
    try:
        before = sim.state_tensors([0, 1])
        z, gr = np.zeros((1, 2, 3)), np.zeros((1, 2), int)
        ticket, prog, status, steps = sim.advance_begin([0], [2], z, gr, [0.0], [6], [-1], [0], [0], cap_min=6, cap=6)
        sim.service_lane(True)
        try:
            for envs in ([0, 1], [1, 0], [0]):
                with pytest.raises(fsim.FlingSimError, match="in flight"):
                    sim.set_state_tensors(envs, pos4=before.pos4[:len(envs)].contiguous(), vel4=before.vel4[:len(envs)].contiguous())
            assert torch.equal(sim.state_tensors([1]).pos4, before.pos4[1:2])   # the refused lists wrote nothing into episode 1 ...
            sim.set_state_tensors([1], pos4=before.pos4[1:2].contiguous() + 0.0)   # ... which is free
        finally:
            sim.service_lane(False)
        prog, status, steps = sim.advance_end(ticket, prog, status, steps)
        assert prog.tolist() == [6] and status.tolist() == [1]
        control.step_list([0], 6)
        _assert_state(sim.state_tensors([0, 1], phases=True), ref.pack_from_getters(control, [0, 1]), "the refused calls changed nothing")
        sim.set_state_tensors([0, 1], pos4=before.pos4, vel4=before.vel4)   # nothing in flight any more
        after = sim.state_tensors([0, 1])
        assert torch.equal(after.pos4, before.pos4) and torch.equal(after.vel4[..., :3], before.vel4[..., :3])
    finally:
        sim.close()
        control.close()
