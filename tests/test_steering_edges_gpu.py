"""The episode-steering kernels of flingbot_amd/csrc/fs_loops.hip (fs_k_cloth_stats, fs_k_stretch_probe, fs_k_max_displacement,
fs_k_stable_check, fs_k_set_particles) and fs_k_wait_check's tolerance rule on the constructed particle sets of
tests/steering_cases.py, through FlingSim's public methods.  Every comparison with the float32 restatements is exact: bits for
floats, isnan where the restatement gives NaN, values for +-0, equality for flags and indices.  Every read-only call is made
twice and must repeat itself, and leaves positions and velocities as they were."""
import numpy as np
import pytest

import steering_cases as sc
from scenarios import cloth_params

pytestmark = pytest.mark.gpu
F = np.float32
SMALL = [c["name"] for c in sc.CASES if c["op"] != "stable" and c["n"] != sc.BIG]
STABLE = [c["name"] for c in sc.CASES if c["op"] == "stable"]
_shared = {}


def _u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _eq(got, want):
    """One float32: NaN where NaN is expected, equal as values where 0 is expected, else the same bits."""
    got, want = F(got), F(want)
    if want != want:
        return bool(got != got)
    return bool(got == want) if want == 0 else got.tobytes() == want.tobytes()


def _scene(ctx, e, n):
    ctx.set_scene(e, cloth_params(*sc.grid_for(n)))
    assert ctx.n_particles(e) == n


def _load(ctx, e, case):
    """The case's particle set into episode e (whose cloth has the case's n particles); for a displacement case the snapshot
    is taken of `pre`, then `pos` is set.  Nothing is stepped."""
    if case["op"] == "disp":
        ctx.set_positions(e, case["pre"].ravel())
        ctx.snapshot_positions([e])
    ctx.set_positions(e, case["pos"].ravel())
    ctx.set_velocities(e, case["vel"].ravel())


def _run(ctx, ids, cases):
    """The operation of `cases` (all of one op) over the episodes `ids` in one call -> one tuple per row."""
    op = cases[0]["op"]
    if op == "stats":
        return [tuple(r) for r in ctx.cloth_stats(ids)]
    if op == "probe":
        single, near = ctx.stretch_probe(ids, np.stack([c["mid"] for c in cases]), np.array([c["thr"] for c in cases], F))
        assert single.dtype == bool and near.dtype == F
        return [(bool(s),) + tuple(p) for s, p in zip(single, near)]
    return [(d,) for d in ctx.max_displacement(ids)]


def _want(case):
    if case["op"] == "stats":
        return sc.stats(case["pos"], case["vel"])
    if case["op"] == "probe":
        single, idx = sc.probe(case["pos"], case["mid"], case["thr"])
        return (single,) + tuple(case["pos"][idx, :3])
    return (sc.displacement(case["pos"], case["pre"]),)


def _check(name, got, want):
    print(f"{name}: kernel {got!r} restatement {want!r}")
    assert len(got) == len(want), name
    for g, w in zip(got, want):
        assert (g == w) if isinstance(w, bool) else _eq(g, w), (name, got, want)


def _unchanged(ctx, e, case):
    assert np.array_equal(_u32(ctx.get_positions(e)), _u32(case["pos"].ravel())), case["name"]
    assert np.array_equal(_u32(ctx.get_velocities(e)), _u32(case["vel"].ravel())), case["name"]


def _by_count():
    """One context with one cloth per particle count; every small read-only case is loaded into the cloth of its size."""
    if "by_count" not in _shared:
        from flingbot_amd import sim as fsim

        sizes = sorted({sc.BY_NAME[n]["n"] for n in SMALL})
        ctx = fsim.FlingSim(n_envs=len(sizes))
        for e, n in enumerate(sizes):
            _scene(ctx, e, n)
        _shared["by_count"] = (ctx, {n: e for e, n in enumerate(sizes)})
    return _shared["by_count"]


def teardown_module(module):
    for key in list(_shared):
        for c in _shared.pop(key)[:2 if key == "stable" else 1]:
            c.close()


@pytest.mark.parametrize("name", SMALL)
def test_case_equals_the_restatement(gpu_required, name):
    ctx, slot = _by_count()
    case = sc.BY_NAME[name]
    e = slot[case["n"]]
    _load(ctx, e, case)
    want = _want(case)
    first = _run(ctx, [e], [case])[0]
    _check(name, first, want)
    again = _run(ctx, [e], [case])[0]
    assert np.array_equal(_u32([float(x) for x in again]), _u32([float(x) for x in first])), (name, first, again)
    _unchanged(ctx, e, case)


@pytest.mark.parametrize("op", ["stats", "probe", "disp"])
def test_one_call_over_episodes_of_different_sizes_out_of_order(gpu_required, op):
    """Episodes of 2, 257, 64 and 1025 particles listed as [2, 0, 3, 1], each with its own midpoint, threshold and snapshot:
    every row is that episode's restatement and what the episode gives when it is called alone."""
    from flingbot_amd import sim as fsim

    cases = [sc.BY_NAME[n] for n in sc.BATCH[op]]
    ctx = fsim.FlingSim(n_envs=len(cases))
    for e, case in enumerate(cases):
        _scene(ctx, e, case["n"])
        _load(ctx, e, case)
    order = list(sc.BATCH_ORDER)
    listed = [cases[e] for e in order]
    rows = _run(ctx, order, listed)
    for k, e in enumerate(order):
        _check(f"{cases[e]['name']} as row {k}", rows[k], _want(cases[e]))
        alone = _run(ctx, [e], [cases[e]])[0]
        assert np.array_equal(_u32([float(x) for x in alone]), _u32([float(x) for x in rows[k]])), (k, e, alone, rows[k])
    again = _run(ctx, order, listed)
    assert np.array_equal(_u32(np.array(again, F)), _u32(np.array(rows, F)))
    for e, case in enumerate(cases):
        _unchanged(ctx, e, case)
    ctx.close()


def test_a_slot_without_a_scene_is_refused_and_the_outputs_stay(gpu_required):
    from flingbot_amd import sim as fsim
    from flingbot_amd.sim import FlingSimError, _fp, _ip

    ctx = fsim.FlingSim(n_envs=3)
    case = sc.BY_NAME["disp_n64_at63"]
    for e in (0, 2):
        _scene(ctx, e, 64)
        _load(ctx, e, case)
    ids = [0, 1, 2]
    with pytest.raises(FlingSimError):
        ctx.cloth_stats(ids)
    with pytest.raises(FlingSimError):
        ctx.stretch_probe(ids, np.zeros((3, 2), F), np.zeros(3, F))
    with pytest.raises(FlingSimError):
        ctx.max_displacement(ids)
    with pytest.raises(FlingSimError):
        ctx.snapshot_positions(ids)
    with pytest.raises(FlingSimError):
        ctx.wait_until_stable(ids, max_steps=1)
    with pytest.raises(FlingSimError):
        ctx.set_particles(ids, [0, 0, 0], np.zeros((3, 4), F))
    # the same calls on the C interface, with the outputs filled beforehand: an error return writes none of them
    idl = np.array(ids, np.int32)
    fout, iout, iout2 = np.full(9, -7.5, F), np.full(3, -7, np.int32), np.full(3, -7, np.int32)
    assert ctx.lib.fs_cloth_stats(ctx.h, 3, _ip(idl), _fp(fout), 9) < 0 and (fout == F(-7.5)).all()
    assert ctx.lib.fs_stretch_probe(ctx.h, 3, _ip(idl), _fp(np.zeros(6, F)), _fp(np.zeros(3, F)), _ip(iout), _fp(fout)) < 0
    assert (fout == F(-7.5)).all() and (iout == -7).all()
    assert ctx.lib.fs_max_displacement(ctx.h, 3, _ip(idl), _fp(fout), 9) < 0 and (fout == F(-7.5)).all()
    assert ctx.lib.fs_wait_until_stable(ctx.h, 3, _ip(idl), 1, 1e-2, _ip(iout), _ip(iout2)) < 0
    assert (iout == -7).all() and (iout2 == -7).all()
    for e in (0, 2):                                            # and the episodes that have a scene are as they were
        _unchanged(ctx, e, case)
        _check("after the refusals", _run(ctx, [e], [case])[0], _want(case))
    ctx.close()


def test_displacement_needs_a_snapshot_of_the_same_cloth_and_the_buffer_regrows(gpu_required):
    """One slot: no snapshot -> refused; 64 particles; then 16512 (more than the snapshot buffer holds at first: it is
    replaced by a larger one), where the decisive particle is the last; then 64 again, refused until a new snapshot is taken
    because set_scene changed n, and right afterwards."""
    from flingbot_amd import sim as fsim
    from flingbot_amd.sim import FlingSimError

    ctx = fsim.FlingSim(n_envs=1)
    small, big = sc.BY_NAME["disp_n64_at63"], sc.BY_NAME[f"disp_n{sc.BIG}_at{sc.BIG - 1}"]
    _scene(ctx, 0, 64)
    with pytest.raises(FlingSimError):
        ctx.max_displacement([0])
    for case in (small, big, small):
        if case is not small or ctx.n_particles(0) != 64:
            _scene(ctx, 0, case["n"])
            with pytest.raises(FlingSimError):                  # the snapshot is of a cloth with another n
                ctx.max_displacement([0])
        _load(ctx, 0, case)
        want = _want(case)
        for _ in range(2):
            _check(case["name"], _run(ctx, [0], [case])[0], want)
        _unchanged(ctx, 0, case)
    ctx.close()


# ---- the stable check: constructed velocities on the cloth as set_scene leaves it, max_steps <= 1
def _stable_ctx():
    """(context, twin context, {name: episode}, {name: (positions, velocities) at the start}): the twin holds the same
    episodes and only ever sees set_positions, set_velocities and step_list."""
    if "stable" not in _shared:
        from flingbot_amd import sim as fsim

        ctx, twin = fsim.FlingSim(n_envs=len(STABLE)), fsim.FlingSim(n_envs=len(STABLE))
        start = {}
        for e, name in enumerate(STABLE):
            for c in (ctx, twin):
                _scene(c, e, sc.BY_NAME[name]["n"])
            start[name] = (ctx.get_positions(e).copy(), sc.BY_NAME[name]["vel"].ravel().copy())
            assert np.array_equal(_u32(twin.get_positions(e)), _u32(start[name][0]))
        _shared["stable"] = (ctx, twin, {name: e for e, name in enumerate(STABLE)}, start)
    return _shared["stable"]


def _reset(names):
    ctx, twin, slot, start = _stable_ctx()
    for name in names:
        for c in (ctx, twin):
            c.set_positions(slot[name], start[name][0])
            c.set_velocities(slot[name], start[name][1])


def _state(c, e):
    return np.concatenate([_u32(c.get_positions(e)), _u32(c.get_velocities(e))])


def _stepped_like_the_twin(names, stepped):
    """Episodes that were found stable kept their bits (a retired id is skipped by the solver); the others hold the bits of
    the twin after step_list(.., 1)."""
    ctx, twin, slot, start = _stable_ctx()
    twin.step_list([slot[n] for n in names if stepped[n]], 1)
    for name in names:
        e = slot[name]
        if not stepped[name]:
            assert np.array_equal(_state(ctx, e), np.concatenate([_u32(start[name][0]), _u32(start[name][1])])), name
        else:
            assert np.array_equal(_state(ctx, e), _state(twin, e)), name
            assert not np.array_equal(_u32(ctx.get_positions(e)), _u32(start[name][0])), name


@pytest.mark.parametrize("name", STABLE)
def test_stable_check_alone(gpu_required, name):
    ctx, twin, slot, start = _stable_ctx()
    case = sc.BY_NAME[name]
    want = sc.stable(case["vel"], case["tol"], case["max_steps"])
    assert want == case["want"]
    _reset([name])
    got = ctx.wait_until_stable(slot[name], max_steps=case["max_steps"], tolerance=case["tol"])
    print(f"{name}: kernel {got!r} restatement {want!r}")
    assert got == want, (name, got, want)
    _stepped_like_the_twin([name], {name: want[1] == 1})


def test_stable_check_mixed_call(gpu_required):
    """Stable-at-entry and unstable episodes of 64, 255 and 1024 particles in one call."""
    ctx, twin, slot, start = _stable_ctx()
    names = list(sc.STABLE_MIX)
    want = [sc.BY_NAME[n]["want"] for n in names]
    assert len({w[0] for w in want}) == 2 and len({sc.BY_NAME[n]["n"] for n in names}) == 3
    _reset(names)
    stable, steps = ctx.wait_until_stable([slot[n] for n in names], max_steps=1, tolerance=sc.TOL)
    assert stable.tolist() == [w[0] for w in want] and steps.tolist() == [w[1] for w in want], (stable, steps)
    _stepped_like_the_twin(names, {n: w[1] == 1 for n, w in zip(names, want)})


def test_advance_waiters_state_the_same_rule(gpu_required):
    """The tolerance-edge velocities through fs_advance's wait entries (kind 1, fs_k_wait_check), budget 1: stable -> status 1
    without a step, else one step and status 2 (finished at the limit)."""
    ctx, twin, slot, start = _stable_ctx()
    names = ["stable_one_below", "stable_at_float32_tol", "stable_one_above", "stable_zero", "stable_nan"]
    want = [sc.BY_NAME[n]["want"] for n in names]
    _reset(names)
    k = len(names)
    prog, status, steps = ctx.advance([slot[n] for n in names], [1] * k, np.zeros((k, 2, 3)), np.zeros((k, 2), int), [0.0] * k,
                                      [1] * k, [-1] * k, [0] * k, [0] * k, tolerance=sc.TOL)
    print("advance:", names, prog, status, steps)
    assert status.tolist() == [1 if w[0] else 2 for w in want]
    assert prog.tolist() == steps.tolist() == [w[1] for w in want]
    _stepped_like_the_twin(names, {n: w[1] == 1 for n, w in zip(names, want)})


# ---- fs_set_particles
def test_set_particles_writes_one_particle_per_episode(gpu_required):
    from flingbot_amd import sim as fsim
    from flingbot_amd.sim import FlingSimError

    ctx = fsim.FlingSim(n_envs=len(sc.SET_SIZES))
    state = []
    for e, n in enumerate(sc.SET_SIZES):
        _scene(ctx, e, n)
        pos, vel = sc.base(n)
        ctx.set_positions(e, pos.ravel())
        ctx.set_velocities(e, vel.ravel())
        state.append((pos, vel))
    ids = [2, 0, 1]                                             # listed out of order; the arguments follow the list
    pids, pos4 = [sc.SET_PIDS[e] for e in ids], np.stack([sc.SET_POS4[e] for e in ids])
    for zero, p4 in ((False, pos4), (True, pos4 + F(0.25))):
        ctx.set_particles(ids, pids, p4, zero_velocity=zero)
        for k, e in enumerate(ids):
            state[e] = sc.set_particle(state[e][0], state[e][1], pids[k], p4[k], zero)
        for e in range(len(ids)):
            assert np.array_equal(_u32(ctx.get_positions(e)), _u32(state[e][0].ravel())), (zero, e)
            assert np.array_equal(_u32(ctx.get_velocities(e)), _u32(state[e][1].ravel())), (zero, e)
    assert all((state[e][1][sc.SET_PIDS[e]] == 0).all() for e in range(3))
    for bad in ([sc.SET_SIZES[2], 0, 0], [0, -1, 0], [0, 0, sc.SET_SIZES[1]]):     # pid = n and pid = -1: nothing is written
        with pytest.raises(FlingSimError):
            ctx.set_particles(ids, bad, pos4 - F(1.0), zero_velocity=True)
        for e in range(len(ids)):
            assert np.array_equal(_u32(ctx.get_positions(e)), _u32(state[e][0].ravel())), (bad, e)
            assert np.array_equal(_u32(ctx.get_velocities(e)), _u32(state[e][1].ravel())), (bad, e)
    ctx.close()
