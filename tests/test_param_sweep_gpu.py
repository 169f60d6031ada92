"""Every shipped solver form against the oracle under NON-DEFAULT parameter tables (tests/param_cases.py).

The rest of the suite compares the kernels with the oracle under FlingBot's table only, which is made of identities
(relaxation 1, damping 1, particle friction 1, static friction 0, gravity along y, the plane y = 0, solidRestDistance =
radius, no speed clamp, 30 iterations, 4 substeps).  tests/test_param_sweep_cpu.py shows that in the scene used here every
slot of the ALL table, one at a time, changes the oracle's bits; here every form runs that scene under ALL and under tables
that differ per episode of one launch, and positions, velocities, neighbour counts and lists and shape-candidate masks equal
the oracle's bit for bit.  The form is asserted through last_kernel_form().  In the per-form launches the EDGES tables only
ride along (which one an episode holds follows from its index, and the large launches compare three episodes); what compares
each EDGES table is test_every_shared_edges_table, test_substep_and_iteration_counts and test_list_caps, on the form classes
grid-64, coded fused, latency streaming and grid-L streaming.

Forms of include/flingsim.h's FS_FORM_* list: all 12 are launched (test_every_form_*).  FS_FORM_STREAM_GRIDL is launched in
its positive-stiffness and general-spring instantiations and with the split and the merged substep boundary.
"""
import numpy as np
import pytest

import list_sort_scenes as L
import param_cases as P
from test_shipped_kernels_gpu import _oracle_runs

pytestmark = pytest.mark.gpu


def _tables(mode, n, counts=None):
    """Per-episode tables of a launch.  "mixed": FlingBot's table, ALL with FlingBot's counts, and the EDGES tables that
    keep those counts in turn -- one launch holds different tables; "all": ALL in every episode.  counts = (substeps,
    iterations) overrides both in every episode (episodes stepped together must share them)."""
    if mode == "all":
        out = [P.ALL] * n
    else:
        out = [(P.DEFAULT, P.ALL_SHARED, P.EDGES[P.EDGES_SHARED[(e // 3) % len(P.EDGES_SHARED)]][0])[e % 3] for e in range(n)]
    return [P.with_counts(t, *counts) for t in out] if counts else out


def _run_launch(solver, kinds, tables, n_frames, sample, form, tmp_path, slot_forms=None):
    from flingbot_amd import sim as fsim

    ctx = fsim.FlingSim(n_envs=len(kinds), solver=solver)
    try:
        for e, kind in enumerate(kinds):
            P.scene(ctx.env(e), seed=e, table=tables[e], **P.cloth(kind, tmp_path))
        for _ in range(n_frames):
            for e in range(len(kinds)):
                P.move_spheres(ctx.env(e))
            ctx.step(1)  # one launch (fused) / one launch sequence (streaming) for all episodes
            assert ctx.last_kernel_form() == form, ctx.last_kernel_form()
        if slot_forms is not None:
            assert ctx.last_slot_forms() == slot_forms, ctx.last_slot_forms()

        def setup(e):
            def go(orc):
                P.scene(orc, seed=e, table=tables[e], **P.cloth(kinds[e], tmp_path))
                P.frames(orc, n_frames)
            return go

        orcs = _oracle_runs([setup(e) for e in sample], 0)
        for e, orc in zip(sample, orcs):
            assert np.array_equal(ctx.get_params(e).view(np.uint32), orc.get_params().view(np.uint32)), e
            L.compare(ctx, e, orc, f"form {form}, {kinds[e]}, episode {e} of {len(kinds)}")
    finally:
        ctx.close()


# id: (solver, kinds of the episodes, FS_FORM_*).  Launch sizes: the smallest that select the form (fs_solver.hip).
FORMS = {
    "fused_grid64_64x8": (2, ["64x8"] * 3, "FUSED_GRID64"),
    "fused_grid64_64x64": (2, ["64x64"] * 3, "FUSED_GRID64"),
    "fused_12": (5, ["16x16"] * 3, "FUSED_12"),
    "fused_16": (2, ["deg16"] * 3, "FUSED_16"),
    "fused_generic": (3, ["16x16"] * 3, "FUSED_GENERIC"),
    "stream_eager": (6, ["16x16"] * 3, "STREAM_EAGER"),
    "stream_gridl_positive": (1, ["16x16"] * 3, "STREAM_GRIDL"),       # fs_k_iterate_gridl<true>
    "stream_gridl_tether": (1, ["16x16", "16x16t", "16x16"], "STREAM_GRIDL"),  # one tether stiffness: fs_k_iterate_gridl<false>
    "stream_gridl_split": (7, ["16x16"] * 3, "STREAM_GRIDL"),
    "stream_gridl_merged": (8, ["16x16"] * 3, "STREAM_GRIDL"),
    "stream_coded": (6, ["64x64"] * 36, "STREAM_CODED"),               # above 32 x 4096 particles, below 96 x 4096
    "stream_ell": (4, ["64x64"] * 36, "STREAM_ELL"),
    "stream_grid": (6, ["64x64"] * 96, "STREAM_GRID"),                 # from 96 x 4096 particles on
    "stream_gridl_tp": (1, ["64x64"] * 66, "STREAM_GRIDL_TP"),         # above 262 144 particles
    "stream_mesh": (10, ["shirt"] * 3, "STREAM_MESH"),
    "stream_mixed": (10, ["shirt", "16x16", "shirt"], "STREAM_MIXED"),
}


@pytest.mark.parametrize("mode", ["mixed", "all"])
@pytest.mark.parametrize("case", sorted(FORMS))
def test_every_form_under_changed_tables(gpu_required, tmp_path, case, mode):
    """4e: each form at the smallest launch that selects it, six frames of the scene; "mixed": FlingBot's table, ALL (with
    FlingBot's counts) and an EDGES table alternate over the episodes of ONE launch; "all": ALL (7 iterations -- odd --, 3
    substeps) everywhere.  The large launches exist only because their form needs the particle count: three sampled
    episodes (first, second, last: one of each table); the small ones compare every episode."""
    from flingbot_amd import sim as fsim

    solver, kinds, form = FORMS[case]
    n = len(kinds)
    sample = list(range(n)) if n <= 3 else [0, 1, n - 1]
    assert n <= 3 or (n - 1) % 3 == 2  # the last episode holds an EDGES table
    slot_forms = None
    if case == "stream_mixed":
        slot_forms = [fsim.FS_FORM_STREAM_MESH, fsim.FS_FORM_STREAM_GRIDL_TP, fsim.FS_FORM_STREAM_MESH]
    _run_launch(solver, kinds, _tables(mode, n), 6, sample, getattr(fsim, "FS_FORM_" + form), tmp_path, slot_forms)


@pytest.mark.parametrize("name", P.EDGES_SHARED)
@pytest.mark.parametrize("case", sorted(["fused_grid64", "fused_12", "stream_eager", "stream_gridl"]))
def test_every_shared_edges_table(gpu_required, tmp_path, case, name):
    """4e, the EDGES tables one by one: every table that keeps FlingBot's counts -- maxNeighbors 1 ... 17, maxContacts 0 (nothing
    is listed: the sheet falls through plane and spheres) and 1 (plane only), the three frictions 0, relaxation 1.5, damping
    0, sleep threshold 0, the speed clamp that never binds -- on each form class, next to FlingBot's table and ALL in the
    same launch; every episode is compared."""
    from flingbot_amd import sim as fsim

    solver, kind, form = COUNT_FORMS[case]
    tables = [P.EDGES[name][0], P.DEFAULT, P.ALL_SHARED, P.EDGES[name][0]]
    _run_launch(solver, [kind] * 4, tables, 6, [0, 1, 2, 3], getattr(fsim, "FS_FORM_" + form), tmp_path)


COUNT_FORMS = {"fused_grid64": (2, "64x8", "FUSED_GRID64"), "fused_12": (5, "16x16", "FUSED_12"),
               "stream_eager": (6, "16x16", "STREAM_EAGER"), "stream_gridl": (1, "16x16", "STREAM_GRIDL")}


# (9 substeps: fused forms only -- the streaming side is test_streaming_refuses_nine_substeps)
COUNT_CASES = [(c, s, i) for c in sorted(COUNT_FORMS) for s, i in [(1, 1), (8, 3), (3, 0), (3, 7), (9, 2)]
               if s <= 8 or c.startswith("fused")]


@pytest.mark.parametrize("case,substeps,iterations", COUNT_CASES)
def test_substep_and_iteration_counts(gpu_required, tmp_path, case, substeps, iterations):
    """4f: one substep and one iteration; 8 substeps (the last row of the streaming sweep table); no iteration at all; an odd
    count (the Jacobi ping-pong ends in the other buffer).  9 substeps: the fused kernels index nothing by substep
    (fs_shape_sweep takes the substep as a number) and run them; the streaming back-end refuses (next test)."""
    from flingbot_amd import sim as fsim

    solver, kind, form = COUNT_FORMS[case]
    tables = _tables("mixed", 3, counts=(substeps, iterations))
    _run_launch(solver, [kind] * 3, tables, 6, [0, 1, 2], getattr(fsim, "FS_FORM_" + form), tmp_path)


def test_streaming_refuses_nine_substeps(gpu_required, tmp_path):
    """4f: 9 substeps on a streaming launch: FS_ERR_STATE from step, nothing launched (the state is untouched), and the
    context stays usable -- back on FlingBot's table the following frames are bit-exact."""
    from flingbot_amd import sim as fsim
    from oracle import OracleSim

    ctx = fsim.FlingSim(n_envs=2, solver=fsim.FS_SOLVER_STREAM)
    try:
        orcs = [OracleSim(), OracleSim()]
        for e in range(2):
            for s in (ctx.env(e), orcs[e]):
                P.scene(s, 16, 16, seed=e)
        ctx.step(1)
        before = [P.bits(ctx.env(e)) for e in range(2)]
        for e in range(2):
            P.apply(ctx.env(e), {1: P.F(9)})
        with pytest.raises(fsim.FlingSimError, match="8 substeps"):
            ctx.step(1)
        assert ctx.lib.fs_step(ctx.h, -1, 1) == fsim.FS_ERR_STATE
        for e in range(2):
            assert np.array_equal(P.bits(ctx.env(e)), before[e])
            P.apply(ctx.env(e), {1: P.F(4)})
            orcs[e].step(1)
        for _ in range(2):
            for e in range(2):
                P.move_spheres(ctx.env(e))
                P.move_spheres(orcs[e])
                orcs[e].step(1)
            ctx.step(1)
        for e in range(2):
            L.compare(ctx, e, orcs[e], f"after the refused launch, episode {e}")
    finally:
        ctx.close()


@pytest.mark.parametrize("solver,form", [(2, "FUSED_GRID64"), (5, "FUSED_12"), (1, "STREAM_GRIDL")])
def test_list_caps(gpu_required, solver, form):
    """4g: the density ramp (every list length from 0 past 23 in one 64 x 6 episode) under maxNeighbors 1, 3, 4, 5, 16, 17 --
    next to the four staged ids / LDS heads and the 16-register sort --, the six caps as six episodes of one launch, compared
    after every frame for three frames.  Premise, on the oracle's side: lists longer than the cap exist before truncation
    and the counts stop at the cap."""
    from flingbot_amd import sim as fsim
    from oracle import OracleSim

    ctx = fsim.FlingSim(n_envs=len(P.LIST_CAPS), solver=solver)
    try:
        free = OracleSim()
        P.ramp_start(free)
        free.step(1)
        orcs = [OracleSim() for _ in P.LIST_CAPS]
        for e, cap in enumerate(P.LIST_CAPS):
            P.ramp_start(orcs[e], {27: P.F(cap)})
            P.ramp_start(ctx.env(e), {27: P.F(cap)})
        for frame in range(3):
            ctx.step(1)
            assert ctx.last_kernel_form() == getattr(fsim, "FS_FORM_" + form), ctx.last_kernel_form()
            for e, cap in enumerate(P.LIST_CAPS):
                orcs[e].step(1)
                if frame == 0:
                    P.assert_capped(orcs[e], free, cap)
                co = L.compare(ctx, e, orcs[e], f"{form}, cap {cap}, frame {frame + 1}")
                assert co.max() == cap
    finally:
        ctx.close()


@pytest.mark.parametrize("solver,form", [(1, "STREAM_GRIDL"), (2, "FUSED_GRID64")])
def test_parameters_take_effect_at_the_next_launch(gpu_required, solver, form):
    """4h: one live context, the same id list in every call (the streaming back-end caches its slot table across such calls:
    table_epoch == desc_epoch): two frames on FlingBot's table, set_params(ALL with FlingBot's counts) on episode 1 ONLY, two
    frames, set back, two frames -- the oracle receives the same calls.  set_scene restores FlingBot's table; fs_fork carries a
    changed table to its destination, which then steps like the oracle."""
    from flingbot_amd import sim as fsim
    from oracle import OracleSim

    ctx = fsim.FlingSim(n_envs=3, solver=solver)
    try:
        orcs = [OracleSim(), OracleSim()]
        for e in range(2):
            for s in (ctx.env(e), orcs[e]):
                P.scene(s, 64, 8, seed=e)
        fresh = ctx.get_params(0).copy()

        def two_frames(what):
            # (no sphere moves here: fs_set_shape_states would rewrite the descriptors and rebuild the cached table by itself)
            for _ in range(2):
                ctx.step_list([0, 1], 1)
                assert ctx.last_kernel_form() == getattr(fsim, "FS_FORM_" + form)
            for e in range(2):
                orcs[e].step(2)
                L.compare(ctx, e, orcs[e], f"{form}, {what}, episode {e}")

        two_frames("FlingBot's table")
        for s in (ctx.env(1), orcs[1]):
            P.apply(s, P.ALL_SHARED)
        assert np.array_equal(ctx.get_params(0).view(np.uint32), fresh.view(np.uint32))
        two_frames("ALL on episode 1")
        for s in (ctx.env(1), orcs[1]):
            s.set_params(fresh)
        two_frames("set back")
        # fork: the destination gets the source's table
        for s in (ctx.env(1), orcs[1]):
            P.apply(s, P.ALL)
        ctx.fork(1, 2)
        assert np.array_equal(ctx.get_params(2).view(np.uint32), orcs[1].get_params().view(np.uint32))
        ctx.step_list([2], 2)
        orcs[1].step(2)
        L.compare(ctx, 2, orcs[1], f"{form}, the fork's destination")
        assert not np.array_equal(P.bits(ctx.env(2)), P.bits(ctx.env(1)))  # stepping the fork left its source alone
        # a new scene is a new episode: FlingBot's table again
        P.scene(ctx.env(1), 64, 8, seed=1)
        assert np.array_equal(ctx.get_params(1).view(np.uint32), fresh.view(np.uint32))
    finally:
        ctx.close()


BAD_TABLES = [(22, 2), (29, 0), (6, 0.01), (10, 0.001), (27, 0), (27, 97), (27, 3.5), (28, -1), (28, 25), (1, 0), (1, 101),
              (0, -1), (0, 1001), (2, 0.0), (2, -0.01), (2, float("nan"))]


def test_refused_tables_change_nothing(gpu_required):
    """4i: every refusal is the host's: a changed numPlanes / relaxationMode / radius / particle margin, counts and dt outside
    their ranges, a short table, and an episode of a chunk in flight on the service lane.  After each one get_params is
    unchanged bit for bit (a valid change riding in the refused table is not applied either); at the end every table of
    param_cases round-trips and the context still steps like the oracle."""
    from fling_helpers import load_fling_golden
    from flingbot_amd import sim as fsim
    from oracle import OracleSim
    from test_fling_gpu import _make

    ctx = fsim.FlingSim(n_envs=1, solver=fsim.FS_SOLVER_FUSED)
    try:
        orc = OracleSim()
        for s in (ctx.env(0), orc):
            P.scene(s, 16, 16)
        t0 = ctx.get_params(0).copy()
        assert np.array_equal(t0.view(np.uint32), orc.get_params().view(np.uint32))
        for slot, value in BAD_TABLES:
            t = t0.copy()
            t[slot] = value
            t[7] = 0.02
            with pytest.raises(fsim.FlingSimError):
                ctx.set_params(0, t)
            assert ctx.lib.fs_set_params(ctx.h, 0, t.ctypes.data_as(fsim.C.POINTER(fsim.C.c_float)), 32) == fsim.FS_ERR_ARG
            assert np.array_equal(ctx.get_params(0).view(np.uint32), t0.view(np.uint32)), (slot, value)
            for s in (ctx.env(0), orc):  # straight after the refusal, before anything rewrites the table: one frame like the oracle's
                P.frames(s, 1)
            L.compare(ctx, 0, orc, f"after the refused slot {slot} = {value}")
        with pytest.raises(fsim.FlingSimError):
            ctx.set_params(0, t0[:31])
        for s in (ctx.env(0), orc):
            P.frames(s, 1)
        L.compare(ctx, 0, orc, "after the refused short table")
        ignored = t0.copy()
        ignored[[19, 20, 21, 30, 31]] = 0.25
        ctx.set_params(0, ignored)
        assert np.array_equal(ctx.get_params(0).view(np.uint32), t0.view(np.uint32))
        for name, table in [("ALL", P.ALL), ("ALL_SHARED", P.ALL_SHARED)] + [(k, v[0]) for k, v in P.EDGES.items()]:
            want = P.apply(ctx.env(0), table)
            assert np.array_equal(ctx.get_params(0).view(np.uint32), want.view(np.uint32)), name
            ctx.set_params(0, t0)
            assert np.array_equal(ctx.get_params(0).view(np.uint32), t0.view(np.uint32)), name
        for s in (ctx.env(0), orc):
            P.frames(s, 3)
        L.compare(ctx, 0, orc, "after the refusals")
    finally:
        ctx.close()
    # the service lane: an episode of a chunk in flight is not rewritten (as tests/test_schedule_gpu.py provokes it)
    g = load_fling_golden()
    ctx = _make(g, 2)
    try:
        z, gr = np.zeros((1, 2, 3)), np.zeros((1, 2), int)
        t0 = ctx.get_params(0).copy()
        ticket, prog, status, steps = ctx.advance_begin([0], [2], z, gr, [0.0], [6], [-1], [0], [0], cap_min=6, cap=6)
        ctx.service_lane(True)
        try:
            with pytest.raises(fsim.FlingSimError, match="in flight"):
                P.apply(ctx.env(0), P.ALL)
        finally:
            ctx.service_lane(False)
        ctx.advance_end(ticket, prog, status, steps)
        assert np.array_equal(ctx.get_params(0).view(np.uint32), t0.view(np.uint32))
        ref = _make(g, 2)
        ref.step_list([0], 6)
        assert np.array_equal(ctx.get_positions(0).view(np.uint32), ref.get_positions(0).view(np.uint32))
        ref.close()
    finally:
        ctx.close()
