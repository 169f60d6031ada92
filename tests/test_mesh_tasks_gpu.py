"""Mesh (shirt) tasks on the device: batched generate_tasks on synthetic quad-mesh shirts against the tasks the REFERENCE's
generate_randomization(cloth_type='mesh') produced on the oracle (tests/golden/mesh_task_golden.npz), bit for bit, in batches
that mix meshes with a grid cloth; and the generated tasks through storage, a fresh context and one batched fling."""
import copy
import random

import numpy as np
import pytest

from mesh_task_helpers import bits as _bits, check_task_against_golden, golden, n_cases, write_case_mesh

pytestmark = pytest.mark.gpu

_CACHE = {}


def _case_params(tmp_dir, difficulty):
    """draw_task_parameters for the golden cases of one difficulty, each seeded like the golden run -> (cases, params)."""
    from flingbot_amd import tasks as ftasks

    g = golden()
    cases = [c for c in range(n_cases()) if str(g[f"c{c}_difficulty"]) == difficulty]
    params = []
    for ci in cases:
        d = tmp_dir / f"case{ci}"
        d.mkdir(exist_ok=True)
        write_case_mesh(g, ci, d)
        seed = int(g[f"c{ci}_seed"])
        random.seed(seed)
        np.random.seed(seed)
        params.append(ftasks.draw_task_parameters(cloth_type='mesh', cloth_mesh_path=d, task_difficulty=difficulty))
    return cases, params


def _grid_params():
    from flingbot_amd import tasks as ftasks

    random.seed(9)
    np.random.seed(9)
    p = ftasks.draw_task_parameters(min_cloth_size=24, strict_min_edge_length=24, max_cloth_size=33)
    assert all(24 <= s <= 32 for s in p["cloth_size"])
    return p


def _grid_alone():
    """The grid entry of the mixed batch generated on its own (once per session)."""
    from flingbot_amd import sim as fsim, tasks as ftasks

    if "grid" not in _CACHE:
        ctx = fsim.FlingSim(n_envs=1, solver=0)
        _CACHE["grid"] = ftasks.generate_tasks(ctx, [_grid_params()])[0]
        ctx.close()
        assert _CACHE["grid"] is not None
    return _CACHE["grid"]


def _hard_batch(tmp_path_factory, solver):
    """[shirt A seed 1, GRID, shirt A seed 2, shirt B] generated in one batch -> (cases, mesh tasks, grid task)."""
    from flingbot_amd import sim as fsim, tasks as ftasks

    if ("hard", solver) not in _CACHE:
        cases, params = _case_params(tmp_path_factory.mktemp("meshes"), "hard")
        assert len(cases) == 3
        params.insert(1, _grid_params())
        ctx = fsim.FlingSim(n_envs=len(params), solver=solver)
        out = ftasks.generate_tasks(ctx, copy.deepcopy(params))
        form = ctx.last_kernel_form()
        ctx.close()
        grid = out.pop(1)
        _CACHE[("hard", solver)] = (cases, out, grid, form)
    return _CACHE[("hard", solver)]


@pytest.mark.parametrize("solver", [0, 1, 2])
def test_mixed_hard_batch_matches_reference(gpu_required, tmp_path_factory, solver):
    """Three hard mesh tasks and one grid task in ONE batch (solver 0 = automatic, 1 = forced streaming, 2 = forced fused): the
    meshes equal the reference's tasks and the grid entry equals the task it is when generated alone, bit for bit -- the 40
    settle steps of the meshes do not reach it."""
    g = golden()
    cases, made, grid, _ = _hard_batch(tmp_path_factory, solver)
    for ci, task in zip(cases, made):
        check_task_against_golden(task, g, ci)
    alone = _grid_alone()
    assert grid is not None and len(grid["mesh_verts"]) == 0 and list(grid["cloth_size"]) == list(alone["cloth_size"])
    for k in ("particle_pos", "particle_vel", "shape_pos"):
        assert np.array_equal(_bits(grid[k]), _bits(alone[k])), k
    assert np.array_equal(grid["phase"], alone["phase"]) and grid["flatten_area"] == alone["flatten_area"]
    assert abs(grid["initial_coverage"] - alone["initial_coverage"]) <= 1e-12


@pytest.mark.parametrize("solver", [0, 1, 2])
def test_easy_mesh_task_matches_reference(gpu_required, tmp_path, solver):
    from flingbot_amd import sim as fsim, tasks as ftasks

    cases, params = _case_params(tmp_path, "easy")
    assert len(cases) == 1
    ctx = fsim.FlingSim(n_envs=1, solver=solver)
    made = ftasks.generate_tasks(ctx, params)
    ctx.close()
    check_task_against_golden(made[0], golden(), cases[0])


def test_generated_mesh_tasks_store_load_and_fling(gpu_required, tmp_path_factory, tmp_path):
    """generate -> taskio.save_tasks -> TaskLoader -> load_tasks into a fresh context: positions bit-identical and the particle
    count is the mesh's vertex count; one batched pick_and_fling + postaction finishes with finite coverage."""
    from flingbot_amd import sim as fsim, taskio, tasks as ftasks
    from flingbot_amd.primitives import FlingPrimitives

    _, made, grid, _ = _hard_batch(tmp_path_factory, 0)
    tasks = [made[0], grid, made[1], made[2]]
    path = str(tmp_path / "mixed.npz")
    assert taskio.save_tasks(path, tasks) == 4
    loaded = taskio.TaskLoader(path, repeat=False).all_tasks()
    assert [t.cloth_size.tolist() for t in loaded] == [[-1, -1], list(grid["cloth_size"]), [-1, -1], [-1, -1]]
    n = len(loaded)
    ctx = fsim.FlingSim(n_envs=n, solver=0)
    assert ftasks.load_tasks(ctx, loaded) == list(range(n))
    for e, (t, src) in enumerate(zip(loaded, tasks)):
        want = len(src["mesh_verts"]) // 3 if len(src["mesh_verts"]) else int(np.prod(src["cloth_size"]))
        assert ctx.n_particles(e) == want == len(src["particle_pos"]) // 4
        assert np.array_equal(_bits(ctx.get_positions(e)), _bits(src["particle_pos"]))
        assert np.array_equal(_bits(ctx.get_velocities(e)), _bits(src["particle_vel"]))
        assert abs(ctx.coverage()[e] - src["initial_coverage"]) <= 1e-12
        stats = t.get_stats()   # what the replay file records of the task: nothing in it is derived from a grid size
        assert t.flatten_area == src["flatten_area"] and stats["max_coverage"] == src["flatten_area"]
        assert stats["init_coverage"] == src["initial_coverage"] and stats["cloth_mass"] == src["cloth_mass"]
        assert np.asarray(stats["cloth_size"]).tolist() == np.asarray(src["cloth_size"]).tolist()
        assert np.array_equal(stats["cloth_stiff"], src["cloth_stiff"]) and stats["task_difficulty"] == src["task_difficulty"]
    prim = FlingPrimitives(ctx, range(n))
    prim.setup_pickers()
    prim.preaction()
    p = [ctx.get_positions(e).reshape(-1, 4) for e in range(n)]
    p1 = np.array([q[np.argmin(q[:, 0]), :3] for q in p], np.float64)
    p2 = np.array([q[np.argmax(q[:, 0]), :3] for q in p], np.float64)
    out = prim.pick_and_fling(p1, p2, [True] * n, [True] * n)
    term = prim.postaction()
    cov = ctx.coverage()
    assert len(out) == n and len(term) == n and all(np.isfinite(cov)) and all(c > 0 for c in cov)
    for e in range(n):
        assert np.isfinite(ctx.get_positions(e)).all()
    ctx.close()


def test_throughput_launch_of_uncoded_meshes_keeps_springs(gpu_required, tmp_path):
    """A streaming launch above the latency form's threshold (more than 32 x 4096 particles) whose cloths have no one-byte
    spring codes (a two-layer shirt: max_deg 18 > 16): it must stream the ELL adjacency (FS_FORM_STREAM_ELL), not run the
    coded form on an empty dictionary -- which drops every spring.  36 copies of a 3 764-vertex shirt, perturbed so that the
    springs act, five steps: episodes of the large launch equal the same cloth stepped alone (the latency form, which the
    parity suite pins to the oracle), bit for bit."""
    import shirt_meshes
    from flingbot_amd import sim as fsim, tasks as ftasks

    path = tmp_path / "big_processed.obj"
    path.write_text(shirt_meshes.shirt_a(body_w=33, body_h=44, sleeve_w=14, sleeve_h=14, neck=11))
    verts, faces, stretch, bend, shear = ftasks.load_cloth(str(path))
    n, copies = len(verts), 36
    assert n <= 4096 and n * copies > 32 * 4096
    sp = np.array([0, 0.15, 0, -1, -1, 0.9, 0.9, 0.9, 2, 0, 2, 0, np.pi / 2, -np.pi / 2, 0, 720, 720, 0.5, 0], np.float32)
    arrays = (verts.reshape(-1), stretch.reshape(-1), bend.reshape(-1), shear.reshape(-1), faces.reshape(-1))
    h = fsim.host_scene(sp, *arrays)
    assert h["max_deg"] > 16 and not (h["stream_dict"] != 0xffffffff).any()      # no codes for this cloth
    rng = np.random.RandomState(3)
    noise = (rng.randn(n, 3) * 0.002).astype(np.float32)
    results = {}
    for envs in (1, copies):
        ctx = fsim.FlingSim(n_envs=envs, solver=fsim.FS_SOLVER_STREAM)
        for e in range(envs):
            ctx.set_scene(e, sp, *arrays)
            pos = ctx.get_positions(e).reshape(-1, 4).copy()
            pos[:, :3] += noise
            ctx.set_positions(e, pos.ravel())
        ctx.step(5)
        form = ctx.last_kernel_form()
        results[envs] = [(ctx.get_positions(e), ctx.get_velocities(e)) for e in sorted({0, envs // 2, envs - 1})]
        ctx.close()
        assert form == (fsim.FS_FORM_STREAM_EAGER if envs == 1 else fsim.FS_FORM_STREAM_ELL), form
    want_p, want_v = results[1][0]
    assert np.isfinite(want_p).all()
    for got_p, got_v in results[copies]:
        assert np.array_equal(_bits(got_p), _bits(want_p)) and np.array_equal(_bits(got_v), _bits(want_v))


def test_generator_command_writes_a_mesh_task_set(gpu_required, tmp_path, capsys):
    """`python -m flingbot_amd.tasks` itself (main()) on a directory with the one-layer shirt: three tasks over two slots, i.e.
    two batches; the file holds three mesh tasks TaskLoader reads back, and the summary line says what was done.  The same
    seed again writes the same tasks."""
    import json

    import shirt_meshes
    from flingbot_amd import taskio, tasks as ftasks

    (tmp_path / "meshes").mkdir()
    (tmp_path / "meshes" / "b_processed.obj").write_text(shirt_meshes.shirt_b())
    n_vertices = len(shirt_meshes.parse(shirt_meshes.shirt_b())[0])
    sets = []
    for name in ("one.npz", "two.npz"):
        out = str(tmp_path / name)
        ftasks.main(["--path", out, "--num_tasks", "3", "--slots", "2", "--cloth_type", "mesh", "--cloth_mesh_path",
                     str(tmp_path / "meshes"), "--num_processes", "16", "--seed", "4"])
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert line["tasks"] == 3 and line["cloth_type"] == "mesh" and line["draws"] >= 3 + line["rejected"]
        assert line["particles_min"] == line["particles_max"] == n_vertices
        sets.append(taskio.TaskLoader(out, repeat=False).all_tasks())
        capsys.readouterr()
    for a, b in zip(*sets):
        assert a.cloth_size.tolist() == [-1, -1] and len(a.mesh_verts) == 3 * n_vertices and len(a.particle_pos) == 4 * n_vertices
        assert a.flatten_area == ftasks.mesh_flatten_area(a.mesh_verts.reshape(-1, 3), a.mesh_faces.reshape(-1, 3))
        assert np.isfinite(a.particle_pos).all() and 0 < a.initial_coverage
        for k in ("particle_pos", "particle_vel", "cloth_stiff"):
            assert np.array_equal(a[k], b[k]), k
    assert len(sets[0]) == 3 and len({t.cloth_mass for t in sets[0]}) == 3     # three draws, not one task three times
