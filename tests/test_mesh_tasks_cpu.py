"""Mesh (shirt) tasks without a GPU: the random draws of tasks.draw_task_parameters(cloth_type='mesh') against the draws the
REFERENCE's generate_randomization made (tests/golden/mesh_task_golden.npz, written by tests/golden/make_mesh_task_golden.py),
mesh_flatten_area against the golden's independently written triangle-area sum, the generator command's parser, the
synthetic shirts' properties, and the mesh branch of generate_tasks on the CPU oracle."""
import os
import random
import re
import shlex
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import shirt_meshes  # noqa: E402

from mesh_task_helpers import check_task_against_golden, golden, n_cases, write_case_mesh  # noqa: E402

GOLD = os.path.join(HERE, "golden")


def test_golden_meshes_are_the_helpers():
    """The fixture's OBJ texts are what tests/shirt_meshes.py writes today (a changed helper needs a regenerated fixture)."""
    g = golden()
    assert str(g["obj_a"]) == shirt_meshes.shirt_a() and str(g["obj_b"]) == shirt_meshes.shirt_b()
    assert sorted({(str(g[f"c{c}_mesh"]), str(g[f"c{c}_difficulty"])) for c in range(n_cases())}) == \
        [("a", "hard"), ("b", "easy"), ("b", "hard")]
    assert sum(str(g[f"c{c}_mesh"]) == "a" for c in range(n_cases())) == 2


@pytest.mark.parametrize("name", ["a", "b"])
def test_shirt_mesh_properties(name):
    text = {"a": shirt_meshes.shirt_a, "b": shirt_meshes.shirt_b}[name]()
    v, q = shirt_meshes.parse(text)
    assert len(v) <= 1000 and (name != "a" or 450 <= len(v) <= 600)
    # every lattice edge is 6.25 mm long, or joins a layer to a seam 2.5 mm off it, or is one of shirt B's re-cut edges
    sides = np.concatenate([np.linalg.norm(v[q[:, k]] - v[q[:, (k + 1) % 4]], axis=1) for k in range(4)])
    assert np.median(sides) == pytest.approx(0.00625, abs=1e-6)
    assert (np.abs(sides - 0.00625) < 1e-6).mean() > 0.85 and sides.min() > 0.004
    # not a row-major grid: neither the vertex order nor the face order is sorted
    assert (np.diff(v[:, 2]) < 0).sum() > len(v) // 4 and (np.diff(q.min(axis=1)) < 0).sum() > len(q) // 4
    val, interior = shirt_meshes.valences(text)
    assert interior.sum() > len(v) // 2 and (val[interior] != 4).any() and (val[interior] == 4).sum() > (val[interior] != 4).sum()
    # no degenerate triangle (load_cloth's split 0-1-2 / 0-2-3)
    for tri in (q[:, [0, 1, 2]], q[:, [0, 2, 3]]):
        area = 0.5 * np.linalg.norm(np.cross(v[tri[:, 1]] - v[tri[:, 0]], v[tri[:, 2]] - v[tri[:, 0]]), axis=1)
        assert area.min() > 0.1 * 0.5 * 0.00625 ** 2


@pytest.mark.parametrize("name,want", [("a", 0), ("b", 1)])
def test_restnear_filter_form(name, want, tmp_path):
    """fs_host_scene_build's flags: shirt A's two layers put more than 16 rest-near neighbours around most vertices, so the packed
    filter sets are refused (restnear_ok 0: the kernels test rest positions); shirt B's sets pack (1)."""
    from flingbot_amd import sim as fsim, tasks as ftasks

    path = tmp_path / "x_processed.obj"
    path.write_text({"a": shirt_meshes.shirt_a, "b": shirt_meshes.shirt_b}[name]())
    verts, faces, stretch, bend, shear = ftasks.load_cloth(str(path))
    sp = np.array([0, 1, 0, -1, -1, 0.9, 0.9, 0.9, 2, 0, 2, 0, np.pi / 2, -np.pi / 2, 0, 720, 720, 0.5, 0])
    h = fsim.host_scene(sp, verts.reshape(-1), stretch.reshape(-1), bend.reshape(-1), shear.reshape(-1), faces.reshape(-1))
    assert h["n"] == len(verts) and h["t"] == len(faces)
    assert h["flags"]["restnear_ok"] == want
    if name == "a":   # "most vertices": count them with the builder's own radius
        r = float(h["params"][2]) + float(h["params"][8])   # radius + particleCollisionMargin
        rest = h["positions"].reshape(-1, 4)[:, :3].astype(np.float64)
        near = ((rest[:, None, :] - rest[None, :, :]) ** 2).sum(axis=2) < r * r
        assert ((near.sum(axis=1) - 1) > 16).mean() > 0.5


def _restated_draws(seed, directory, difficulty, n_vertices):
    """The calls generate_randomization makes on the global generators for a mesh task, in its order."""
    random.seed(seed)
    np.random.seed(seed)
    np.random.randint(64, 104)
    np.random.randint(64, 104)
    random.choice(list(Path(directory).rglob('*_processed.obj')))
    np.random.uniform(0.85, 0.95, 3)
    np.random.uniform(0.2, 2.0)
    if difficulty == 'hard':
        random.randint(0, n_vertices // 3 - 1)
        np.random.random(1)
    else:
        for _ in range(10):
            random.randint(0, n_vertices // 3 - 1)
            np.random.uniform(-0.2, 0.2, 3)
    return random.getstate(), np.random.get_state()


def _same_state(a, b):
    return a[0] == b[0] and a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:]


@pytest.mark.parametrize("ci", range(4))
def test_mesh_draws_match_reference(ci, tmp_path):
    from flingbot_amd import tasks as ftasks

    g = golden()
    assert ci < n_cases()
    path = write_case_mesh(g, ci, tmp_path)
    seed, difficulty = int(g[f"c{ci}_seed"]), str(g[f"c{ci}_difficulty"])
    random.seed(seed)
    np.random.seed(seed)
    p = ftasks.draw_task_parameters(cloth_type='mesh', cloth_mesh_path=tmp_path, task_difficulty=difficulty)
    after = (random.getstate(), np.random.get_state())
    assert p is not None and p["cloth_size"] == [-1, -1] and p["task_difficulty"] == difficulty
    assert p["mesh_path"] == path and int(g[f"c{ci}_file_index"]) == 0 and int(g[f"c{ci}_n_files"]) == 1
    assert np.array_equal(p["cloth_stiff"], g[f"c{ci}_draw_stiff"]) and np.array_equal(p["cloth_stiff"], g[f"c{ci}_cloth_stiff"])
    assert p["cloth_mass"] == float(g[f"c{ci}_draw_mass"]) == float(g[f"c{ci}_cloth_mass"])
    verts = p["mesh_verts"]
    assert verts.shape == (len(g[f"c{ci}_mesh_verts"]) // 3, 3)
    assert int(g[f"c{ci}_num_particle"]) == len(verts) // 3          # the reference's quirk: a third of the vertices
    if difficulty == "hard":
        assert [p["pickpoint"]] == g[f"c{ci}_draw_pickpoints"].tolist()
        assert np.array_equal(p["height"], g[f"c{ci}_draw_height"] * 1.0 + 0.5) and p["height"].shape == (1,)
    else:
        assert [t[0] for t in p["throws"]] == g[f"c{ci}_draw_pickpoints"].tolist() and len(p["throws"]) == 10
        drawn = g[f"c{ci}_draw_displacements"].copy()
        drawn[:, 1] = 0.2
        assert np.array_equal(np.stack([t[1] for t in p["throws"]]), drawn)
    assert max(np.atleast_1d(g[f"c{ci}_draw_pickpoints"])) < len(verts) // 3
    # the five arrays are load_cloth's, and the golden's task stores them flattened
    for k, arr in zip(("mesh_verts", "mesh_faces", "mesh_stretch_edges", "mesh_bend_edges", "mesh_shear_edges"),
                      ftasks.load_cloth(path)):
        assert np.array_equal(p[k], arr) and np.array_equal(np.asarray(p[k]).reshape(-1), g[f"c{ci}_{k}"]), k
    # flatten_area: two float64 sums of <= 10^4 positive terms in different orders differ by at most n * eps
    want = float(g[f"c{ci}_flatten_area"])
    assert abs(p["flatten_area"] - want) <= 1e-12 * want
    assert p["flatten_area"] == ftasks.mesh_flatten_area(verts, p["mesh_faces"])
    assert _same_state(after, _restated_draws(seed, tmp_path, difficulty, len(verts)))


def test_mesh_flatten_area_quads_and_triangles():
    from flingbot_amd import tasks as ftasks

    v = np.array([[0, 0, 0], [2, 0, 0], [2, 0, 1], [0, 0, 1], [0, 3, 0], [2, 3, 0]], float)
    quads = np.array([[0, 1, 2, 3], [0, 1, 5, 4]])
    assert ftasks.mesh_flatten_area(v, quads) == pytest.approx((2.0 + 6.0) / 2, rel=1e-15)
    tris = np.array([[0, 1, 2], [0, 2, 3], [0, 1, 5], [0, 5, 4]])
    assert ftasks.mesh_flatten_area(v, tris) == ftasks.mesh_flatten_area(v, quads)
    assert ftasks.mesh_flatten_area(v.reshape(-1), tris.reshape(-1)) == ftasks.mesh_flatten_area(v, quads)
    v2, q2 = shirt_meshes.parse(shirt_meshes.shirt_b())
    cells = len(q2)      # one layer of unit lattice cells (the re-cut hexagon keeps its two cells' area)
    assert ftasks.mesh_flatten_area(v2, q2) == pytest.approx(cells * 0.00625 ** 2 / 2, rel=1e-9)


def test_square_defaults_unchanged():
    """With the new arguments at their defaults the draws are those of tests/golden/task_golden.npz (the reference's grid draws)."""
    from flingbot_amd import tasks as ftasks

    g = np.load(os.path.join(GOLD, "task_golden.npz"))
    cases = [int(k[1:-5]) for k in g.files if k.endswith("_seed")]
    assert cases
    for ci in cases:
        seed, difficulty = int(g[f"t{ci}_seed"]), str(g[f"t{ci}_difficulty"])
        draws = []
        for extra in ({}, dict(cloth_type='square', cloth_mesh_path=None)):
            random.seed(seed)
            np.random.seed(seed)
            draws.append(ftasks.draw_task_parameters(min_cloth_size=20, strict_min_edge_length=20, max_cloth_size=30,
                                                     task_difficulty=difficulty, **extra))
        p = draws[0]
        assert list(p["cloth_size"]) == g[f"t{ci}_cloth_size"].tolist()
        assert np.array_equal(p["cloth_stiff"], g[f"t{ci}_cloth_stiff"]) and p["cloth_mass"] == float(g[f"t{ci}_cloth_mass"])
        assert set(p) == {"cloth_size", "cloth_stiff", "cloth_mass", "task_difficulty"} | ({"pickpoint", "height"} if difficulty == "hard"
                                                                                          else {"throws"})
        assert set(draws[1]) == set(p) and draws[1]["cloth_size"] == p["cloth_size"] and draws[1]["cloth_mass"] == p["cloth_mass"]
        if difficulty == "hard":
            assert draws[1]["pickpoint"] == p["pickpoint"] and np.array_equal(draws[1]["height"], p["height"])
    random.seed(0)
    np.random.seed(0)
    assert ftasks.draw_task_parameters(min_cloth_size=10, strict_min_edge_length=64, max_cloth_size=20) is None
    np.random.seed(0)   # the early None applies to a mesh too: both size draws happen first
    assert ftasks.draw_task_parameters(min_cloth_size=10, strict_min_edge_length=64, max_cloth_size=20, cloth_type='mesh',
                                       cloth_mesh_path="/nonexistent") is None


def test_mesh_choice_follows_directory_walk(tmp_path):
    """Three meshes in nested directories: the chosen file is random.choice(list(rglob)) in the walk's own order."""
    from flingbot_amd import tasks as ftasks

    (tmp_path / "sub" / "deeper").mkdir(parents=True)
    texts = {"zz_processed.obj": shirt_meshes.shirt_b(), "sub/aa_processed.obj": shirt_meshes.shirt_a(),
             "sub/deeper/mm_processed.obj": shirt_meshes.shirt_b(body_w=8, body_h=10, sleeve_w=3, sleeve_h=3)}
    for rel, text in texts.items():
        (tmp_path / rel).write_text(text)
    (tmp_path / "sub" / "ignored.obj").write_text(shirt_meshes.shirt_b())
    files = list(Path(tmp_path).rglob('*_processed.obj'))
    assert len(files) == 3
    seen = set()
    for seed in range(8):
        random.seed(seed)
        want = str(random.choice(files))
        random.seed(seed)
        np.random.seed(seed)
        p = ftasks.draw_task_parameters(cloth_type='mesh', cloth_mesh_path=str(tmp_path))
        assert p["mesh_path"] == want
        assert len(p["mesh_verts"]) == len(shirt_meshes.parse(Path(want).read_text())[0])
        seen.add(want)
    assert len(seen) == 3


README_COMMANDS = (
    "python -m flingbot_amd.tasks --path new-normal-rect-tasks.npz --num_processes 16 --num_tasks 200 --cloth_type square "
    "--min_cloth_size 64 --max_cloth_size 104",
    "python -m flingbot_amd.tasks --path new-large-rect-tasks.npz --num_processes 16 --num_tasks 200 --cloth_type square "
    "--min_cloth_size 64 --max_cloth_size 120 --strict_min_edge_length 112",
    "python -m flingbot_amd.tasks --path new-shirt-tasks.npz --num_processes 16 --num_tasks 200 --cloth_type mesh "
    "--cloth_mesh_path cloth3d/val",
)


def test_generator_command_parser():
    from flingbot_amd import tasks as ftasks

    ap = ftasks.build_parser()
    readme = open(os.path.join(os.path.dirname(HERE), "README.md")).read()
    in_readme = [ln.strip() for ln in readme.splitlines() if ln.strip().startswith("python -m flingbot_amd.tasks ")]
    for cmd in README_COMMANDS:
        assert cmd in in_readme, cmd
    got = [ap.parse_args(shlex.split(cmd)[3:]) for cmd in README_COMMANDS]
    assert [(a.cloth_type, a.min_cloth_size, a.max_cloth_size, a.strict_min_edge_length, a.num_tasks) for a in got] == \
        [("square", 64, 104, 64, 200), ("square", 64, 120, 112, 200), ("mesh", 64, 104, 64, 200)]
    assert got[2].cloth_mesh_path == "cloth3d/val" and all(a.task_difficulty == "hard" and a.seed is None for a in got)
    d = ap.parse_args(["--path", "x.npz"])   # the reference's defaults (environment/tasks.py:466-484)
    assert (d.cloth_type, d.num_tasks, d.num_processes, d.min_cloth_size, d.strict_min_edge_length, d.max_cloth_size,
            d.cloth_mesh_path) == ("square", 100, 8, 64, 64, 104, None)
    e = ap.parse_args(["--path", "x.npz", "--task_difficulty", "easy", "--seed", "3", "--slots", "7"])
    assert (e.task_difficulty, e.seed, e.slots) == ("easy", 3, 7)
    with pytest.raises(SystemExit):
        ap.parse_args(["--path", "x.npz", "--cloth_type", "shirt"])
    with pytest.raises(SystemExit):
        ftasks.main(["--path", "x.npz", "--cloth_type", "mesh"])   # no --cloth_mesh_path: refused before any GPU is touched
    assert re.search(r"num_processes.*ignored", ap.format_help(), re.S)


class _Batch:
    """generate_task_set's view of a simulator, scripted: which of the drawn entries the generator would reject."""

    def __init__(self, n_envs, reject):
        self.n_envs, self.reject, self.batches = n_envs, set(reject), []


def test_generate_task_set_redraws(monkeypatch):
    """None draws are redrawn at once and rejected tasks are replaced by later draws, until num_tasks are accepted."""
    from flingbot_amd import tasks as ftasks

    serial = iter(range(1000))
    monkeypatch.setattr(ftasks, "draw_task_parameters", lambda **kw: (lambda k: None if k % 4 == 1 else dict(id=k, **kw))(next(serial)))

    def fake_generate(sim, params, picker_radius=0.05):
        sim.batches.append([p["id"] for p in params])
        return [None if p["id"] in sim.reject else dict(id=p["id"]) for p in params]
    monkeypatch.setattr(ftasks, "generate_tasks", fake_generate)
    sim = _Batch(3, reject={2, 6})
    tasks, draws, rejected = ftasks.generate_task_set(sim, 5, cloth_type="square")
    assert sim.batches == [[0, 2, 3], [4, 6, 7], [8]] and [t["id"] for t in tasks] == [0, 3, 4, 7, 8]
    assert rejected == 2 and draws == 9


class _OracleMeshSim:
    """fling_helpers.OracleTaskSim with set_scene's mesh arguments."""

    def __new__(cls, n):
        from fling_helpers import OracleTaskSim

        class Sim(OracleTaskSim):
            def set_scene(self, e, scene_params, *mesh):
                self.sims[e].set_scene(scene_params, *mesh)
        return Sim(n)


def test_mesh_generation_on_oracle_matches_reference(tmp_path):
    """generate_tasks' mesh branch on the CPU oracle, shirt B / hard: every field the reference returned, bit for bit."""
    from flingbot_amd import tasks as ftasks

    g = golden()
    ci = [c for c in range(n_cases()) if (str(g[f"c{c}_mesh"]), str(g[f"c{c}_difficulty"])) == ("b", "hard")][0]
    write_case_mesh(g, ci, tmp_path)
    seed = int(g[f"c{ci}_seed"])
    random.seed(seed)
    np.random.seed(seed)
    p = ftasks.draw_task_parameters(cloth_type='mesh', cloth_mesh_path=tmp_path)
    task = ftasks.generate_tasks(_OracleMeshSim(1), [p])[0]
    check_task_against_golden(task, g, ci)
