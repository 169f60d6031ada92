"""Generates tests/golden/mesh_task_golden.npz: the REFERENCE's own generate_randomization(cloth_type='mesh',
cloth_mesh_path=<a temporary directory>) (environment/tasks.py:105-284 with load_cloth :39-103 and flex_utils' set_scene /
center_object / wait_until_stable / get_current_covered_area) run on the oracle-backed `pyflex` stub, exactly as
make_golden.py's task_vectors does for grid cloths, on the synthetic shirts of tests/shirt_meshes.py.

    python tests/golden/make_mesh_task_golden.py

`trimesh`, which the reference uses for one number (`trimesh.load(path).area / 2`, tasks.py:142), is a stub here whose
load(path).area is the float64 sum of the OBJ's triangle areas, written out below on its own (Heron-free: half the norm
of the edge cross product, accumulated triangle by triangle) -- NOT through flingbot_amd.tasks.mesh_flatten_area, so that
the product function is compared against an independent statement of the formula.

Stored per case c<k>: the OBJ text, the seed, every drawn value (file index in the directory walk, stiffnesses, mass, pick
point and height or the ten throws), the simulation-step count and all task fields.  Seeds were chosen so that the
reference returns a task, not None; a seed that stops doing so fails the script.
"""
import math
import os
import random
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
from make_golden import REF  # noqa: E402  (where the reference lives; make_golden.py itself is left untouched)

# (mesh, difficulty, seed)
CASES = (("a", "hard", 1), ("a", "hard", 2), ("b", "hard", 1), ("b", "easy", 1))


class _Any:
    def __init__(self, *a, **k): pass
    def __call__(self, *a, **k): return _Any()
    def __getattr__(self, name): return _Any()


def _anystub(name):
    m = types.ModuleType(name)

    def _ga(attr):
        if attr.startswith("__"):
            raise AttributeError(attr)
        return _Any()
    m.__getattr__ = _ga
    m.__path__ = []
    m.__file__ = "<stub %s>" % name
    sys.modules[name] = m
    return m


def _obj_surface_area(path):
    """What trimesh reports as `.area` for a quad OBJ: the sum of its triangles' areas (each quad as 0-1-2 and 0-2-3)."""
    verts, total = [], 0.0
    with open(path) as fh:
        rows = fh.read().splitlines()
    for row in rows:
        if row.startswith("v "):
            verts.append(tuple(float(t) for t in row.split()[1:4]))
    for row in rows:
        if not row.startswith("f "):
            continue
        ids = [int(t.split("/")[0]) - 1 for t in row.split()[1:]]
        for a, b, c in ((ids[0], ids[1], ids[2]), (ids[0], ids[2], ids[3])):
            ux, uy, uz = (verts[b][k] - verts[a][k] for k in range(3))
            vx, vy, vz = (verts[c][k] - verts[a][k] for k in range(3))
            total += 0.5 * math.sqrt((uy * vz - uz * vy) ** 2 + (uz * vx - ux * vz) ** 2 + (ux * vy - uy * vx) ** 2)
    return total


def main():
    from oracle import OracleSim
    import shirt_meshes
    import torch  # noqa: F401  (before the stubs: its import machinery inspects sys.modules)
    import scipy.ndimage  # noqa: F401

    if not hasattr(np, "alltrue"):
        np.alltrue = np.all
    if not hasattr(np, "float"):
        np.float = float
    for name in ("h5py", "filelock", "imageio", "trimesh", "OpenEXR", "Imath", "cv2", "PIL", "skimage", "skimage.morphology",
                 "matplotlib", "matplotlib.pyplot", "ray", "pyflex", "tqdm"):
        if name not in ("pyflex", "trimesh"):
            try:
                __import__(name)
                continue
            except Exception:
                pass
        _anystub(name)
    sys.modules["ray"].remote = lambda f: f
    loaded = []

    def _trimesh_load(path, *a, **k):
        loaded.append(str(path))
        return types.SimpleNamespace(area=_obj_surface_area(path))
    sys.modules["trimesh"].load = _trimesh_load
    box, counter = {}, {"steps": 0}
    pf = sys.modules["pyflex"]
    for name in ("get_positions", "set_positions", "get_velocities", "set_velocities", "get_shape_states",
                 "set_shape_states", "add_sphere", "get_phases", "set_phases"):
        setattr(pf, name, (lambda nm: lambda *a, **k: getattr(box["o"], nm)(*a, **k))(name))

    def _step(*a, **k):
        counter["steps"] += 1
        box["o"].step(1)
    pf.step = _step
    pf.set_scene = lambda scene_idx=0, scene_params=None, vertices=(), stretch_edges=(), bend_edges=(), shear_edges=(), \
        faces=(), thread_idx=0: box["o"].set_scene(scene_params, vertices, stretch_edges, bend_edges, shear_edges, faces)
    for m in [k for k in sys.modules if k == "environment" or k.startswith("environment.") or k in ("flex_utils", "nets")]:
        del sys.modules[m]
    sys.path.insert(0, REF)
    from environment import tasks as ref_tasks
    from environment import flex_utils as ref_fu

    texts = {"a": shirt_meshes.shirt_a(), "b": shirt_meshes.shirt_b()}
    out = {"n_cases": np.array(len(CASES)), "obj_a": np.array(texts["a"]), "obj_b": np.array(texts["b"])}
    # the draws are recorded by watching the generators the reference draws from
    drawn = {}
    real_randint, real_choice = random.randint, random.choice
    real_uniform, real_random = np.random.uniform, np.random.random

    def spy_randint(a, b):
        v = real_randint(a, b)
        drawn.setdefault("pickpoints", []).append(v)
        drawn["num_particle"] = b + 1
        return v

    def spy_choice(seq):
        v = real_choice(seq)
        drawn["file_index"], drawn["n_files"] = list(seq).index(v), len(seq)
        return v

    def spy_uniform(lo, hi, size=None):
        v = real_uniform(lo, hi, size)
        drawn.setdefault("uniform", []).append(np.array(v, np.float64).copy())
        return v

    def spy_random(size=None):
        v = real_random(size)
        drawn.setdefault("random", []).append(np.array(v, np.float64).copy())
        return v

    for ci, (mesh, difficulty, seed) in enumerate(CASES):
        with tempfile.TemporaryDirectory() as tmp:
            with open(os.path.join(tmp, "x_processed.obj"), "w") as fh:
                fh.write(texts[mesh])
            drawn.clear()
            del loaded[:]
            random.seed(seed)
            np.random.seed(seed)
            box["o"] = OracleSim()
            tool = ref_fu.PickerPickPlace(num_picker=2, particle_radius=0.00625, picker_radius=0.05,
                                          picker_low=(-5, 0, -5), picker_high=(5, 5, 5))
            counter["steps"] = 0
            random.randint, random.choice = spy_randint, spy_choice
            np.random.uniform, np.random.random = spy_uniform, spy_random
            try:
                task = ref_tasks.generate_randomization(tool, cloth_mesh_path=tmp, task_difficulty=difficulty, cloth_type="mesh")
            finally:
                random.randint, random.choice = real_randint, real_choice
                np.random.uniform, np.random.random = real_uniform, real_random
            assert task is not None, f"case {ci}: seed {seed} gives None; choose another"
            assert loaded == [str(next(Path(tmp).rglob("*_processed.obj")))]
        n = len(task["particle_pos"]) // 4
        print("mesh task", ci, mesh, difficulty, "seed", seed, "V", n, "num_particle", drawn["num_particle"], "mass %.4f" %
              float(task["cloth_mass"]), "coverage %.6f" % float(task["initial_coverage"]), "flatten_area %.6f" %
              float(task["flatten_area"]), "steps", counter["steps"], "max height %.4f" %
              float(np.asarray(task["particle_pos"]).reshape(-1, 4)[:, 1].max()))
        pre = f"c{ci}_"
        out[pre + "mesh"], out[pre + "difficulty"], out[pre + "seed"] = np.array(mesh), np.array(difficulty), np.array(seed)
        out[pre + "steps"] = np.array(counter["steps"])
        out[pre + "file_index"], out[pre + "n_files"] = np.array(drawn["file_index"]), np.array(drawn["n_files"])
        out[pre + "num_particle"] = np.array(drawn["num_particle"])
        out[pre + "draw_stiff"], out[pre + "draw_mass"] = drawn["uniform"][0], drawn["uniform"][1]
        out[pre + "draw_pickpoints"] = np.array(drawn["pickpoints"])
        if difficulty == "hard":
            out[pre + "draw_height"] = drawn["random"][0]
        else:
            out[pre + "draw_displacements"] = np.stack(drawn["uniform"][2:])   # as drawn (y is overwritten with 0.2 afterwards)
        for k in ("particle_pos", "particle_vel", "shape_pos"):
            out[pre + k] = np.asarray(task[k], np.float32)
        out[pre + "phase"] = np.asarray(task["phase"], np.int32)
        out[pre + "mesh_verts"] = np.asarray(task["mesh_verts"], np.float64)
        for k in ("mesh_stretch_edges", "mesh_bend_edges", "mesh_shear_edges", "mesh_faces"):
            out[pre + k] = np.asarray(task[k], np.int32)
        for k in ("cloth_size", "cloth_stiff"):
            out[pre + k] = np.asarray(task[k])
        for k in ("initial_coverage", "flatten_area", "cloth_mass"):
            out[pre + k] = np.array(float(task[k]))
        out[pre + "flip_mesh"], out[pre + "task_difficulty"] = np.array(int(task["flip_mesh"])), np.array(str(task["task_difficulty"]))
    path = os.path.join(HERE, "mesh_task_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
