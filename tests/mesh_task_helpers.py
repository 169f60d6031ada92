"""Shared by the mesh-task tests: the golden file of tests/golden/make_mesh_task_golden.py and the comparison against it."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden():
    return np.load(os.path.join(GOLD, "mesh_task_golden.npz"))


def n_cases():
    return int(golden()["n_cases"])


def write_case_mesh(g, ci, directory):
    path = os.path.join(str(directory), "x_processed.obj")
    with open(path, "w") as fh:
        fh.write(str(g["obj_" + str(g[f"c{ci}_mesh"])]))
    return path


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def check_task_against_golden(task, g, ci):
    assert task is not None and task["task_difficulty"] == str(g[f"c{ci}_task_difficulty"]) and task["flip_mesh"] == 0
    assert np.asarray(task["cloth_size"]).tolist() == [-1, -1] == g[f"c{ci}_cloth_size"].tolist()
    for k in ("particle_pos", "particle_vel", "shape_pos"):
        assert np.array_equal(bits(task[k]), bits(g[f"c{ci}_{k}"])), (ci, k)
    assert np.array_equal(task["phase"], g[f"c{ci}_phase"])
    assert abs(task["initial_coverage"] - float(g[f"c{ci}_initial_coverage"])) <= 1e-12
    assert np.array_equal(task["cloth_stiff"], g[f"c{ci}_cloth_stiff"]) and task["cloth_mass"] == float(g[f"c{ci}_cloth_mass"])
    assert abs(task["flatten_area"] - float(g[f"c{ci}_flatten_area"])) <= 1e-12 * float(g[f"c{ci}_flatten_area"])
    for k in ("mesh_verts", "mesh_faces", "mesh_stretch_edges", "mesh_bend_edges", "mesh_shear_edges"):
        assert np.asarray(task[k]).ndim == 1 and np.array_equal(task[k], g[f"c{ci}_{k}"]), k
