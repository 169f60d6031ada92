"""Development helper: one large streaming launch of shirts (or of shirts and grids, alternating slots) stepped first under
FS_SOLVER_STREAM (one iterate kernel per launch: fs_k_iterate<false>) and then under FS_SOLVER_STREAM_MESH (fs_k_iterate_mesh /
fs_k_iterate_mixed), so that a `rocprofv3 --kernel-trace --stats` run of this script shows the three kernels' times on the same
state (scripts/profile_mesh_forms.sh; EXPERIMENTS R29.1).  The cloths are perturbed by seeded noise of 2 mm and fall freely:
springs act, contacts are few -- the iterate kernels' times are those of a launch whose cost is the spring phase.

usage: mesh_forms_trace.py {mesh,mixed} [--size 9000] [--slots 192] [--frames 3]"""
import argparse
import json
import math
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np
from flingbot_amd import sim as fsim, tasks as ftasks
from shirt_eval_timing import FORMS, scaled_shirt


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("launch", choices=["mesh", "mixed"])
    ap.add_argument("--size", type=int, default=9000)
    ap.add_argument("--slots", type=int, default=192)
    ap.add_argument("--frames", type=int, default=3)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "shirt_processed.obj")
        with open(path, "w") as fh:
            fh.write(scaled_shirt(a.size))
        verts, faces, stretch, bend, shear = ftasks.load_cloth(path)
    n = len(verts)
    dimx = int(math.sqrt(n))
    sp = np.array([0, 0.15, 0, -1, -1, 0.9, 0.9, 0.9, 2, 0, 2, 0, np.pi / 2, -np.pi / 2, 0, 720, 720, 0.5, 0], np.float32)
    grid_sp = sp.copy()
    grid_sp[3:5] = [dimx, int(round(n / dimx))]
    mesh = (verts.reshape(-1), stretch.reshape(-1), bend.reshape(-1), shear.reshape(-1), faces.reshape(-1))
    ctx = fsim.FlingSim(n_envs=a.slots, solver=fsim.FS_SOLVER_STREAM)
    for e in range(a.slots):
        if a.launch == "mixed" and e % 2:
            ctx.set_scene(e, grid_sp)
        else:
            ctx.set_scene(e, sp, *mesh)
        pos = ctx.get_positions(e).reshape(-1, 4).copy()
        pos[:, :3] += (np.random.RandomState(e).randn(len(pos), 3) * 0.002).astype(np.float32)
        ctx.set_positions(e, pos.ravel())
    for solver in (fsim.FS_SOLVER_STREAM, fsim.FS_SOLVER_STREAM_MESH):
        ctx.set_solver(solver)
        ms = ctx.step_timed(a.frames)
        forms = ctx.last_slot_forms()
        print(json.dumps(dict(launch=a.launch, solver=solver, slots=a.slots, shirt_particles=n, frames=a.frames,
                              ms_per_frame=round(ms / a.frames, 3), kernel_form=FORMS.get(ctx.last_kernel_form()),
                              slot_forms={FORMS.get(f, str(f)): forms.count(f) for f in sorted(set(forms))})), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
