"""Development helper: the evaluation loop on shirts against rectangles of equal particle count (EXPERIMENTS, "shirts").

Shirt-A-like meshes (tests/shirt_meshes.py: two joined layers, general rest-pose filter) scaled to about 4 k and 9 k
vertices, and grid cloths of the same particle counts; a handful of hard tasks of each kind is generated and repeated to fill
the slots.  evaluate.run_tasks then runs one action per episode on 64 and on 192 slots, mesh and grid ALTERNATING in one
process on one GPU, `--repeats` times each; flings/s and episode-steps/s per run, their medians and spreads, the mesh/grid
ratio, the iterate kernel form of each run's LAST solver launch (FlingSim.last_kernel_form, read once after run_tasks: a
run whose launches shrink as episodes end may have used a larger launch's form earlier, which is why a kind can show two
forms over its repeats) and the adjacency bytes a particle-iteration reads for the cloth are printed as JSON lines.

--kinds adds the MIXED case: shirts in the even slots, grids of equal particle count in the odd ones -- a task set as README
describes it.  --solver lists the fs_set_solver ids every (kind, slots) case is run under, alternating inside each repeat:
id 1 (FS_SOLVER_STREAM) picks one iterate kernel per launch as the code did before the per-episode forms existed, so
`--solver 1 0` is the A/B of those forms on the same tasks in one process (EXPERIMENTS R29.1): 0 (AUTO) takes them above the
latency threshold, 10 at every launch size.

usage: shirt_eval_timing.py [--sizes 4000 9000] [--slots 64 192] [--repeats 5] [--actions 1] [--distinct 4]
                            [--kinds mesh grid mixed] [--solver 1 0] [--out FILE]"""
import argparse
import json
import math
import os
import random
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))   # the synthetic shirts live with the tests that pin them (tests/shirt_meshes.py);
                                                  # this developer tool borrows them rather than keep a second generator
import numpy as np
import torch
import shirt_meshes
from flingbot_amd import nets, sim as fsim, tasks as ftasks
from flingbot_amd.env import BatchedFlingEnv
from flingbot_amd.evaluate import run_tasks

FORMS = {getattr(fsim, k): k[8:] for k in dir(fsim) if k.startswith("FS_FORM_")}


def scaled_shirt(target):
    """shirt_a with the default proportions (body 12 x 16, sleeves 5 x 5, neck 4) scaled until it has about `target` vertices."""
    best = None
    for k in range(10, 200):
        s = k / 10.0
        dims = dict(body_w=round(12 * s), body_h=round(16 * s), sleeve_w=round(5 * s), sleeve_h=round(5 * s), neck=max(2, round(4 * s)))
        layer = (dims["body_w"] + 1) * (dims["body_h"] + 1) + 2 * dims["sleeve_w"] * (dims["sleeve_h"] + 1)
        if best is None or abs(2 * layer - target) < abs(2 * best[0] - target):
            best = (layer, dims)
    return shirt_meshes.shirt_a(**best[1])


def grid_params(n):
    """draw_task_parameters' dictionary for a hard task on a dimx x dimz grid of about n particles (sizes fixed, the rest drawn)."""
    dimx = int(math.sqrt(n))
    dimz = int(round(n / dimx))
    return dict(cloth_size=[dimx, dimz], cloth_stiff=np.random.uniform(0.85, 0.95, 3), cloth_mass=np.random.uniform(0.2, 2.0),
                task_difficulty='hard', pickpoint=random.randint(0, dimx * dimz - 1), height=np.random.random(1) * 1.0 + 0.5)


def adjacency_bytes(task):
    """Bytes of adjacency one particle-iteration of the streaming solver reads for this cloth: 16 where the host built the
    one-byte spring codes (a canonical grid, or any cloth of max_deg <= 16 with <= 255 distinct springs: fs_scene.h), else
    the ELL arrays, 12 bytes (neighbour id, rest length, stiffness) in each of max_deg slots."""
    h = fsim.host_scene(*ftasks.task_scene_arguments(task))
    coded = bool((h["stream_dict"] != 0xffffffff).any()) and h["max_deg"] <= 16
    return dict(max_deg=int(h["max_deg"]), coded=coded, bytes_per_particle_iteration=16 if coded else 12 * int(h["max_deg"]),
                mesh_ok=int(h["mesh_ok"]), mesh_word_bytes_per_particle_iteration=8 * int(h["max_deg"]) if h["mesh_ok"] else None,
                restnear_ok=h["flags"]["restnear_ok"], particles=int(h["n"]), springs=int(h["m"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4000, 9000])
    ap.add_argument("--slots", type=int, nargs="+", default=[64, 192])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--actions", type=int, default=1)
    ap.add_argument("--distinct", type=int, default=4, help="generated tasks per kind (repeated to fill the slots)")
    ap.add_argument("--kinds", nargs="+", default=["mesh", "grid"], choices=["mesh", "grid", "mixed"])
    ap.add_argument("--solver", type=int, nargs="+", default=[0], help="fs_set_solver ids, alternating inside every repeat")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    random.seed(0); np.random.seed(0); torch.manual_seed(0)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    for size in a.sizes:
        with tempfile.TemporaryDirectory() as tmp:
            with open(os.path.join(tmp, "shirt_processed.obj"), "w") as fh:
                fh.write(scaled_shirt(size))
            mesh_params = [ftasks.draw_task_parameters(cloth_type='mesh', cloth_mesh_path=tmp) for _ in range(a.distinct)]
        n_vertices = len(mesh_params[0]["mesh_verts"])
        sets = {}
        for kind, params in (("mesh", mesh_params), ("grid", [grid_params(n_vertices) for _ in range(a.distinct)])):
            if kind not in a.kinds and "mixed" not in a.kinds:
                continue
            gen = fsim.FlingSim(n_envs=a.distinct, solver=0)
            t0 = time.perf_counter()
            sets[kind] = [t for t in ftasks.generate_tasks(gen, params) if t is not None]
            gen.close()
            emit(dict(stage="generate", kind=kind, target=size, tasks=len(sets[kind]), seconds=round(time.perf_counter() - t0, 2),
                      **adjacency_bytes(sets[kind][0])))
        for slots in a.slots:
            cases = [(kind, solver) for kind in a.kinds for solver in a.solver]
            runs = {case: [] for case in cases}
            for rep in range(a.repeats):
                for kind, solver in cases:             # alternating: drift of the machine hits all alike
                    if kind == "mixed":                # shirts in the even slots, grids in the odd ones
                        tasks = [sets["grid" if i % 2 else "mesh"][(i // 2) % len(sets["grid" if i % 2 else "mesh"])] for i in range(slots)]
                    else:
                        tasks = [sets[kind][i % len(sets[kind])] for i in range(slots)]
                    ctx = fsim.FlingSim(n_envs=slots, solver=solver)
                    env = BatchedFlingEnv(ctx, episode_length=a.actions)
                    policy = nets.MaximumValuePolicy(action_primitives=["fling"], num_rotations=12, scale_factors=list(env.scale_factors),
                                                     obs_dim=64, pix_grasp_dist=8, pix_drag_dist=8, pix_place_dist=5, rgb_only=True,
                                                     depth_only=False, action_expl_prob=0.0, action_expl_decay=1.0,
                                                     value_expl_prob=0.0, value_expl_decay=1.0, device="cuda:0")
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    stats = run_tasks(policy, env, tasks)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    flings = sum(stats["action_primitive_counts"].values())
                    slot_forms = ctx.last_slot_forms()
                    row = dict(stage="run", kind=kind, solver=solver, target=size, particles=len(tasks[0]["particle_pos"]) // 4, slots=slots, rep=rep,
                               slot_forms={FORMS.get(f, str(f)): slot_forms.count(f) for f in sorted(set(slot_forms))},
                               seconds=round(dt, 3), flings=flings, flings_per_s=round(flings / dt, 2),
                               episode_steps=stats["simulation_steps"], episode_steps_per_s=round(stats["simulation_steps"] / dt, 1),
                               kernel_form=FORMS.get(ctx.last_kernel_form(), str(ctx.last_kernel_form())))
                    ctx.close()
                    runs[(kind, solver)].append(row)
                    emit(row)
            summary = dict(stage="summary", target=size, slots=slots, repeats=a.repeats)
            for (kind, solver), got in runs.items():
                name = kind if len(a.solver) == 1 else f"{kind}_solver{solver}"
                for key in ("flings_per_s", "episode_steps_per_s"):
                    v = np.array([r[key] for r in got])
                    summary[f"{name}_{key}_median"] = float(np.median(v))
                    summary[f"{name}_{key}_min"], summary[f"{name}_{key}_max"] = float(v.min()), float(v.max())
                summary[f"{name}_kernel_forms"] = sorted({r["kernel_form"] for r in got})
            if len(a.solver) == 1 and "mesh" in a.kinds and "grid" in a.kinds:
                for key in ("flings_per_s", "episode_steps_per_s"):
                    summary[f"mesh_over_grid_{key}"] = round(summary[f"mesh_{key}_median"] / summary[f"grid_{key}_median"], 3)
            base = a.solver[0]                         # every other id against the first one listed, per kind
            for kind in a.kinds:
                for solver in a.solver[1:]:
                    b, c = f"{kind}_solver{base}_episode_steps_per_s", f"{kind}_solver{solver}_episode_steps_per_s"
                    summary[f"{kind}_solver{solver}_over_solver{base}"] = round(summary[c + "_median"] / summary[b + "_median"], 4)
                    summary[f"{kind}_solver{base}_spread"] = round(summary[b + "_max"] - summary[b + "_min"], 1)
                    summary[f"{kind}_solver{solver}_gain"] = round(summary[c + "_median"] - summary[b + "_median"], 1)
            emit(summary)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
