"""The probe on the GPU: fs_lattice_actions (csrc/fs_action.hip, ActionSelector.lattice) on constructed inputs against the CPU
oracle cell for cell, and probe.run_episodes end to end -- the followed trajectory is evaluate.run_episodes' own, every measured
cell is the reward of that action executed alone from a fresh reset, and neither the number of passes nor the off-cloth filter
changes a cell.  All comparisons are exact."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import probe_reference as ref

pytestmark = pytest.mark.gpu

# ---- 1. fs_lattice_actions ----------------------------------------------------------------------------------------------------
N, PRIMS, ROTATIONS, D, G, S, DRAG, PLACE, REACH = 2, ["fling", "place"], [-35.0, 20.0], 32, 4, 48, 6, 5, 0.71
SCALES = [np.array([0.7, 1.1]), np.array([0.9, 1.3])]   # (no rotation 0 at scale 1: its transformed coordinates are integers)
T = len(ROTATIONS) * 2
RADII = (0, 1, 3)


def lattice_requests():
    """Every (episode, primitive, transform) map at strides 1, 3 and 5: stride 1 over all rows (reach points that leave the
    map included) and 12 columns -- 384 cells, more than one trip of the workgroup's 256 threads --, strides 3 and 5 from
    origins that do not divide the map.  No lattice has column D / 2: the map's centre pixel is the fixed point of every
    transform and lands on the integer 24 exactly, the one place where no choice of rotation or scale keeps a truncation away
    from its boundary."""
    shapes = [(0, 4, 1, 32, 12), (1, 2, 3, 11, 10), (4, 3, 5, 6, 6)]
    return [(e, p, t, y0, z0, stride, gy, gz) for e in range(N) for p in range(len(PRIMS)) for t in range(T)
            for y0, z0, stride, gy, gz in shapes]


def make_lattice_case():
    """(values [N, P, T, D, D] with 10 % NaN, depth [N, S, S]): background 2.0, a cloth blob per episode -- episode 1's touches
    the image border, so discs around its grasp points are clipped --, a few exact 0.0 pixels."""
    rng = np.random.default_rng(5)
    values = rng.standard_normal((N, len(PRIMS), T, D, D)).astype(np.float32)
    values[rng.random(values.shape) < 0.1] = np.nan
    yy, xx = np.mgrid[0:S, 0:S]
    depth = np.full((N, S, S), 2.0, np.float32)
    for e, (cx, cy, r) in enumerate([(22.0, 26.0, 15.0), (33.0, 20.0, 21.0)]):
        blob = (xx - cx) ** 2 + (yy - cy) ** 2 < r * r
        depth[e][blob] = (1.97 - 0.04 * rng.random(int(blob.sum()))).astype(np.float32)
        depth[e][rng.random((S, S)) < 0.02] = 0.0
    return values, depth


@pytest.fixture(scope="module")
def lattice_case():
    values, depth = make_lattice_case()
    cfgs = [ref.oracle_cfg(depth[e], SCALES[e], ROTATIONS, D, G, DRAG, PLACE, REACH) for e in range(N)]
    requests = lattice_requests()
    return dict(values=values, depth=depth, cfgs=cfgs, requests=requests, oracle=ref.lattice_oracle(PRIMS, cfgs, requests))


def _selector():
    from flingbot_amd.action import ActionSelector

    return ActionSelector(PRIMS, ROTATIONS, D, G, DRAG, PLACE, REACH)


def test_lattice_inputs_meet_the_condition(lattice_case):
    """On the CPU, before anything is compared: no cell of any request sits at a rounding boundary, so device and oracle have
    to agree on EVERY cell; and the inputs hold what the kernel can get wrong."""
    oracle, depth = lattice_case["oracle"], lattice_case["depth"]
    print("reach margin", oracle["reach_margin"], "pixel margin", oracle["pixel_margin"], "cut by reach", oracle["reach_cut"])
    assert oracle["reach_margin"] > 1e-9 and oracle["pixel_margin"] > 1e-9
    assert oracle["reach_cut"] >= 20, "the reach limit cuts through the lattices"
    valid = np.concatenate([v.ravel() for v, _ in oracle["cells"]])
    assert 0.1 < valid.mean() < 0.9
    assert (depth == 0.0).any() and (depth == 2.0).any() and np.isnan(lattice_case["values"]).mean() > 0.05
    assert (depth[1][:, -1] != 2.0).any(), "cloth touches the image border"
    for radius in (1, 3):
        codes = np.concatenate([c.ravel() for c in ref.lattice_codes(oracle, lattice_case["cfgs"], lattice_case["requests"], radius)])
        assert {1, 3, 5, 7} <= set(codes.tolist()), "every combination of the on-cloth bits on a valid cell"


@pytest.mark.parametrize("radius", RADII)
def test_lattice_equals_oracle(gpu_required, lattice_case, radius):
    sel = _selector()
    requests = lattice_case["requests"]
    valid, on1, on2, value = sel.lattice(torch.tensor(lattice_case["values"]).cuda(), SCALES, torch.tensor(lattice_case["depth"]).cuda(),
                                         requests, radius)
    want = ref.lattice_codes(lattice_case["oracle"], lattice_case["cfgs"], requests, radius)
    assert valid.shape == (len(requests), 32, 12) and value.dtype == np.float32
    for k, (e, p, t, y0, z0, stride, gy, gz) in enumerate(requests):
        code = valid[k, :gy, :gz] * 1 + on1[k, :gy, :gz] * 2 + on2[k, :gy, :gz] * 4
        assert np.array_equal(code, want[k]), (k, requests[k])
        cells = lattice_case["values"][e, p, t, y0:y0 + gy * stride:stride, z0:z0 + gz * stride:stride]
        assert np.array_equal(value[k, :gy, :gz].view(np.uint32), cells.view(np.uint32)), (k, requests[k])   # NaN bits too
        assert not valid[k, gy:].any() and not valid[k, :, gz:].any() and np.isnan(value[k, gy:]).all()
        if radius == 0:
            assert np.array_equal(on1[k], valid[k]) and np.array_equal(on2[k], valid[k])


def test_lattice_refusals(gpu_required, lattice_case):
    """Every refusal returns an error that names the entry point and launches nothing: the outputs keep their fill."""
    from flingbot_amd import sim as fsim

    sel, lib = _selector(), fsim.load_library()
    values, depth = torch.tensor(lattice_case["values"]).cuda(), torch.tensor(lattice_case["depth"]).cuda()
    from flingbot_amd.action import CAMERA_FOV_DEG, KINDS, compute_intrinsics
    mats = np.ascontiguousarray([sel._transform_mats(S, D, s) for s in SCALES], np.float64)
    kinds = np.ascontiguousarray([KINDS[a] for a in PRIMS], np.int32)
    fx = float(compute_intrinsics(CAMERA_FOV_DEG, S)[0, 0])
    pose = np.ascontiguousarray(sel.pose, np.float64)
    work = fsim.work_buffer("fs_lattice_actions_work_bytes", "cuda:0", N, T, 2, 64)
    dp = C.POINTER(C.c_double)
    good = np.array([[0, 0, 0, 4, 4, 3, 8, 8], [1, 1, 3, 0, 0, 1, 8, 8]], np.int32)

    def call(table=good, m=None, **kw):
        code, value = np.full((2, 64), 255, np.uint8), np.full((2, 64), 7.0, np.float32)
        table = np.ascontiguousarray(table, np.int32)   # (alive until the call returns)
        a = dict(values=values.data_ptr(), kinds=kinds.ctypes.data_as(C.POINTER(C.c_int)), mats=mats.ctypes.data_as(dp),
                 depth=depth.data_ptr(), pose=pose.ctypes.data_as(dp), left=sel.left_arm_base.ctypes.data_as(dp),
                 right=sel.right_arm_base.ctypes.data_as(dp), requests=table.ctypes.data,
                 code=code.ctypes.data_as(C.POINTER(C.c_ubyte)), value=value.ctypes.data_as(C.POINTER(C.c_float)),
                 work=work.data_ptr())
        a.update(kw)
        rc = lib.fs_lattice_actions(a["values"], N, len(PRIMS), a["kinds"], T, D, G, DRAG, PLACE, a["mats"], a["depth"], S, fx,
                                    a["pose"], a["left"], a["right"], REACH, 0.3, 0.02, a["requests"], len(table) if m is None else m,
                                    1, a["code"], a["value"], a["work"], torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc, code, value

    rc, code, value = call()
    assert rc == 0 and (code != 255).all() and np.array_equal(value[0].reshape(8, 8), lattice_case["values"][0, 0, 0, 4:28:3, 4:28:3],
                                                              equal_nan=True)

    def edited(column, v, row=1):
        t = good.copy()
        t[row, column] = v
        return t

    bad = [dict(kw) for kw in ({"values": None}, {"kinds": None}, {"mats": None}, {"depth": None}, {"pose": None}, {"left": None},
                               {"right": None}, {"requests": None}, {"code": None}, {"value": None}, {"work": None},
                               {"work": work.data_ptr() + 4}, {"m": 0}, {"m": 65536})]
    bad += [dict(table=edited(5, 0)), dict(table=edited(6, 0)), dict(table=edited(7, 0)),
            dict(table=edited(6, 4097)), dict(table=edited(7, 600)),          # 8 x 600 = 4800 cells
            dict(table=edited(3, -1)), dict(table=edited(3, 25)),             # 25 + 7 = 32 leaves [0, D)
            dict(table=edited(4, 11, row=0)),                                 # 11 + 7 * 3 = 32
            dict(table=edited(0, 2)), dict(table=edited(0, -1)), dict(table=edited(1, 2)), dict(table=edited(2, 4)),
            dict(table=edited(2, -1))]
    for kw in bad:
        rc, code, value = call(**kw)
        assert rc != 0 and b"fs_lattice_actions" in lib.fs_last_error(), kw
        assert (code == 255).all() and (value == 7.0).all(), kw


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------
E_ROTATIONS, E_SCALES, SEED, STRIDE = 3, (1.0, 1.5), 2, 16


def _env_policy(slots, **env_kwargs):
    from flingbot_amd import nets, sim as fsim
    from flingbot_amd.env import BatchedFlingEnv

    ctx = fsim.FlingSim(n_envs=slots, solver=0)
    env = BatchedFlingEnv(ctx, image_dim=128, num_rotations=E_ROTATIONS, scale_factors=E_SCALES, episode_length=2, **env_kwargs)
    torch.manual_seed(SEED)
    policy = nets.MaximumValuePolicy(action_primitives=["fling"], num_rotations=E_ROTATIONS, scale_factors=list(env.scale_factors),
                                     obs_dim=64, pix_grasp_dist=8, pix_drag_dist=8, pix_place_dist=5, rgb_only=True,
                                     depth_only=False, action_expl_prob=0.0, action_expl_decay=1.0, value_expl_prob=0.0,
                                     value_expl_decay=1.0, device="cuda:0")
    return ctx, env, policy


@pytest.fixture(scope="module")
def tasks(gpu_required):
    from flingbot_amd import sim as fsim, tasks as ftasks

    random.seed(SEED); np.random.seed(SEED)
    gen = fsim.FlingSim(n_envs=2, solver=0)
    made = ftasks.generate_tasks(gen, [ftasks.draw_task_parameters(min_cloth_size=24, strict_min_edge_length=24, max_cloth_size=32)
                                       for _ in range(2)])
    gen.close()
    assert all(t is not None for t in made)
    return made


def _probe(tasks, slots, **kwargs):
    from flingbot_amd import probe

    ctx, env, policy = _env_policy(slots, record_experience=True)
    got = probe.run_episodes(policy, env, tasks, STRIDE, steps=(0,), **kwargs)
    ctx.close()
    return got


@pytest.fixture(scope="module")
def probed(tasks):
    """The probed run every test below reads: 2 tasks and 18 free slots -- one pass."""
    return _probe(tasks, 20)


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)
    return a == b


MAP_ARRAYS = ("predicted", "valid", "on_cloth1", "on_cloth2", "measured", "terminated")


def test_followed_trajectory_equals_run_episodes(gpu_required, tasks, probed):
    from flingbot_amd import evaluate

    ctx, env, policy = _env_policy(2, record_experience=True)
    want = evaluate.run_episodes(policy, env, tasks)
    ctx.close()
    assert set(want) <= set(probed)
    for key in want:
        assert _same(probed[key], want[key]), key
    block = probed["probe"]
    assert block["stride"] == STRIDE and block["steps_probed"] == [0] and len(block["maps"]) == 2
    assert all(m["shape"] == [3, 3] and m["step"] == 0 for m in block["maps"])
    assert block["n_executed"] == sum(m["n_executed"] for m in block["maps"]) >= 4, "a run that executed next to nothing shows nothing"
    assert block["simulation_steps"] > 0


def test_chosen_cell_is_executed_first_in_rank(gpu_required, probed):
    recs = probed["lane_records"]
    for m in probed["probe"]["maps"]:
        i, j = m["chosen_cell"]
        assert [m["origin"][0] + i * STRIDE, m["origin"][1] + j * STRIDE] == m["chosen_pixel"]
        assert m["valid"][i, j] and not np.isnan(m["measured"][i, j])
        mine = [r for r in recs if r["task"] == m["task"] and r["step"] == 0]
        assert len(mine) == m["n_executed"] == int((~np.isnan(m["measured"])).sum())
        assert sorted(r["rank"] for r in mine) == list(range(len(mine)))
        first = next(r for r in mine if r["rank"] == 0)
        y, z = m["chosen_pixel"]
        assert first["experience"][0]["actions"][y, z] and int(first["experience"][0]["max_indices"][0]) == m["transform_index"]
        followed = probed["records"][m["task"]]["rewards"][0]
        assert first["rewards"] == [followed] and m["measured"][i, j] == np.float32(followed)
        assert m["stats"]["chosen_reward"] == float(np.float32(followed)) and m["stats"]["lattice_regret"] >= 0


def test_cells_equal_actions_executed_alone(gpu_required, tasks, probed):
    """Every executed cell once more, alone: the same task reset into a fresh context, the cell's action built by
    `_candidate` and the host's `_on_cloth` from that reset's own observation, one step_actions on one slot."""
    maps = probed["probe"]["maps"]
    cells = [(m, int(i), int(j)) for m in maps for i, j in np.argwhere(~np.isnan(m["measured"]))]
    ctx, env, _ = _env_policy(len(cells))
    env.reset([tasks[m["task"]] for m, _, _ in cells])
    for slot, (m, i, j) in enumerate(cells):
        depth = env.pretransform_depth[slot]
        params = env.selector._candidate(m["primitive"], m["transform_index"], m["origin"][0] + i * STRIDE, m["origin"][1] + j * STRIDE,
                                         env.adaptive_scale_factors[slot], depth)
        assert params is not None
        pix = params["pretransform_pixels"]
        params["p1_grasp_cloth"] = env._on_cloth(depth, (pix[0][1], pix[0][0]))
        params["p2_grasp_cloth"] = env._on_cloth(depth, (pix[1][1], pix[1][0]))
        assert (params["p1_grasp_cloth"], params["p2_grasp_cloth"]) == (bool(m["on_cloth1"][i, j]), bool(m["on_cloth2"][i, j]))
        rewards, _ = env.step_actions([slot], {slot: (m["primitive"], params)})
        assert np.float32(rewards[slot]) == m["measured"][i, j], (m["task"], i, j)
        assert bool(env.terminate[slot]) == bool(m["terminated"][i, j])
    ctx.close()


def test_passes_do_not_change_a_cell(gpu_required, tasks, probed):
    few = _probe(tasks, 2 + 4)       # 4 free slots: several passes
    assert few["probe"]["n_executed"] == probed["probe"]["n_executed"] > 4
    for a, b in zip(few["probe"]["maps"], probed["probe"]["maps"]):
        for key in MAP_ARRAYS:
            assert _same(a[key], b[key]), key
        assert a["stats"] == b["stats"]
    assert _same(few["lane_records"], probed["lane_records"])
    assert _same(few["coverage_steps"], probed["coverage_steps"])


def test_off_cloth_cells_are_a_superset(gpu_required, tasks, probed):
    every = _probe(tasks, 20, skip_off_cloth=False)
    for a, b in zip(every["probe"]["maps"], probed["probe"]["maps"]):
        done_a, done_b = ~np.isnan(a["measured"]), ~np.isnan(b["measured"])
        assert (done_a | ~done_b).all() and np.array_equal(done_a, a["valid"])
        assert np.array_equal(a["measured"][done_b], b["measured"][done_b])
        for key in ("predicted", "valid", "on_cloth1", "on_cloth2"):
            assert _same(a[key], b[key]), key
        skipped = b["valid"] & ~done_b
        assert not (b["on_cloth1"] | b["on_cloth2"])[skipped].any()


# ---- 2. fs_probe_panels -------------------------------------------------------------------------------------------------------
PD, PS = 32, 48


def _probe_records(seed):
    """Four records at D = 32, S = 48 that between them hold: a lattice with all four cell kinds (finite, valid and not
    executed, invalid, and map pixels outside it) with the chosen cell in its last corner; stride 1 from the map's corner; a
    null after; vmax == vmin; NaN and out-of-range values on both maps; a measured value on an invalid cell (drawn: a finite
    cell is jet whatever its code says).  Host arrays."""
    from flingbot_amd.report import action_overlays
    rng = np.random.default_rng(seed)
    lattices = [((4, 5), 3, (8, 7), (7, 6)), ((0, 0), 1, (32, 32), (0, 31)), ((6, 2), 5, (5, 6), (0, 0)), ((9, 9), 4, (1, 1), None)]
    out = []
    for k, (origin, stride, (gy, gz), chosen) in enumerate(lattices):
        stack = rng.uniform(-0.2, 1.2, (4, PD, PD)).astype(np.float32)
        value_map = rng.standard_normal((PD, PD)).astype(np.float32)
        value_map[rng.random((PD, PD)) < 0.05] = np.nan
        valid = rng.random((gy, gz)) < 0.7
        measured = np.where(valid & (rng.random((gy, gz)) < 0.7), rng.standard_normal((gy, gz)), np.nan).astype(np.float32)
        if k == 0:
            valid[0, 0], measured[0, 0] = False, 0.25
            valid[1, 1], measured[1, 1] = True, np.nan
            valid[2, 2], measured[2, 2] = False, np.nan
            measured[3, 3] = np.inf
        vrange = np.array([[-1.0, 1.5], [-0.5, 0.5], [0.3, 0.3], [-2.0, 2.0]][k], np.float32)
        after = None if k == 1 else rng.uniform(-0.2, 1.2, (3 + k % 2, PS, PS)).astype(np.float32)
        small = action_overlays(("fling", "place", "drag", "stretchdrag")[k], np.array([[20, 11], [12, 11 + k]]), 1)
        out.append(dict(stack=stack, value_map=value_map, range=vrange, measured=measured, valid=valid, origin=origin, stride=stride,
                        chosen_cell=chosen, after=after, small=small))
    return out


def _probe_item(rec):
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    return dict(rec, stack=up(rec["stack"]), value_map=up(rec["value_map"]), range=up(rec["range"]), after=up(rec["after"]),
                measured=up(rec["measured"]), valid=up(rec["valid"].astype(np.uint8)))


@pytest.mark.parametrize("panel", [40, 96])
def test_probe_panels_match_reference(gpu_required, panel):
    from flingbot_amd import report

    host = _probe_records(seed=panel)
    dev = [_probe_item(r) for r in host]
    got = report.compose_probe(dev, panel=panel)
    assert got.dtype == np.uint8 and got.shape == (len(host), panel, 4 * panel, 3)
    table = report.jet_table()
    for k, r in enumerate(host):
        want = ref.strip(table, r["stack"], r["value_map"], r["range"], r["measured"], r["valid"], r["origin"], r["stride"],
                         r["chosen_cell"], r["after"], r["small"], panel, PS)
        diff = np.argwhere(got[k] != want)
        assert diff.size == 0, (k, len(diff), diff[:4], got[k][tuple(diff[0][:2])], want[tuple(diff[0][:2])])
        assert (report.compose_probe([dev[k]], panel=panel)[0] == got[k]).all(), k       # a strip is a function of its own record
    assert not got[1][:, 3 * panel:].any()                                               # a null after: black
    # the four cell kinds and the frame, looked at directly on record 0 at panel 96 = 3 D (a source pixel is 3 x 3)
    if panel == 96:
        m = got[0][:, 2 * panel:3 * panel]
        at = lambda y, z: tuple(int(c) for c in m[3 * y + 1, 3 * z + 1])   # noqa: E731
        assert at(4 + 3, 5 + 3) == (128, 128, 128) and at(4 + 6, 5 + 6) == (64, 64, 64) and at(0, 0) == (0, 0, 0)
        assert at(4 + 9, 5 + 9) == (128, 128, 128) or at(4 + 9, 5 + 9) == (64, 64, 64)   # an infinite reward is not drawn as one
        assert at(4, 5) == tuple(int(c) for c in ref.ref.jet(table, np.float32([[0.25]]), -1.0, 1.5)[0, 0])
        assert at(4 + 21 - 1, 5 + 18 - 1) == (255, 255, 255) and at(4 + 21 + 1, 5 + 18 + 1) == (255, 255, 255)   # the frame
        assert at(28, 5) == (0, 0, 0)                                                    # past the last row's cell, which ends at 4 + 7 * 3 + 1 = 26
    # vmax == vmin: entry 0 of the table on both maps
    cells = got[2][:, panel:2 * panel].reshape(-1, 3)
    assert (cells == table[0]).all()


def test_probe_panels_default_range_and_refusals(gpu_required):
    from flingbot_amd import report, sim as fsim

    lib = fsim.load_library()
    rec = _probe_records(seed=1)[0]
    predicted = rec["value_map"][4:4 + 8 * 3:3, 5:5 + 7 * 3:3]
    item = dict(_probe_item(rec), range=None, predicted=predicted)
    done = np.isfinite(rec["measured"])
    v = np.concatenate([predicted[done & np.isfinite(predicted)], rec["measured"][done]])
    want = ref.strip(report.jet_table(), rec["stack"], rec["value_map"], np.float32([v.min(), v.max()]), rec["measured"], rec["valid"],
                     rec["origin"], rec["stride"], rec["chosen_cell"], rec["after"], rec["small"], 40, PS)
    assert (report.compose_probe([item], panel=40)[0] == want).all()
    for change, word in ((dict(stride=0), "stride"), (dict(origin=(4, 14)), "lattice"), (dict(origin=(-1, 5)), "lattice"),
                         (dict(chosen_cell=(8, 0)), "chosen"), (dict(small=[(7, 0, 0, 1, 1, 1, 0, 0, 0)]), "kind"),
                         (dict(small=rec["small"] * 3), None)):
        with pytest.raises((RuntimeError, ValueError)) as err:
            report.compose_probe([dict(_probe_item(rec), **change)], panel=40)
        if word is not None:
            assert "fs_probe_panels" in str(err.value) and word in str(err.value), change
            assert lib.fs_last_error().decode() in str(err.value)
    table = np.zeros(1, report.PROBE_RECORD)
    out = torch.zeros((1, 8, 32, 3), dtype=torch.uint8, device="cuda:0")
    work = fsim.work_buffer("fs_probe_panels_work_bytes", "cuda:0", 1)
    stream = torch.cuda.current_stream().cuda_stream
    for args in ((None, 1, PD, PS, 8, out.data_ptr(), work.data_ptr()), (table.ctypes.data, 1, PD, PS, 8, None, work.data_ptr()),
                 (table.ctypes.data, 1, PD, PS, 8, out.data_ptr(), None), (table.ctypes.data, 0, PD, PS, 8, out.data_ptr(), work.data_ptr()),
                 (table.ctypes.data, 65536, PD, PS, 8, out.data_ptr(), work.data_ptr()),
                 (table.ctypes.data, 1, 0, PS, 8, out.data_ptr(), work.data_ptr()), (table.ctypes.data, 1, PD, 4097, 8, out.data_ptr(), work.data_ptr()),
                 (table.ctypes.data, 1, PD, PS, 0, out.data_ptr(), work.data_ptr()), (table.ctypes.data, 1, PD, PS, 8, out.data_ptr(), work.data_ptr() + 4),
                 (table.ctypes.data, 1, PD, PS, 8, out.data_ptr() + 1, work.data_ptr()),
                 (table.ctypes.data, 1, PD, PS, 8, out.data_ptr(), work.data_ptr())):      # the last: a record of null pointers
        assert lib.fs_probe_panels(*args, stream) == -1 and b"fs_probe_panels" in lib.fs_last_error(), args
    torch.cuda.synchronize()
    assert not out.any()
