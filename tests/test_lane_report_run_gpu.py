"""lookahead.run_episodes with the lane report on: two generated tasks, k = 3 lanes in six slots, panel 50.  The report must
change nothing the run returns, write one strip and one line per executed step, and the strips must be the reference's
(tests/lane_report_reference.py) of what the step observed and executed."""
import json
import os
import random

import numpy as np
import pytest
import torch

import lane_report_reference as lref

pytestmark = pytest.mark.gpu

K, ROTATIONS, SCALES, SEED, PANEL = 3, 3, (1.0, 1.5), 2, 50


def _env_policy(slots, **env_kwargs):
    from flingbot_amd import nets, sim as fsim
    from flingbot_amd.env import BatchedFlingEnv

    ctx = fsim.FlingSim(n_envs=slots, solver=0)
    env = BatchedFlingEnv(ctx, image_dim=128, num_rotations=ROTATIONS, scale_factors=SCALES, episode_length=2,
                          record_experience=True, **env_kwargs)
    torch.manual_seed(SEED)
    policy = nets.MaximumValuePolicy(action_primitives=["fling"], num_rotations=ROTATIONS, scale_factors=list(env.scale_factors),
                                     obs_dim=64, pix_grasp_dist=8, pix_drag_dist=8, pix_place_dist=5, rgb_only=True,
                                     depth_only=False, action_expl_prob=0.0, action_expl_decay=1.0, value_expl_prob=0.0,
                                     value_expl_decay=1.0, device="cuda:0")
    return ctx, env, policy


def _same(a, b, where="stats"):
    """Equality of what run_episodes returns, through dictionaries, lists and arrays."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), (where, list(a), list(b))
        for key in a:
            _same(a[key], b[key], f"{where}[{key!r}]")
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), where
        for k, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{where}[{k}]")
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), where
    else:
        assert type(a) is type(b) and (a == b or (a != a and b != b)), (where, a, b)


@pytest.fixture(scope="module")
def runs(gpu_required, tmp_path_factory):
    from flingbot_amd import lookahead, report, sim as fsim, tasks as ftasks

    random.seed(SEED); np.random.seed(SEED)
    gen = fsim.FlingSim(n_envs=2, solver=0)
    tasks = ftasks.generate_tasks(gen, [ftasks.draw_task_parameters(min_cloth_size=24, strict_min_edge_length=24, max_cloth_size=32)
                                        for _ in range(2)])
    gen.close()
    assert all(t is not None for t in tasks)
    ctx, env, policy = _env_policy(2 * K)
    off = lookahead.run_episodes(policy, env, tasks, K, follow="best")
    ctx.close()
    root = str(tmp_path_factory.mktemp("lanes") / "report")
    ctx, env, policy = _env_policy(2 * K, action_report=True, report_root=root, report_panel=PANEL)
    composed, compose_lanes = [], report.compose_lanes

    def keeping(items, lanes, panel=200):       # what every compose_lanes call was given, as host arrays, and what it returned
        strips = compose_lanes(items, lanes, panel=panel)
        host = lambda t: None if t is None else t.cpu().numpy()   # noqa: E731
        composed.append([dict(before=host(it["before"]), afters=[host(l["after"]) for l in it["lanes"]],
                              prims=[list(l["prims"]) for l in it["lanes"]], followed=it["followed"], lanes=lanes, panel=panel,
                              strip=s) for it, s in zip(items, strips)])
        return strips

    report.compose_lanes = keeping
    try:
        on = lookahead.run_episodes(policy, env, tasks, K, follow="best")
    finally:
        report.compose_lanes = compose_lanes
        ctx.close()
    return dict(tasks=tasks, off=off, on=on, root=root, composed=composed)


def test_report_changes_nothing_the_run_returns(runs):
    off, on = runs["off"], runs["on"]
    assert list(off) == list(on) and "lane_records" in on and "lane_panels" not in on
    _same(off, on)
    executed = [len(s["candidates"]) for steps in on["lookahead"]["steps"] for s in steps]
    assert max(executed) >= 2, "a run that never executed a second lane shows nothing"


def test_one_strip_and_one_line_per_executed_step(runs):
    from PIL import Image
    from flingbot_amd import report

    on, root = runs["on"], runs["root"]
    steps = {(i, s): entry for i, entries in enumerate(on["lookahead"]["steps"]) for s, entry in enumerate(entries) if entry["candidates"]}
    assert steps
    rows = report.read_actions(root)
    assert sorted((int(r["task"][len("episode"):]), r["step"]) for r in rows) == sorted(steps) and all("lanes" in r for r in rows)
    # ONE compose_lanes call per step of the run, for all groups at once
    by_step = sorted({s for _, s in steps})
    assert [len(call) for call in runs["composed"]] == [sum(1 for _, s in steps if s == step) for step in by_step]
    pngs = sorted(os.path.relpath(os.path.join(d, f), root) for d, _, files in os.walk(root) for f in files if f.endswith(".png"))
    assert pngs == sorted(os.path.join(f"episode{i:05d}", f"step{s:02d}_lanes.png") for i, s in steps)
    flat = [float(t["flatten_area"]) for t in runs["tasks"]]
    for r in rows:
        i, s = int(r["task"][len("episode"):]), r["step"]
        entry = steps[(i, s)]
        assert r["key"] == f"episode{i:05d}_step{s:02d}_lanes" and r["png"] == os.path.join(f"episode{i:05d}", f"step{s:02d}_lanes.png")
        assert r["followed_rank"] == entry["followed_rank"] and r["max_coverage"] == flat[i]
        keep = ("rank", "primitive", "transform_index", "pixel", "value", "reward", "terminated")
        assert r["lanes"] == [{f: c[f] for f in keep} for c in entry["candidates"]]
        # the coverages: before the step (one state for all lanes), and after the FOLLOWED lane -- the trajectory's own
        assert r["preaction_coverage"] == on["records"][i]["preaction_coverage"][s]
        assert r["postaction_coverage"] == on["records"][i]["coverage"][s + 1]
        with Image.open(os.path.join(root, r["png"])) as im:
            assert im.mode == "RGB" and im.size == ((1 + K) * PANEL, PANEL)
    html = open(report.write_report(root)).read()
    assert all(html.count(f'src="{p}"') == 1 for p in pngs) and html.count("regret ") == len(rows)


def test_strips_are_the_reference_of_what_the_step_saw(runs):
    from PIL import Image
    from flingbot_amd.report import RING, SEGMENT

    on, root = runs["on"], runs["root"]
    look = on["lookahead"]["steps"]
    by_step = sorted({s for entries in look for s, entry in enumerate(entries) if entry["candidates"]})   # a call per such step
    assert len(by_step) == len(runs["composed"])
    shown = [(s, item) for s, call in zip(by_step, runs["composed"]) for item in call]
    tasks_of = [i for s in by_step for i, entries in enumerate(look) if s < len(entries) and entries[s]["candidates"]]
    assert len(shown) == len(tasks_of)
    seen_two = False
    for (s, item), i in zip(shown, tasks_of):
        entry = on["lookahead"]["steps"][i][s]
        assert item["lanes"] == K and item["panel"] == PANEL and item["followed"] == entry["followed_rank"]
        assert len(item["prims"]) == len(entry["candidates"]) and all(a is not None for a in item["afters"])
        assert item["before"].shape == (3, 128, 128)
        for prims in item["prims"]:      # a fling at thickness 3: ring, segment between the two centres, ring
            assert [p[0] for p in prims] == [RING, SEGMENT, RING] and all(p[5] == 3 for p in prims)
            assert tuple(prims[1][1:5]) == tuple(prims[0][1:3]) + tuple(prims[2][1:3])
        want = lref.strip(item["before"], item["afters"], item["prims"], item["followed"], K, PANEL)
        assert (item["strip"] == want).all()
        with Image.open(os.path.join(root, f"episode{i:05d}", f"step{s:02d}_lanes.png")) as im:
            png = np.asarray(im)
        assert (png == want).all()
        # panel 0: the stored observation with the candidates on it, sampled
        assert (png[:, :PANEL] == lref.ref.sample(lref.before_panel(item["before"], item["prims"]), PANEL)).all()
        assert (png[:, :PANEL] != lref.ref.sample(lref.ref.image_of(item["before"]), PANEL)).any()
        for j in range(len(item["prims"]), K):
            assert not png[:, (1 + j) * PANEL:(2 + j) * PANEL].any()
        seen_two = seen_two or len(item["prims"]) >= 2
    assert seen_two
