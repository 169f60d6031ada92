"""fs_value_range and fs_action_panels (csrc/fs_panels.hip) against tests/report_reference.py, byte for byte, and the action
report end to end through both drivers of the evaluation loop."""
import json
import os
import random

import numpy as np
import pytest
import torch

import report_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


# ---- fs_value_range -----------------------------------------------------------------------------------------------------------
COUNTS = (1, 63, 64, 65, 4096, 5 * 64 * 64 + 3)


def _range_cases():
    rng = np.random.default_rng(11)
    cases = []
    for n in COUNTS:
        base = rng.standard_normal(n).astype(np.float32)
        cases.append((f"random{n}", base))
        for where in (0, n - 1):            # the extreme at the first element, then at the last
            for sign in (-1.0, 1.0):
                v = base.copy()
                v[where] = np.float32(sign * 100.0)
                cases.append((f"extreme{n}@{where}{sign:+.0f}", v))
        cases.append((f"equal{n}", np.full(n, np.float32(-0.375))))
        v = base.copy()
        v[rng.integers(0, n, max(1, n // 7))] = np.float32(np.inf)
        v[rng.integers(0, n, max(1, n // 7))] = np.float32(-np.inf)
        v[rng.integers(0, n, max(1, n // 5))] = np.float32(np.nan)
        cases.append((f"mixed{n}", v))
        cases.append((f"nonfinite{n}", rng.choice(np.float32([np.nan, np.inf, -np.inf]), n)))
    cases.append(("zeros", np.float32([-0.0, 0.0, -0.0, np.nan])))
    cases.append(("finite_only_last", np.concatenate([np.full(4099, np.float32(np.nan)), np.float32([7.5])])))
    return cases


def test_value_range_matches_reference(gpu_required):
    from flingbot_amd import report

    cases = _range_cases()
    # every case at every offset from a 16-byte boundary: the kernel reads an aligned middle in float4s and the ends one by one
    tensors, want, names = [], [], []
    for name, v in cases:
        for shift in range(4):
            buf = torch.zeros(v.size + 8, dtype=torch.float32, device=DEV)
            buf[:] = float("nan") if "nonfinite" in name else 1e9      # what lies around the item must not be read as part of it
            buf[shift:shift + v.size] = torch.from_numpy(v).to(DEV)
            tensors.append(buf[shift:shift + v.size])
            want.append(ref.value_range(v))
            names.append(f"{name}+{shift}")
    assert len(tensors) > 128                                          # more than one launch's worth of items
    got = report.value_range(tensors)
    assert got.is_cuda and tuple(got.shape) == (len(tensors), 2)
    got = got.cpu().numpy()
    bad = [n for n, g, w in zip(names, got, want) if not (_bits(g) == _bits(w)).all()]
    assert not bad, bad[:8]


def test_value_range_does_not_depend_on_the_batch(gpu_required):
    from flingbot_amd import report

    rng = np.random.default_rng(12)
    item = torch.from_numpy(rng.standard_normal((96, 64, 64)).astype(np.float32)).to(DEV)
    others = [torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(DEV) for n in (5, 4096, 70000, 1)]
    alone = report.value_range([item]).cpu().numpy()[0]
    assert (_bits(alone) == _bits(ref.value_range(item.cpu().numpy()))).all()
    for place in range(5):
        batch = others[:place] + [item] + others[place:]
        got = report.value_range(batch).cpu().numpy()
        assert (_bits(got[place]) == _bits(alone)).all(), place


# ---- fs_action_panels ---------------------------------------------------------------------------------------------------------
def _items(D, S, seed):
    """Three actions that between them hold every case of the issue's list, as host arrays."""
    from flingbot_amd.report import RING, SEGMENT, action_overlays
    rng = np.random.default_rng(seed)
    at = lambda size, fy, fx: (int(fy * (size - 1)), int(fx * (size - 1)))   # noqa: E731

    def pair(size, a, b):
        return np.array([at(size, *a), at(size, *b)])

    def images():
        before = rng.uniform(-0.2, 1.2, (4, S, S)).astype(np.float32)     # four planes: only the first three are shown
        after = rng.uniform(-0.2, 1.2, (3, S, S)).astype(np.float32)
        stack = rng.uniform(-0.3, 1.3, (4, D, D)).astype(np.float32)      # below 0 and above 1: the spline's overshoot
        stack[0, 0, :3] = [np.nan, 1.0, 0.0]
        return stack, before, after

    items = []
    # 0: a fling at thickness 1 and 3; the range is the map's own, so vmin and vmax themselves are looked up
    stack, before, after = images()
    vmap = rng.standard_normal((D, D)).astype(np.float32)
    items.append(dict(stack=stack, value_map=vmap, range=np.float32([vmap.min(), vmap.max()]), before=before, after=after,
                      small=action_overlays("fling", pair(D, (0.3, 0.5), (0.8, 0.45)), 1),
                      large=action_overlays("fling", pair(S, (0.3, 0.5), (0.8, 0.45)), 3)))
    # 1: stretchdrag plus a ring on the corner and a segment from outside the image; a flat range; no after-image
    stack, before, _ = images()
    corner_far = (S - 1, S - 1)
    items.append(dict(stack=stack, value_map=rng.standard_normal((D, D)).astype(np.float32), range=np.float32([0.25, 0.25]),
                      before=before, after=None,
                      small=action_overlays("stretchdrag", pair(D, (0.5, 0.2), (0.6, 0.8)), 1)
                      + [(RING, 0, 0, 2, 0, 1, 10, 20, 30), (SEGMENT, -5, -3, D // 2, D + 4, 1, 200, 100, 50)],
                      large=[(RING, 0, 0, 6, 0, 3, 10, 20, 30), (RING, *corner_far, 6, 0, 3, 0, 0, 255),
                             (SEGMENT, -40, S // 3, S // 2, S + 25, 3, 200, 100, 50),
                             (SEGMENT, S // 4, S // 4, S // 4, S // 4, 3, 255, 255, 255),            # zero length
                             (SEGMENT, 2, 2, S - 3, S - 3, 3, 255, 0, 0), (SEGMENT, 2, S - 3, S - 3, 2, 3, 0, 255, 0),   # a cross
                             (RING, S // 2, S // 2, 9, 0, 2, 0, 0, 0),                              # over the crossing
                             (SEGMENT, S // 2, 0, S // 2, S - 1, 1, 1, 2, 3)]))
    # 2: drag and place; a range narrower than the values (indices clamp at both ends), non-finite values in the map
    stack, before, after = images()
    vmap = rng.standard_normal((D, D)).astype(np.float32)
    vmap[0, 0], vmap[1, 1], vmap[2, 2], vmap[3, 3] = np.nan, np.inf, -np.inf, 0.5
    vmap[4, 4], vmap[5, 5] = -0.5, np.float32(0.5) - np.float32(2 ** -20)
    items.append(dict(stack=stack, value_map=vmap, range=np.float32([-0.5, 0.5]), before=before, after=after,
                      small=action_overlays("drag", pair(D, (0.2, 0.2), (0.7, 0.9)), 1)
                      + action_overlays("place", pair(D, (0.9, 0.9), (0.9, 0.9)), 1),              # a zero-length arrow
                      large=action_overlays("place", pair(S, (0.2, 0.2), (0.7, 0.9)), 3)
                      + action_overlays("drag", pair(S, (0.7, 0.9), (0.1, 0.6)), 3)))
    return items


def _to_device(item):
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    return dict(item, **{k: up(item[k]) for k in ("stack", "value_map", "range", "before", "after")})


@pytest.fixture(scope="module")
def jet_table():
    from flingbot_amd import report
    return report.jet_table()


@pytest.mark.parametrize("panel", [40, 64, 96, 200])
@pytest.mark.parametrize("S", [50, 400])
@pytest.mark.parametrize("D", [8, 64])
def test_action_panels_match_reference(gpu_required, jet_table, D, S, panel):
    from flingbot_amd import report

    host = _items(D, S, seed=1000 * D + S)
    dev = [_to_device(it) for it in host]
    got = report.compose(dev, panel=panel)
    assert got.dtype == np.uint8 and got.shape == (3, panel, 5 * panel, 3)
    for k, it in enumerate(host):
        want = ref.strip(jet_table, it["stack"], it["value_map"], it["range"], it["before"], it["after"], it["small"],
                         it["large"], panel)
        diff = np.argwhere(got[k] != want)
        assert diff.size == 0, (k, len(diff), diff[:4], got[k][tuple(diff[0])], want[tuple(diff[0])])
        # batch invariance: the item composed alone (at an odd panel every other strip starts off the dword grid)
        assert (report.compose([dev[k]], panel=panel)[0] == got[k]).all(), k
    assert not got[1][:, 4 * panel:].any()                              # the null after-pointer: black
    assert (got[1][:, panel:2 * panel] == jet_table[0]).all()           # vmax == vmin: entry 0 everywhere


def test_action_panels_odd_panel_and_overlays_show(gpu_required, jet_table):
    """An odd panel (byte stores for every other strip) and a sanity check that the overlay is really there: the kernel and
    the reference could agree on drawing nothing."""
    from flingbot_amd import report

    host = _items(64, 50, seed=5)
    got = report.compose([_to_device(it) for it in host], panel=37)
    for k, it in enumerate(host):
        want = ref.strip(jet_table, it["stack"], it["value_map"], it["range"], it["before"], it["after"], it["small"],
                         it["large"], 37)
        assert (got[k] == want).all(), k
    big = report.compose([_to_device(host[0])], panel=400)[0]           # panel > both sources
    assert (big == ref.strip(jet_table, *(host[0][n] for n in ("stack", "value_map", "range", "before", "after", "small",
                                                               "large")), 400)).all()
    plain = report.compose([_to_device(dict(host[0], small=[], large=[]))], panel=400)[0]
    changed = (big != plain).any(axis=2)
    assert changed[:, 800:1200].sum() > 50 and changed[:, 1200:1600].sum() > 200
    assert not changed[:, :800].any() and not changed[:, 1600:].any()
    assert (big[:, :400] == plain[:, 1200:1600]).all()                  # panel 0 is panel 3 without the action


# ---- end to end ---------------------------------------------------------------------------------------------------------------
PANEL = 48


@pytest.fixture(scope="module")
def small_run(gpu_required):
    """Two small tasks, a fixed-weight policy, and the evaluation loop without reporting."""
    from flingbot_amd import evaluate, nets, sim as fsim, tasks as ftasks
    from flingbot_amd.env import BatchedFlingEnv

    random.seed(1); np.random.seed(1); torch.manual_seed(1)
    n = 2
    gen = fsim.FlingSim(n_envs=n, solver=0)
    tasks = ftasks.generate_tasks(gen, [ftasks.draw_task_parameters(min_cloth_size=24, strict_min_edge_length=24, max_cloth_size=32)
                                        for _ in range(n)])
    gen.close()
    ctx = fsim.FlingSim(n_envs=n, solver=0)
    env = BatchedFlingEnv(ctx, image_dim=128, episode_length=2)
    torch.manual_seed(1)
    policy = nets.MaximumValuePolicy(action_primitives=["fling"], num_rotations=12, scale_factors=list(env.scale_factors),
                                     obs_dim=64, pix_grasp_dist=8, pix_drag_dist=8, pix_place_dist=5, rgb_only=True,
                                     depth_only=False, action_expl_prob=0.0, action_expl_decay=1.0, value_expl_prob=0.0,
                                     value_expl_decay=1.0, device=DEV)
    calls = _count_calls(env)
    plain = evaluate.run_tasks(policy, env, tasks, max_steps=2)
    ctx.close()
    assert calls == dict(look=0, panels=0, items=[])                   # reporting off: neither service is ever requested
    assert sum(a is not None for r in plain["records"] for a in r["actions"]) >= 2
    return dict(tasks=tasks, policy=policy, plain=plain)


def _count_calls(env):
    """Count what the "look" and "panels" services reach, and keep the inputs of every composed action as host arrays."""
    calls = dict(look=0, panels=0, items=[])
    look, compose = env.look_batch, env.compose_reports

    def look_batch(envs):
        calls["look"] += 1
        return look(envs)

    def compose_reports(held):
        calls["panels"] += 1
        strips = compose(held)
        for item, strip in zip(held, strips):
            host = {k: None if item[k] is None else item[k].cpu().numpy() for k in ("stack", "value_map", "range", "before", "after")}
            calls["items"].append(dict(item, **host, strip=strip))
        return strips

    env.look_batch, env.compose_reports = look_batch, compose_reports
    return calls


def _reporting_env(root=None, **kwargs):
    from flingbot_amd import sim as fsim
    from flingbot_amd.env import BatchedFlingEnv

    ctx = fsim.FlingSim(n_envs=2, solver=0)
    return ctx, BatchedFlingEnv(ctx, image_dim=128, episode_length=2, action_report=True, report_panel=PANEL, report_root=root,
                                **kwargs)


def test_report_leaves_the_run_as_it_was_and_both_drivers_agree(small_run, jet_table):
    from flingbot_amd import evaluate

    tasks, policy, plain = small_run["tasks"], small_run["policy"], small_run["plain"]
    ctx, env = _reporting_env()
    calls = _count_calls(env)
    stats = evaluate.run_tasks(policy, env, tasks, max_steps=2)
    ctx.close()
    assert stats["simulation_steps"] == plain["simulation_steps"]
    for a, b in zip(stats["records"], plain["records"]):
        assert a["coverage"] == b["coverage"] and a["actions"] == b["actions"]
    assert (stats["coverage_steps"] == plain["coverage_steps"]).all()
    chosen = sum(a is not None for r in stats["records"] for a in r["actions"])
    assert calls["panels"] >= 1 and calls["look"] >= 1 and len(calls["items"]) == chosen
    for rec in stats["records"]:        # one entry per action, None where no action was chosen
        assert len(rec["panels"]) == len(rec["actions"])
        for strip, action in zip(rec["panels"], rec["actions"]):
            assert (strip is None) == (action is None)
            assert strip is None or (strip.shape == (PANEL, 5 * PANEL, 3) and strip.dtype == np.uint8)
    # a stored action's inputs through the reference give the stored strip; the action is on it
    for item in calls["items"]:
        want = ref.strip(jet_table, item["stack"], item["value_map"], item["range"], item["before"], item["after"],
                         item["small"], item["large"], PANEL)
        assert (item["strip"] == want).all()
        assert item["after"] is not None and item["range"][0] <= item["value_map"].min() <= item["value_map"].max() <= item["range"][1]
        assert len(item["small"]) == 3 and len(item["large"]) == 3 and item["large"][0][5] == 3 and item["small"][0][5] == 1
        bare = ref.strip(jet_table, item["stack"], item["value_map"], item["range"], item["before"], item["after"], [], [], PANEL)
        assert (bare != want).any(axis=2)[:, 2 * PANEL:4 * PANEL].sum() > 4
    # the lock-step driver draws the same strips (task i runs in episode i there)
    ctx, env = _reporting_env(scheduled=False)
    lock = evaluate.run_episodes(policy, env, tasks, max_steps=2)
    ctx.close()
    for i, rec in enumerate(stats["records"]):
        assert lock["records"][i]["actions"] == rec["actions"]
        assert len(env.panels[i]) == len(rec["panels"])
        for a, b in zip(env.panels[i], rec["panels"]):
            assert (a is None and b is None) or (a == b).all()


def test_report_directory(small_run, tmp_path):
    from flingbot_amd import evaluate, report

    tasks, policy, plain = small_run["tasks"], small_run["policy"], small_run["plain"]
    root = str(tmp_path / "report")
    ctx, env = _reporting_env(root=root, report=[1])
    stats = evaluate.run_tasks(policy, env, tasks, max_steps=2)
    ctx.close()
    assert [r["actions"] for r in stats["records"]] == [r["actions"] for r in plain["records"]]
    assert all("panels" not in r for r in stats["records"])
    chosen = sum(a is not None for a in stats["records"][1]["actions"])          # task 1 only
    rows = report.read_actions(root)
    pngs = [os.path.join(d, f) for d, _, fs in os.walk(root) for f in fs if f.endswith(".png")]
    assert len(pngs) == len(rows) == chosen >= 1
    name = evaluate.film_name(tasks, 1)
    rec = stats["records"][1]
    for r in rows:
        k = r["step"]
        assert r["key"] == f"{name}_step{k:02d}" and r["task"] == name and r["primitive"] == rec["actions"][k] == "fling"
        assert r["preaction_coverage"] == rec["preaction_coverage"][k] and r["postaction_coverage"] == rec["coverage"][k + 1]
        assert r["max_coverage"] == float(tasks[1]["flatten_area"]) and len(r["max_indices"]) == 3 and r["film_dir"] is None
        assert r["png"] == os.path.join(name, f"step{k:02d}.png") and os.path.exists(os.path.join(root, r["png"]))
    path = report.write_report(root)
    html = open(path).read()
    assert os.path.basename(path) == "index.html" and all(html.count(r["png"]) == 1 for r in rows)
    with open(os.path.join(root, report.ACTIONS_FILE)) as f:
        assert len([json.loads(line) for line in f]) == chosen


def test_film_and_report_together_with_relative_directories(small_run, tmp_path, monkeypatch):
    """`--dump-visualizations films --report report`, both relative to the working directory, in both drivers: the line of
    actions.jsonl names the film's directory in full, and the page's link leads from report/ to a film that exists."""
    import re
    from flingbot_amd import evaluate, report, sim as fsim
    from flingbot_amd.env import BatchedFlingEnv

    tasks, policy = small_run["tasks"][:1], small_run["policy"]
    for scheduled in (True, False):
        work = tmp_path / ("scheduled" if scheduled else "lockstep")
        work.mkdir()
        monkeypatch.chdir(work)
        ctx = fsim.FlingSim(n_envs=1, solver=0)
        env = BatchedFlingEnv(ctx, image_dim=128, episode_length=1, scheduled=scheduled, action_report=True, report_panel=PANEL,
                              report_root="report", dump_visualizations=True, visualize=[0], frame_size=(48, 48),
                              visualization_root="films")
        stats = (evaluate.run_tasks if scheduled else evaluate.run_episodes)(policy, env, tasks, max_steps=1)
        ctx.close()
        assert stats["records"][0]["actions"] == ["fling"]
        rows = report.read_actions("report")
        assert len(rows) == 1 and os.path.isabs(rows[0]["film_dir"])
        assert os.path.exists(os.path.join(rows[0]["film_dir"], "top.png")) and rows[0]["film_dir"].startswith(str(work / "films"))
        page = report.write_report("report")
        links = re.findall(r'href="([^"]+)"', open(page).read())
        assert len(links) == 1 and links[0].startswith(".." + os.sep + "films")
        assert os.path.exists(os.path.normpath(os.path.join(str(work / "report"), links[0])))
