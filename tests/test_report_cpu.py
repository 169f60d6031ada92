"""The host side of the action report (flingbot_amd/report.py) and the argument checks of its two entry points
(include/flingsim.h: fs_value_range, fs_action_panels) -- everything that needs no GPU."""
import ctypes as C
import io
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS_ERR_ARG = -1   # include/flingsim.h
ENTRIES = ("fs_value_range", "fs_action_panels", "fs_action_panels_work_bytes", "fs_jet_table")


def test_entries_declared_and_exported():
    from flingbot_amd import build, sim as fsim

    lib = fsim.load_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flingsim.h")).read(), flags=re.S)
    raw = C.CDLL(build.LIB)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} is not declared in flingsim.h"
        assert hasattr(raw, name) and name in lib._fs_symbols
    assert "fs_panels.hip" in build.LIB_SOURCES
    assert lib.fs_action_panels_work_bytes(3) == 3 * 624 and lib.fs_action_panels_work_bytes(0) == 0


# ---- refusals: FS_ERR_ARG and a message, before any HIP call (there is no device here) --------------------------------
FAKE = 4096   # stands for a device address: a refused call never looks behind it


def _record(n_small=1, n_large=1, prim=(1, 2, 3, 4, 5, 1, 255, 0, 0)):
    from flingbot_amd import report
    table = np.zeros(1, report.PANEL_RECORD)
    for name in ("stack", "value_map", "range", "before", "after"):
        table[name] = FAKE
    table["n_small"], table["n_large"] = n_small, n_large
    table["small"][0, :min(n_small, 8)] = prim
    table["large"][0, :min(n_large, 8)] = prim
    return table


def _panels(lib, table, B=1, D=64, S=400, panel=200, out=FAKE, work=FAKE):
    return lib.fs_action_panels(None if table is None else table.ctypes.data, B, D, S, panel, out, work, None)


def _refused(lib, rc, *words):
    assert rc == FS_ERR_ARG
    msg = lib.fs_last_error().decode()
    assert msg and all(w in msg for w in words), msg


def test_action_panels_refusals():
    from flingbot_amd import sim as fsim

    lib = fsim.load_library()
    good = _record()
    _refused(lib, _panels(lib, None), "null")
    _refused(lib, _panels(lib, good, out=None), "null")
    _refused(lib, _panels(lib, good, work=None), "null")
    for field in ("stack", "value_map", "range", "before"):
        bad = _record()
        bad[field] = 0
        _refused(lib, _panels(lib, bad), "null", "action 0")
    _refused(lib, _panels(lib, good, B=0), "actions")
    _refused(lib, _panels(lib, good, B=-3), "actions")
    for kw in (dict(panel=0), dict(panel=4097), dict(S=0), dict(S=4097), dict(D=0), dict(D=4097)):
        _refused(lib, _panels(lib, good, **kw), "4096")
    _refused(lib, _panels(lib, _record(n_small=9)), "9 primitives")
    _refused(lib, _panels(lib, _record(n_large=9)), "9 primitives")
    _refused(lib, _panels(lib, _record(n_large=-1)), "primitives")
    for slot in (1, 2, 3, 4):
        for value in (8192, -8192):
            prim = [1, 2, 3, 4, 5, 1, 255, 0, 0]
            prim[slot] = value
            _refused(lib, _panels(lib, _record(prim=tuple(prim))), "8191")
    _refused(lib, _panels(lib, _record(prim=(1, 2, 3, 4, 5, 0, 255, 0, 0))), "thickness")
    _refused(lib, _panels(lib, _record(prim=(0, 2, 3, 4, 5, 65, 255, 0, 0))), "thickness")
    _refused(lib, _panels(lib, _record(prim=(2, 2, 3, 4, 5, 1, 255, 0, 0))), "kind")
    _refused(lib, _panels(lib, _record(prim=(1, 2, 3, 4, 5, 1, 256, 0, 0))), "colour")
    # the limits themselves pass: records are checked in order, so a table whose FIRST record sits on every limit (8 + 8
    # primitives, +-8191, thickness 64, colour 255, D = S = panel = 4096) and whose second one is bad is refused for the second
    edge = _record(n_small=8, n_large=8, prim=(1, 8191, -8191, 8191, -8191, 64, 255, 255, 255))
    for field, value, words in (("n_large", 9, ("action 1", "9 primitives")), ("stack", 0, ("action 1", "null"))):
        two = np.concatenate([edge, _record()])
        two[field][1] = value
        _refused(lib, _panels(lib, two, B=2, D=4096, S=4096, panel=4096), *words)
    two = np.concatenate([edge, edge])
    two["small"][1, 7, 5] = 65
    _refused(lib, _panels(lib, two, B=2), "action 1", "primitive 7", "thickness")
    ring = _record(n_small=8, n_large=8, prim=(0, -8191, 8191, 8191, 0, 1, 0, 0, 0))
    two = np.concatenate([ring, _record(prim=(0, 0, 0, 8192, 0, 1, 0, 0, 0))])
    _refused(lib, _panels(lib, two, B=2), "action 1", "8191")


def test_value_range_refusals():
    from flingbot_amd import report, sim as fsim

    lib = fsim.load_library()
    items = np.zeros(2, report.RANGE_ITEM)
    items["values"], items["count"] = FAKE, 5
    call = lambda t, n, out=FAKE: lib.fs_value_range(None if t is None else t.ctypes.data, n, out, None)   # noqa: E731
    _refused(lib, call(None, 2), "null")
    _refused(lib, call(items, 2, out=None), "null")
    _refused(lib, call(items, 0), "fewer than one")
    bad = items.copy()
    bad["values"][1] = 0
    _refused(lib, call(bad, 2), "item 1")
    bad = items.copy()
    bad["count"][0] = 0
    _refused(lib, call(bad, 2), "item 0")


# ---- the colour table -------------------------------------------------------------------------------------------------------
def test_jet_table_is_the_closed_form():
    from flingbot_amd import report

    table = report.jet_table()
    assert table.shape == (256, 3) and table.dtype == np.uint8
    assert (table == report.jet_closed_form()).all()
    # the closed form, written out once more: np.interp over the breakpoints in the issue's words
    x = np.linspace(0, 1, 256)
    red = np.interp(x, [0, 0.35, 0.66, 0.89, 1], [0, 0, 1, 1, 0.5])
    green = np.interp(x, [0, 0.125, 0.375, 0.64, 0.91, 1], [0, 0, 1, 1, 0, 0])
    blue = np.interp(x, [0, 0.11, 0.34, 0.65, 1], [0.5, 1, 1, 0, 0])
    assert (table == np.trunc(np.stack([red, green, blue], 1) * 255).astype(np.uint8)).all()
    assert tuple(table[0]) == (0, 0, 127) and tuple(table[255]) == (127, 0, 0)


def test_jet_table_is_matplotlibs():
    matplotlib = pytest.importorskip("matplotlib")
    from flingbot_amd import report

    jet = matplotlib.colormaps["jet"]
    table = report.jet_table()
    assert (table == jet(np.arange(256), bytes=True)[:, :3]).all()
    # the index rule: what jet(v, bytes=True) picks for v in [0, 1]
    import report_reference as ref
    v = np.concatenate([np.random.default_rng(0).random(4000, dtype=np.float32), np.float32([0, 1, 0.5, 255 / 256, 1 / 256])])
    got = ref.jet(table, v.reshape(1, -1), 0.0, 1.0)[0]
    assert (got == jet(v, bytes=True)[:, :3]).all()


# ---- draw_action as primitives ------------------------------------------------------------------------------------------------
GREEN, YELLOW, RED, MAGENTA, CYAN = (0, 255, 0), (255, 255, 0), (255, 0, 0), (255, 0, 255), (0, 255, 255)


def test_overlays_fling():
    from flingbot_amd.report import RING, SEGMENT, action_overlays

    pix = np.array([[10, 20], [30, 40]])
    assert action_overlays("fling", pix, 1) == [(RING, 10, 20, 2, 0, 1) + GREEN, (SEGMENT, 10, 20, 30, 40, 1) + YELLOW,
                                                (RING, 30, 40, 2, 0, 1) + RED]
    assert action_overlays("fling", pix, 3) == [(RING, 10, 20, 6, 0, 3) + GREEN, (SEGMENT, 10, 20, 30, 40, 3) + YELLOW,
                                                (RING, 30, 40, 6, 0, 3) + RED]


def test_overlays_stretchdrag_direction():
    from flingbot_amd.report import RING, SEGMENT, action_overlays

    # a horizontal pair (same row): left - right = (0, -20), cross((0, -20, 0), (0, 0, 1))[:2] = (-20, 0): towards row 0
    got = action_overlays("stretchdrag", np.array([[20, 10], [20, 30]]), 1)
    assert got[:3] == [(RING, 20, 10, 2, 0, 1) + MAGENTA, (SEGMENT, 20, 10, 20, 30, 1) + YELLOW, (RING, 20, 30, 2, 0, 1) + CYAN]
    assert len(got) == 6 and got[3] == (SEGMENT, 20, 20, 0, 20, 1) + RED
    assert all(p[0] == SEGMENT and p[1:3] == (0, 20) and p[6:] == RED for p in got[4:])
    # a vertical pair (same column): left - right = (-20, 0), the cross product's first two entries are (0, 20)
    got = action_overlays("stretchdrag", np.array([[10, 20], [30, 20]]), 3)
    assert got[3] == (SEGMENT, 20, 20, 20, 40, 3) + RED
    # the midpoint is truncated to integers: ((11 + 20) / 2, (10 + 31) / 2) = (15.5, 20.5) -> (15, 20)
    got = action_overlays("stretchdrag", np.array([[11, 10], [20, 31]]), 1)
    assert got[3][1:3] == (15, 20) and got[3][3:5] == (15 - 21, 20 + 9)


def test_overlays_arrows():
    from flingbot_amd.report import SEGMENT, action_overlays

    # axis-aligned, along a row: length 100, tips of 10 at 45 degrees: 10 / sqrt(2) = 7.07 -> 7 rows, 92.93 -> column 93
    got = action_overlays("drag", np.array([[0, 0], [0, 100]]), 1)
    assert got == [(SEGMENT, 0, 0, 0, 100, 1) + MAGENTA, (SEGMENT, 0, 100, -7, 93, 1) + MAGENTA,
                   (SEGMENT, 0, 100, 7, 93, 1) + MAGENTA]
    # 3-4-5: (0, 0) -> (30, 40), length 50, tips of 5.  Back along the shaft: (-0.6, -0.8); turned by +-45 degrees:
    # (-0.98995, -0.14142) and (0.14142, -0.98995); times 5, from (30, 40): (25.05, 39.29) and (30.71, 35.05)
    got = action_overlays("place", np.array([[0, 0], [30, 40]]), 3)
    assert got == [(SEGMENT, 0, 0, 30, 40, 3) + CYAN, (SEGMENT, 30, 40, 25, 39, 3) + CYAN, (SEGMENT, 30, 40, 31, 35, 3) + CYAN]
    # zero length: three degenerate segments, no error
    got = action_overlays("drag", np.array([[5, 6], [5, 6]]), 1)
    assert got == [(SEGMENT, 5, 6, 5, 6, 1) + MAGENTA] * 3
    with pytest.raises(NotImplementedError):
        action_overlays("fold", np.zeros((2, 2), int), 1)


def test_reference_rules_on_hand_cases():
    """report_reference itself, on cases small enough to check by hand (the GPU test trusts it)."""
    import report_reference as ref

    # ring, radius 2, thickness 1 at (4, 4): 9 <= 4 d2 <= 25, so d2 in {3, 4, 5, 6}: the 4 axis points and the 8 knight moves
    m = ref.mask_of((0, 4, 4, 2, 0, 1), 9)
    yy, xx = np.nonzero(m)
    d2 = (yy - 4) ** 2 + (xx - 4) ** 2
    assert sorted(set(d2)) == [4, 5] and m.sum() == 12
    # a horizontal segment of thickness 1: exactly its own pixels; of thickness 3: one pixel more to every side
    m = ref.mask_of((1, 2, 1, 2, 5, 1), 8)
    assert m.sum() == 5 and m[2, 1:6].all()
    m = ref.mask_of((1, 2, 1, 2, 5, 3), 8)
    assert m[1:4, 0:7].all() and m.sum() == 21    # (the round caps reach the diagonal neighbours: 4 * 2 <= 9)
    # a zero-length segment of thickness 1 is one pixel; off the image it covers nothing
    assert ref.mask_of((1, 3, 3, 3, 3, 1), 8).sum() == 1 and ref.mask_of((1, -3, 3, -3, 3, 1), 8).sum() == 0
    # blending: the later primitive's colour, once
    img = np.full((8, 8, 3), 100, np.uint8)
    out = ref.draw(img, [(1, 2, 0, 2, 7, 1, 255, 0, 0), (1, 0, 3, 7, 3, 1, 0, 255, 0)])
    assert tuple(out[2, 3]) == (10, 240, 10) and tuple(out[2, 4]) == (240, 10, 10) and tuple(out[0, 0]) == (100, 100, 100)
    # sampling: (dst * size) // panel
    src = np.arange(25).reshape(5, 5)
    assert (ref.sample(src, 3) == src[[0, 1, 3]][:, [0, 1, 3]]).all() and ref.sample(src, 8).shape == (8, 8)
    # the colour index at the ends of the range and for a flat map
    table = np.arange(768).reshape(256, 3) % 251
    v = np.float32([[0.0, 1.0, 0.5, np.nan, np.inf, -1.0, 2.0]])
    assert (ref.jet(table, v, 0.0, 1.0) == table[[0, 255, 128, 0, 0, 0, 255]]).all()
    assert (ref.jet(table, v, 0.5, 0.5) == table[[0] * 7]).all()
    assert (ref.value_range([np.nan, -np.inf, 3.0, -0.0, np.inf]) == [0.0, 3.0]).all()
    assert (ref.value_range([np.nan, np.inf]) == [0.0, 0.0]).all()


# ---- files ------------------------------------------------------------------------------------------------------------------
def test_write_png_round_trip(tmp_path):
    from PIL import Image
    from flingbot_amd.report import write_png

    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (7, 13, 3), dtype=np.uint8)
    path = write_png(str(tmp_path / "odd.png"), rgb)
    with Image.open(path) as im:
        assert im.mode == "RGB" and im.size == (13, 7) and getattr(im, "n_frames", 1) == 1
        assert (np.asarray(im) == rgb).all()
    grey = rng.integers(0, 256, (5, 3), dtype=np.uint8)
    with Image.open(write_png(str(tmp_path / "grey.png"), grey)) as im:
        assert im.mode == "L" and (np.asarray(im) == grey).all()
    with pytest.raises(ValueError):
        write_png(str(tmp_path / "bad.png"), rgb.astype(np.float32))


def test_write_report_names_every_png_once_in_key_order(tmp_path):
    from flingbot_amd import report

    root = str(tmp_path / "report")
    log = report.ActionLog(root)
    strip = np.zeros((4, 20, 3), np.uint8)
    # written out of order, two episodes, one with a film
    for name, step, film in (("taskB", 1, None), ("taskA", 0, os.path.join(root, "..", "films", "taskA")), ("taskB", 0, None),
                             ("taskA", 1, os.path.join(root, "..", "films", "taskA"))):
        meta = dict(key=f"{name}_step{step:02d}", task=name, step=step, primitive="fling", rotation=-90.0, scale=1.5,
                    max_indices=[3, 20, 30], preaction_coverage=0.5, postaction_coverage=0.75, max_coverage=1.0, film_dir=film)
        png = log.write(name, meta, strip)
        assert os.path.exists(png)
    rows = [json.loads(line) for line in open(os.path.join(root, report.ACTIONS_FILE))]
    assert len(rows) == 4 and all(set(r) >= {"key", "task", "step", "primitive", "rotation", "scale", "max_indices",
                                             "preaction_coverage", "postaction_coverage", "max_coverage", "png", "film_dir"}
                                  for r in rows)
    path = report.write_report(root)
    assert path == os.path.join(root, "index.html")
    html = open(path).read()
    want = ["taskA/step00.png", "taskA/step01.png", "taskB/step00.png", "taskB/step01.png"]
    assert [html.count(p) for p in want] == [1, 1, 1, 1]
    at = [html.index(p) for p in want]
    assert at == sorted(at)
    assert html.count("<tr>") == 5 and html.count("top.png") == 2 and "50.0 %" in html and "75.0 %" in html
    # the film's link leads from the report directory to the film, wherever the two lie
    films = [m for m in re.findall(r'href="([^"]+)"', html)]
    assert films == [os.path.join("..", "films", "taskA", "top.png")] * 2
    assert all(os.path.normpath(os.path.join(root, f)) == str(tmp_path / "films" / "taskA" / "top.png") for f in films)
    # the command-line tool rewrites the page from the list
    os.remove(path)
    from flingbot_amd import visualize
    visualize.main([root])
    assert open(path).read() == html


def test_film_link_with_relative_directories(tmp_path, monkeypatch):
    """The README's own form: `--dump-visualizations films --report report`, both relative to the working directory.  The
    page lies IN report/, so the link must climb out of it; and it must still be right when the page is rewritten from
    another working directory."""
    from flingbot_amd import report, visualize

    monkeypatch.chdir(tmp_path)
    log = report.ActionLog("report")
    for step in (0, 1):
        meta = dict(key=f"t_step{step:02d}", task="t", step=step, primitive="fling", rotation=0.0, scale=1.0, max_indices=[0, 9, 9],
                    preaction_coverage=0.5, postaction_coverage=0.75, max_coverage=1.0, film_dir=os.path.join("films", "t"))
        log.write("t", meta, np.zeros((4, 20, 3), np.uint8))
    os.makedirs(os.path.join("films", "t"))
    open(os.path.join("films", "t", "top.png"), "wb").close()
    rows = report.read_actions("report")
    assert all(os.path.isabs(r["film_dir"]) and r["film_dir"] == str(tmp_path / "films" / "t") for r in rows)
    assert all(r["png"] == os.path.join("t", f"step{r['step']:02d}.png") for r in rows)

    def targets(page):
        html = open(page).read()
        links = re.findall(r'href="([^"]+)"', html) + re.findall(r'src="([^"]+)"', html)
        assert len(links) == 4
        return [os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(page)), l)) for l in links]

    for t in targets(report.write_report("report")):
        assert os.path.exists(t), t
    first = open(os.path.join("report", "index.html")).read()
    assert 'href="../films/t/top.png"' in first
    elsewhere = tmp_path / "elsewhere"
    elsewhere.mkdir()
    monkeypatch.chdir(elsewhere)
    visualize.main([str(tmp_path / "report")])
    assert open(str(tmp_path / "report" / "index.html")).read() == first


def test_summarize_prints_collect_stats(tmp_path):
    from flingbot_amd import report, taskio

    task = {"cloth_mass": 0.5, "flatten_area": 2.0, "task_difficulty": "hard", "initial_coverage": 0.5}
    easy = dict(task, task_difficulty="easy")
    recs = [dict(coverage=[1.0, 1.25, 1.5, 1.5], actions=["fling", "drag", None], rewards=[0.25, 0.25, 0.0],
                 preaction_coverage=[1.0, 1.25, 1.5]),
            dict(coverage=[0.5, 0.75], actions=["fling"], rewards=[0.25], preaction_coverage=[0.5]),
            dict(coverage=[0.5, 1.0, 1.5], actions=["fling", "fling"], rewards=[0.5, 0.5], preaction_coverage=[0.5, 1.0])]
    path = str(tmp_path / "replay.npz")
    taskio.save_replay(path, recs, [task, task, easy])
    out = io.StringIO()
    report.summarize([path], file=out)
    text = out.getvalue()
    stats = taskio.collect_stats(path, num_points=int(1e7))
    # every statistic that is one number, and no other: written out by hand for this file
    want = {"delta_coverage/easy/mean": "0.2500", "delta_coverage/easy/percent_positive": "1.0000",
            "delta_coverage/hard/mean": "0.0938", "delta_coverage/hard/percent_zero": "0.2500",
            "final_coverage/hard/mean": "0.5625", "init_coverage/hard/mean": "0.2500", "best_coverage/easy/mean": "0.7500",
            "episode_delta_coverage/easy/mean": "0.5000", "episode_length/hard/mean": "1.0000",
            "episode_length/easy/mean": "1.0000", "action_primitive/percent_fling": "0.6667",
            "action_primitive/percent_drag": "0.1667", "action_primitive/percent_place": "0.0000"}
    rows = dict(re.findall(r"^\t\[(\S+) *\]:\t(\S+)$", text, flags=re.M))
    for key, value in want.items():
        assert rows.get(key) == value, (key, rows.get(key))
        assert "\t[" + key + " " * (36 - len(key)) + "]:\t" + value + "\n" in text
    assert set(rows) == {k for k in stats if np.ndim(stats[k]) == 0 and not k.endswith(("/min", "/max"))} and len(rows) == 21
    # the episode lengths: the easy figures with four decimals, the hard ones with two (visualize.py:25-43); the stored
    # lengths are the last step's index: hard episodes 2 and 0, the easy one 1
    tail = text[text.index("Easy Episode Lengths:"):].splitlines()
    assert tail == ["Easy Episode Lengths:", "\tmean: 1.0000", "\t25-quantile: 1.0000", "\tmedian: 1.0000", "\t75-quantile: 1.0000",
                    "Hard Episode Lengths:", "\tmean: 1.00", "\t25-quantile: 0.50", "\tmedian: 1.00", "\t75-quantile: 1.50"]
    # a run without easy tasks still prints the easy header (visualize.py:22), and nothing under it
    hard_only = str(tmp_path / "hard.npz")
    taskio.save_replay(hard_only, recs[:2], [task, task])
    out = io.StringIO()
    report.summarize(hard_only, file=out)
    tail = out.getvalue()[out.getvalue().index("Easy Episode Lengths:"):].splitlines()
    assert tail[:2] == ["Easy Episode Lengths:", "Hard Episode Lengths:"] and len(tail) == 6


def test_evaluate_report_options():
    from flingbot_amd import evaluate

    ap = evaluate.build_parser()
    a = ap.parse_args(["--tasks", "t.npz"])
    assert evaluate.report_env_kwargs(a) == {}
    a = ap.parse_args(["--tasks", "t.npz", "--report", "out", "--report-panel", "96", "--report-tasks", "0", "3", "7"])
    assert evaluate.report_env_kwargs(a) == dict(action_report=True, report_root="out", report_panel=96, report=[0, 3, 7])
    a = ap.parse_args(["--tasks", "t.npz", "--report", "out"])
    assert evaluate.report_env_kwargs(a) == dict(action_report=True, report_root="out", report_panel=200, report=None)
