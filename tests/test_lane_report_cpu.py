"""The lane report's host side (flingbot_amd/report.py, include/flingsim.h fs_lane_panels): the reference's frame and overwrite
rules on cases small enough to check by hand, the argument checks of the entry point, and index.html -- no GPU needed."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS_ERR_ARG = -1
FAKE = 4096   # stands for a device address: a refused call never looks behind it


def test_entries_declared_exported_and_mirrored():
    from flingbot_amd import build, report, sim as fsim
    import lane_report_reference as lref

    lib = fsim.load_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flingsim.h")).read(), flags=re.S)
    raw = C.CDLL(build.LIB)
    for name in ("fs_lane_panels", "fs_lane_panels_work_bytes", "fs_lane_colours"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} is not declared in flingsim.h"
        assert hasattr(raw, name) and name in lib._fs_symbols
    assert re.search(r"#define FS_LANE_MAX 8\b", hdr)
    assert report.LANE_RECORD.itemsize == 2416
    assert lib.fs_lane_panels_work_bytes(3) == 3 * 2416 and lib.fs_lane_panels_work_bytes(0) == 0
    # the compiled-in rank colours are the ones the header states (the reference copies them from there)
    assert (report.lane_colours() == lref.RANK_COLOURS).all()
    assert len({tuple(c) for c in lref.RANK_COLOURS}) == 8 and not (lref.RANK_COLOURS == 255).all(axis=1).any()


# ---- the frame rule -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("panel", [1, 2, 49, 50, 101])
def test_frame_rule(panel):
    import lane_report_reference as lref

    t = {1: 1, 2: 1, 49: 1, 50: 1, 101: 2}[panel]          # max(1, panel / 50), written out
    assert lref.frame_width(panel) == t
    base = np.full((panel, panel, 3), 7, np.uint8)
    for rank, followed in ((0, False), (3, True)):
        got = lref.frame(base, rank, followed)
        for y in range(panel):
            for x in range(panel):
                m = min(y, x, panel - 1 - y, panel - 1 - x)
                if m < t:
                    want = tuple(lref.RANK_COLOURS[rank])
                elif followed and m < 2 * t:
                    want = (255, 255, 255)
                else:
                    want = (7, 7, 7)
                assert tuple(got[y, x]) == want, (panel, rank, followed, y, x)
    if panel <= 2:      # every pixel is on the edge: the whole panel is the frame, followed or not
        assert (lref.frame(base, 1, True) == lref.RANK_COLOURS[1]).all()
    if panel == 101:    # two rings of width 2: 101^2 - 97^2 coloured pixels, 97^2 - 93^2 white ones
        got = lref.frame(base, 2, True)
        assert (got == lref.RANK_COLOURS[2]).all(axis=2).sum() == 101 ** 2 - 97 ** 2
        assert (got == 255).all(axis=2).sum() == 97 ** 2 - 93 ** 2


def test_overwrite_order_across_lanes():
    import lane_report_reference as lref

    S = 12
    before = np.zeros((3, S, S), np.float32)
    before[:] = 100.5 / 255.0                                           # quantises to 100
    row = [(1, 4, 0, 4, 11, 1, 1, 2, 3)]                                # lane 0: a horizontal segment (its own colour is ignored)
    column = [(1, 0, 6, 11, 6, 1, 9, 9, 9)]                             # lane 1: a vertical one: they cross at (4, 6)
    img = lref.before_panel(before, [row, column])
    c0, c1 = lref.RANK_COLOURS[0].astype(int), lref.RANK_COLOURS[1].astype(int)
    assert tuple(img[4, 6]) == tuple((9 * c1 + 100 + 5) // 10)          # the later lane, blended ONCE with the base
    assert tuple(img[4, 5]) == tuple((9 * c0 + 100 + 5) // 10) and tuple(img[3, 6]) == tuple((9 * c1 + 100 + 5) // 10)
    assert tuple(img[0, 0]) == (100, 100, 100)
    swapped = lref.before_panel(before, [column, row])                 # rank order decides, not the geometry
    assert tuple(swapped[4, 6]) == tuple((9 * c1 + 100 + 5) // 10) and tuple(swapped[4, 5]) == tuple((9 * c1 + 100 + 5) // 10)
    assert tuple(swapped[3, 6]) == tuple((9 * c0 + 100 + 5) // 10)
    # the strip: black panels for the lanes that were not executed and for a null after, no frame on them
    after = np.ones((3, S, S), np.float32)
    strip = lref.strip(before, [after, None], [row, column], 0, 3, 10)
    assert strip.shape == (10, 40, 3)
    assert (strip[:, 20:] == 0).all()                                   # lane 1 (null after) and lane 2 (not executed)
    assert tuple(strip[0, 10]) == tuple(c0) and tuple(strip[1, 11]) == (255, 255, 255) and tuple(strip[2, 12]) == (255, 255, 255)
    assert tuple(lref.strip(before, [after], [row], -1, 1, 10)[1, 11]) == (255, 255, 255)   # (the after image itself: no white frame ...
    assert tuple(lref.strip(before, [after * 0.5], [row], -1, 1, 10)[1, 11]) == (127, 127, 127)   # ... as a grey one shows)


# ---- refusals: FS_ERR_ARG and a message, before any HIP call (there is no device here) --------------------------------------
def _record(n_lanes=2, followed=0, n_prims=1, prim=(1, 2, 3, 4, 5, 1, 255, 0, 0)):
    from flingbot_amd import report
    table = np.zeros(1, report.LANE_RECORD)
    table["before"] = FAKE
    table["after"][0, :] = FAKE
    table["n_lanes"], table["followed"] = n_lanes, followed
    table["n_prims"][0, :] = n_prims
    table["prims"][0, :, :min(max(n_prims, 0), 8)] = prim
    return table


def _panels(lib, table, n=1, lanes=2, S=400, panel=200, out=FAKE, work=FAKE):
    return lib.fs_lane_panels(None if table is None else table.ctypes.data, n, lanes, S, panel, out, work, None)


def _refused(lib, rc, *words):
    assert rc == FS_ERR_ARG
    msg = lib.fs_last_error().decode()
    assert msg and all(w in msg for w in words), msg


def test_lane_panels_refusals():
    from flingbot_amd import sim as fsim

    lib = fsim.load_library()
    good = _record()
    _refused(lib, _panels(lib, None), "null")
    _refused(lib, _panels(lib, good, out=None), "null")
    _refused(lib, _panels(lib, good, work=None), "null")
    for n in (0, -1, 65536):
        _refused(lib, _panels(lib, good, n=n), "records")
    for lanes in (0, 9):
        _refused(lib, _panels(lib, good, lanes=lanes), "lanes")
    for kw in (dict(panel=0), dict(panel=4097), dict(S=0), dict(S=4097)):
        _refused(lib, _panels(lib, good, **kw), "4096")
    _refused(lib, _panels(lib, good, work=FAKE + 8), "aligned")
    _refused(lib, _panels(lib, good, out=FAKE + 2), "aligned")
    bad = _record()
    bad["before"] = 0
    _refused(lib, _panels(lib, bad), "record 0", "null")
    bad = _record()
    bad["after"][0, 1] = FAKE + 2
    _refused(lib, _panels(lib, bad), "record 0", "float grid")
    for n_lanes in (0, 3, -1):
        _refused(lib, _panels(lib, _record(n_lanes=n_lanes, followed=-1)), "record 0", "lanes")
    for followed in (-2, 2):
        _refused(lib, _panels(lib, _record(followed=followed)), "record 0", "follows")
    _refused(lib, _panels(lib, _record(n_prims=9)), "lane 0", "9 primitives")
    _refused(lib, _panels(lib, _record(n_prims=-1)), "primitives")
    for slot in (1, 2, 3, 4):
        for value in (8192, -8192):
            prim = [1, 2, 3, 4, 5, 1, 255, 0, 0]
            prim[slot] = value
            _refused(lib, _panels(lib, _record(prim=tuple(prim))), "8191")
    _refused(lib, _panels(lib, _record(prim=(1, 2, 3, 4, 5, 0, 255, 0, 0))), "thickness")
    _refused(lib, _panels(lib, _record(prim=(0, 2, 3, 4, 5, 65, 255, 0, 0))), "thickness")
    _refused(lib, _panels(lib, _record(prim=(2, 2, 3, 4, 5, 1, 255, 0, 0))), "kind")
    _refused(lib, _panels(lib, _record(prim=(1, 2, 3, 4, 5, 1, 256, 0, 0))), "colour")
    # records are checked in order and every limit itself passes: a first record on all limits, a bad second one
    edge = _record(n_lanes=8, followed=7, n_prims=8, prim=(1, 8191, -8191, 8191, -8191, 64, 255, 255, 255))
    two = np.concatenate([edge, _record()])
    two["prims"][1, 1, 0, 5] = 65
    _refused(lib, _panels(lib, two, n=2, lanes=8, S=4096, panel=4096), "record 1", "lane 1", "primitive 0", "thickness")
    # a lane that was not executed is not looked at
    two = np.concatenate([edge, _record(n_lanes=1)])
    two["n_prims"][1, 1] = 99
    two["before"][1] = 0
    _refused(lib, _panels(lib, two, n=2, lanes=8), "record 1", "null")


# ---- switches -----------------------------------------------------------------------------------------------------------------
def test_evaluate_lane_report_options(capsys, monkeypatch):
    from flingbot_amd import evaluate

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    ap = evaluate.build_parser()
    a = evaluate.parse_lookahead_options(ap, ap.parse_args(["--tasks", "t.npz", "--lookahead", "4", "--lane-report", "out",
                                                            "--report-panel", "96", "--report-tasks", "0", "3"]))
    assert evaluate.report_env_kwargs(a) == dict(action_report=True, report_root="out", report_panel=96, report=[0, 3])
    for extra, message in ((["--lane-report", "out"], "--lookahead"), (["--lookahead", "9", "--slots", "96", "--lane-report", "out"], "8 lanes")):
        with pytest.raises(SystemExit) as err:
            evaluate.parse_lookahead_options(ap, ap.parse_args(["--tasks", "t.npz"] + extra))
        assert err.value.code == 2 and message in capsys.readouterr().err


def test_run_episodes_refuses_films_only():
    """The refusal is raised before the environment is used: a stand-in with the two switches is enough."""
    from types import SimpleNamespace
    from flingbot_amd import lookahead

    with pytest.raises(ValueError, match="film") as err:
        lookahead.run_episodes(None, SimpleNamespace(dump_visualizations=True, action_report=False), [], 2)
    assert "report" not in str(err.value)
    # with the report on and nine lanes the strip cannot be drawn: refused before anything runs, too
    env = SimpleNamespace(dump_visualizations=False, action_report=True, sim=SimpleNamespace(n_envs=18))
    with pytest.raises(ValueError, match="8 lanes"):
        lookahead.run_episodes(None, env, [], 9)


# ---- index.html ---------------------------------------------------------------------------------------------------------------
def test_write_report_names_every_lane_strip(tmp_path):
    from flingbot_amd import report

    root = str(tmp_path / "report")
    log = report.ActionLog(root)
    strip = np.zeros((4, 16, 3), np.uint8)
    lanes = [dict(rank=0, primitive="fling", transform_index=3, pixel=[10, 11], value=0.5, reward=0.25, terminated=False),
             dict(rank=1, primitive="fling", transform_index=5, pixel=[20, 21], value=0.4, reward=0.75, terminated=False)]
    for task, step in ((7, 1), (7, 0), (2, 0)):
        name = f"episode{task:05d}"
        meta = dict(key=f"{name}_step{step:02d}_lanes", task=name, step=step, lanes=lanes, followed_rank=1,
                    preaction_coverage=0.5, postaction_coverage=1.25, max_coverage=2.0)
        png = log.write(name, meta, strip, suffix="_lanes")
        assert os.path.basename(png) == f"step{step:02d}_lanes.png" and os.path.exists(png)
    # an ordinary action next to them, in the same list
    meta = dict(key="episode00002_step00", task="episode00002", step=0, primitive="fling", rotation=0.0, scale=1.0,
                max_indices=[0, 1, 2], preaction_coverage=0.5, postaction_coverage=1.0, max_coverage=2.0, film_dir=None)
    log.write("episode00002", meta, np.zeros((4, 20, 3), np.uint8))
    rows = [json.loads(line) for line in open(os.path.join(root, report.ACTIONS_FILE))]
    assert len(rows) == 4 and sum("lanes" in r for r in rows) == 3
    html = open(report.write_report(root)).read()
    want = ["episode00002/step00.png", "episode00002/step00_lanes.png", "episode00007/step00_lanes.png",
            "episode00007/step01_lanes.png"]
    assert [html.count(f'src="{p}"') for p in want] == [1, 1, 1, 1]
    at = [html.index(f'src="{p}"') for p in want]
    assert at == sorted(at) and html.count("<tr>") == 5
    # the per-step regret: (0.75 - 0.25) / 2.0, and what each lane earned
    assert html.count("regret 0.2500") == 3 and html.count("followed rank 1") == 3
    assert "rank 1: fling, value 0.4000, reward 37.5 %" in html and "62.5 %" in html
    # a directory without lane entries gives the page it gave before: no word about lanes
    plain = str(tmp_path / "plain")
    report.ActionLog(plain).write("episode00002", meta, np.zeros((4, 20, 3), np.uint8))
    assert "look-ahead" not in open(report.write_report(plain)).read()
