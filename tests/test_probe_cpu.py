"""The probe's host side (flingbot_amd/probe.py, report.compose_probe's rules, evaluate's options): lattice geometry, rank
statistics on constructed maps against tests/probe_reference.py's independent restatement, the strip's restatement on a map
small enough to check by hand, lane records through the replay file into ONE group, and the command line."""
import json
import os
import re

import numpy as np
import pytest

import probe_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- lattice geometry ---------------------------------------------------------------------------------------------------------
def test_lattice_always_contains_the_chosen_pixel():
    from flingbot_amd import probe

    for D, g in ((64, 8), (32, 4), (17, 3)):
        for stride in range(1, D):
            for chosen in range(g, D - g):
                origin, count = probe.lattice_axis(chosen, stride, g, D)
                cells = [origin + i * stride for i in range(count)]
                assert chosen in cells and g <= cells[0] < g + stride and cells[-1] <= D - 1 - g < cells[-1] + stride
    assert probe.lattice_axis(8, 1, 8, 64) == (8, 48)            # stride 1: the whole interior
    assert probe.lattice_axis(55, 16, 8, 64) == (23, 3)          # 23, 39, 55: the chosen pixel is the last row
    assert probe.lattice_axis(30, 5, 8, 64) == (10, 10)          # 48 interior pixels, stride 5 does not divide them: 10 .. 55
    assert probe.lattice_axis(9, 5, 8, 64) == (9, 10)            # ... and from 9 the last cell is 54
    for bad in ((7, 4), (56, 4), (20, 0)):
        with pytest.raises(ValueError):
            probe.lattice_axis(bad[0], bad[1], 8, 64)


# ---- statistics ---------------------------------------------------------------------------------------------------------------
def _check(predicted, measured, chosen, flat=2.0):
    from flingbot_amd import probe

    got = probe.map_stats(predicted, measured, chosen, flat)
    want = ref.spearman(predicted, measured)
    assert (got["spearman"] is None) == (want is None)
    if want is not None:
        assert abs(got["spearman"] - want) <= 1e-12
    assert (got["pairs"], got["concordant"]) == ref.pair_counts(predicted, measured)
    return got


def test_stats_on_constructed_maps():
    nan = np.nan
    # ties on both sides; the chosen cell (0, 1) shares the best reward with (1, 0): ties go to the chosen cell
    predicted = np.float32([[0.5, 0.9, 0.9], [0.1, 0.1, nan]])
    measured = np.float32([[0.2, 0.4, 0.1], [0.4, nan, 0.3]])
    got = _check(predicted, measured, (0, 1))
    assert got["n_cells"] == 4 and got["chosen_rank"] == 0 and got["lattice_regret"] == 0.0
    assert got["chosen_reward"] == float(np.float32(0.4)) == got["best_reward"]
    # rewards b = d = 0.4 > a = 0.2 > c = 0.1: the pairs (b, a), (b, c), (d, a), (d, c), (a, c); predicted 0.9 / 0.1 / 0.5 / 0.9
    # agrees on (b, a) alone -- (b, c) is a tie of predictions, which is not agreement
    assert got["pairs"] == 5 and got["concordant"] == 1
    # the chosen cell is the worst of three
    got = _check(np.float32([[3.0, 2.0, 1.0]]), np.float32([[0.0, 0.5, 1.0]]), (0, 0), flat=4.0)
    assert got["chosen_rank"] == 2 and got["lattice_regret"] == 0.25 and got["spearman"] == pytest.approx(-1.0, abs=1e-15)
    assert got["pairs"] == 3 and got["concordant"] == 0
    # one executed cell: nothing to correlate
    got = _check(np.float32([[1.0, 2.0]]), np.float32([[nan, 0.3]]), (0, 1))
    assert got["spearman"] is None and got["n_cells"] == 1 and got["chosen_rank"] == 0 and got["pairs"] == 0
    # zero variance on one side
    assert _check(np.float32([[1.0, 1.0, 1.0]]), np.float32([[0.1, 0.2, 0.3]]), (0, 0))["spearman"] is None
    assert _check(np.float32([[1.0, 2.0, 3.0]]), np.float32([[0.1, 0.1, 0.1]]), (0, 0))["spearman"] is None
    # all NaN, and an empty map
    for p, m in ((np.float32([[1.0, 2.0]]), np.float32([[nan, nan]])), (np.zeros((0, 0), np.float32), np.zeros((0, 0), np.float32))):
        got = _check(p, m, None)
        assert got == dict(n_cells=0, chosen_reward=None, best_reward=None, lattice_regret=None, chosen_rank=None, spearman=None,
                           pairs=0, concordant=0)
    # the chosen cell was not executed: what needs it is None, the rest stands
    got = _check(np.float32([[1.0, 2.0, 3.0]]), np.float32([[nan, 0.2, 0.1]]), (0, 0))
    assert got["chosen_rank"] is None and got["lattice_regret"] is None and got["best_reward"] == float(np.float32(0.2))


def test_spearman_equals_the_counting_restatement_on_random_maps():
    rng = np.random.default_rng(3)
    for n, levels in ((7, 3), (64, 5), (4096, 50), (300, 10 ** 6)):       # many ties ... practically none
        predicted = rng.integers(0, levels, n).astype(np.float32).reshape(1, n)
        measured = (rng.integers(0, levels, n) / levels).astype(np.float32).reshape(1, n)
        measured[0, rng.random(n) < 0.2] = np.nan
        if n <= 300:
            _check(predicted, measured, (0, 0))
        else:   # (the reference's pair count is a Python double loop: the correlation alone at the largest size)
            from flingbot_amd import probe
            assert abs(probe.map_stats(predicted, measured, None, 1.0)["spearman"] - ref.spearman(predicted, measured)) <= 1e-12


def test_summarize_and_ranks():
    from flingbot_amd import probe

    maps = [dict(n_executed=3, stats=dict(lattice_regret=0.1, chosen_rank=1, spearman=0.5, pairs=3, concordant=2)),
            dict(n_executed=1, stats=dict(lattice_regret=0.3, chosen_rank=0, spearman=None, pairs=0, concordant=0)),
            dict(n_executed=0, stats=dict(lattice_regret=None, chosen_rank=None, spearman=None, pairs=1, concordant=0))]
    got = probe.summarize(maps)
    assert got == dict(lattice_regret=pytest.approx(0.2), chosen_rank=0.5, spearman=0.5, pairs=4, concordant=2, pair_accuracy=0.5,
                       n_maps=3, n_executed=4)
    assert probe.summarize([])["lattice_regret"] is None and probe.summarize([])["pair_accuracy"] is None
    predicted = np.float32([[0.5, 0.9, 0.9], [0.1, np.nan, 0.9]])
    executed = np.array([[True, True, True], [False, True, True]])
    assert probe.cell_ranks(predicted, executed) == {(0, 1): 0, (0, 2): 1, (1, 2): 2, (0, 0): 3, (1, 1): 4}


# ---- the strip's restatement, by hand -----------------------------------------------------------------------------------------
def test_measured_image_by_hand():
    table = np.arange(768, dtype=np.int64).reshape(256, 3) % 251
    table = table.astype(np.uint8)
    nan = np.nan
    measured = np.float32([[0.0, nan], [nan, 1.0]])
    valid = np.array([[False, True], [False, True]])
    # D = 8, origin (2, 3), stride 3: cell rows 1 .. 3 | 4 .. 6, cell columns 2 .. 4 | 5 .. 7; row 0, 7 and columns 0, 1 outside
    img = ref.measured_image(table, 8, measured, valid, (0.0, 2.0), (2, 3), 3, (1, 1))
    assert not img[0].any() and not img[7].any() and not img[:, :2].any()
    assert (img[1:4, 2:5] == table[0]).all()                    # finite, invalid: still jet; t = 0
    assert (img[1:4, 5:8] == 128).all() and (img[4:7, 2:5] == 64).all()
    assert (img[5, 6] == table[128]).all()                      # t = 0.5 -> entry 128, the chosen cell's centre
    ring = [(y, z) for y in (4, 5, 6) for z in (5, 6, 7) if (y, z) != (5, 6)]
    assert all((img[y, z] == 255).all() for y, z in ring)
    # stride 1: every cell is its own outermost pixel; stride 2: ny = y - y0 + 1, the cell of pixel y0 - 1 is 0
    img = ref.measured_image(table, 4, np.float32([[0.5, 0.5], [0.5, 0.5]]), np.ones((2, 2), bool), (0.0, 1.0), (1, 1), 1, (1, 1))
    assert (img[2, 2] == 255).all() and (img[1, 1] == table[128]).all() and not img[0].any() and not img[3].any()
    img = ref.measured_image(table, 6, np.float32([[0.5]]), np.ones((1, 1), bool), (0.0, 1.0), (3, 3), 2, None)
    assert (img[2:4, 2:4] == table[128]).all() and not img[4:].any() and not img[:2].any()
    strip = ref.strip(table, np.zeros((4, 8, 8), np.float32), np.zeros((8, 8), np.float32), (0.0, 2.0), measured, valid, (2, 3), 3,
                      (1, 1), None, [], 5, 12)
    assert strip.shape == (5, 20, 3) and not strip[:, 15:].any() and (strip[:, 5:10] == table[0]).all()


def test_probe_range():
    from flingbot_amd import report

    predicted = np.float32([[5.0, -1.0, np.nan], [0.2, 0.3, 9.0]])
    measured = np.float32([[np.nan, 0.1, 0.7], [0.4, np.nan, np.inf]])
    assert list(report.probe_range(predicted, measured)) == [np.float32(-1.0), np.float32(0.7)]
    assert list(report.probe_range(predicted, np.full((2, 3), np.nan, np.float32))) == [0.0, 0.0]
    assert report.PROBE_RECORD.itemsize == 368


# ---- lane records -> replay file -> one group ---------------------------------------------------------------------------------
def _cell(task, step, pre, post, pixel):
    D = 64
    mask = np.zeros((D, D), bool)
    mask[pixel] = True
    exp = dict(observations=np.full((4, D, D), 0.01 * pixel[0], np.float32), actions=mask, value_map=np.zeros((D, D), np.float32),
               max_indices=np.array([3, *pixel], np.int64), rotation=10.0, scale=1.5)
    return dict(action="fling", pre=pre, post=post, reward=post - pre, experience=exp)


def test_lane_records_come_back_as_one_group_per_map(tmp_path):
    from flingbot_amd import lookahead, probe
    from flingbot_amd.replay import ExperienceSet

    tasks = [dict(cloth_mass=0.5, flatten_area=2.0, task_difficulty="easy", initial_coverage=1.0),
             dict(cloth_mass=0.7, flatten_area=4.0, task_difficulty="hard", initial_coverage=1.2)]
    nan = np.nan
    maps = [dict(task=0, step=0, predicted=np.float32([[0.1, 0.9], [0.9, 0.5]]), measured=np.float32([[0.5, 0.2], [nan, -0.1]])),
            dict(task=1, step=0, predicted=np.float32([[0.3, 0.4]]), measured=np.float32([[1.0, 0.4]])),
            dict(task=1, step=1, predicted=np.zeros((0, 0), np.float32), measured=np.zeros((0, 0), np.float32))]
    cells = [{(0, 0): _cell(0, 0, 1.0, 1.5, (8, 8)), (0, 1): _cell(0, 0, 1.0, 1.2, (8, 24)), (1, 1): _cell(0, 0, 1.0, 0.9, (24, 24))},
             {(0, 0): _cell(1, 0, 1.2, 2.2, (10, 10)), (0, 1): _cell(1, 0, 1.2, 1.6, (10, 26))}, {}]
    recs = probe.lane_records(maps, cells)
    assert [(r["task"], r["step"], r["rank"]) for r in recs] == [(0, 0, 0), (0, 0, 1), (0, 0, 2), (1, 0, 0), (1, 0, 1)]
    assert [r["rewards"][0] for r in recs] == pytest.approx([0.2, -0.1, 0.5, 0.4, 1.0])     # by predicted value, descending
    assert set(recs[0]) == {"coverage", "actions", "rewards", "preaction_coverage", "experience", "task", "step", "rank"}
    path = str(tmp_path / "probes.npz")
    assert lookahead.save_replay(path, dict(lane_records=recs), tasks) == 5
    ds = ExperienceSet(path, obs_color_jitter=False)
    assert len(ds.keys) == 5 and ds.n_invalid == 0 and ds.n_without_arrays == 0
    assert [len(m) for m in ds.group_members()] == [3, 2]                                   # a map is one group
    assert np.array_equal(ds.labels, np.float32([0.2 / 2, -0.1 / 2, 0.5 / 2, 0.4 / 4, 1.0 / 4]))
    idx, bounds, _ = ds.draw_groups(3, np.random.default_rng(0))
    members = [set(m.tolist()) for m in ds.group_members()]
    for (begin, end) in {tuple(b) for b in bounds.tolist()}:
        assert any(set(idx[begin:end].tolist()) <= m for m in members)
    # one draw of a whole map: with room for three and the first map drawn, all of its cells come back together
    for seed in range(20):
        idx, bounds, _ = ds.draw_groups(3, np.random.default_rng(seed))
        if set(idx.tolist()) == members[0]:
            assert bounds.tolist() == [[0, 3]] * 3
            break
    else:
        pytest.fail("no draw returned the three-cell map")
    z = np.load(path)
    assert [int(z[f"{k}/lane_rank"]) for k in z["keys"]] == [0, 1, 2, 0, 1]


def test_save_maps_and_report_row(tmp_path):
    from flingbot_amd import probe, report

    m = dict(task=3, step=1, primitive="fling", transform_index=5, chosen_pixel=[24, 40], origin=[8, 8], shape=[1, 2],
             predicted=np.float32([[0.1, 0.2]]), measured=np.float32([[np.nan, 0.3]]), valid=np.array([[True, True]]),
             on_cloth1=np.array([[False, True]]), on_cloth2=np.array([[False, True]]), terminated=np.array([[False, False]]))
    assert probe.save_maps(str(tmp_path / "maps.npz"), [m, probe._empty_map(4, 0)]) == 2
    z = np.load(str(tmp_path / "maps.npz"))
    assert list(z["keys"]) == ["00003_step01", "00004_step00"] and list(z["00003_step01/lattice"]) == [5, 24, 40, 8, 8, 1, 2]
    assert np.array_equal(z["00003_step01/measured"], m["measured"], equal_nan=True) and z["00004_step00/predicted"].shape == (0, 0)
    log = report.ActionLog(str(tmp_path))
    m.update(n_executed=1, chosen_cell=[0, 1], stats=probe.map_stats(m["predicted"], m["measured"], (0, 1), 2.0))
    probe._file_strip(m, np.zeros((4, 16, 3), np.uint8), 10, log, {3: 2.0}, {})
    row = json.loads(open(os.path.join(str(tmp_path), "actions.jsonl")).read())
    assert row["key"] == "episode00013_step01_probe" and row["png"] == os.path.join("episode00013", "step01_probe.png")
    assert row["stats"]["lattice_regret"] == 0.0 and row["probe"]["measured"] == [[None, float(np.float32(0.3))]]
    page = open(report.write_report(str(tmp_path))).read()
    assert "lattice regret 0.0000" in page and "step01_probe.png" in page and "Spearman -" in page


# ---- the command line ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,message", [
    (["--probe-stride", "4", "--lookahead", "2"], "--lookahead"),
    (["--probe-stride", "4", "--gpus", "2"], "one GPU"),
    (["--probe-stride", "4", "--report", "out"], "--report"),
    (["--probe-stride", "4", "--dump-visualizations", "out"], "--dump-visualizations"),
    (["--probe-steps", "0", "1"], "--probe-stride"),
    (["--probe-report", "out"], "--probe-stride"),
    (["--probe-stride", "0"], ">= 1"),
    (["--probe-stride", "4", "--probe-steps", "-1"], ">= 0"),
    (["--probe-stride", "4", "--slots", "1"], "--slots"),
])
def test_command_line_refusals(capsys, monkeypatch, extra, message):
    from flingbot_amd import evaluate

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as err:
        evaluate.main(["--tasks", "set.npz"] + extra)      # refused while the options are read: no file is opened, no GPU touched
    assert err.value.code == 2 and message in capsys.readouterr().err


def test_command_line_accepts_the_probe(monkeypatch):
    from flingbot_amd import evaluate

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    ap = evaluate.build_parser()
    a = evaluate.parse_probe_options(ap, ap.parse_args(["--tasks", "set.npz", "--slots", "192", "--probe-stride", "4", "--probe-steps",
                                                        "0", "1", "--probe-report", "out", "--report-panel", "96"]))
    assert (a.probe_stride, a.probe_steps, a.probe_report) == (4, [0, 1], "out") and evaluate.report_env_kwargs(a) == {}
    a = evaluate.parse_probe_options(ap, ap.parse_args(["--tasks", "set.npz", "--gpus", "2", "--report", "x"]))
    assert a.probe_stride is None and a.probe_steps is None      # without --probe-stride nothing is checked here, as before


# ---- header and library -------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    from flingbot_amd import sim as fsim

    with open(os.path.join(ROOT, "include", "flingsim.h")) as fh:
        header = fh.read()
    assert re.search(r"\bint fs_lattice_actions\(const float \*d_values, int n, int n_primitives,", header)
    assert re.search(r"\bsize_t fs_lattice_actions_work_bytes\(int n, int n_transforms, int m, int max_cells\);", header)
    assert re.search(r"\bint fs_probe_panels\(const fs_probe_record \*table, int n_records, int obs_dim, int image_dim, int panel,", header)
    lib = fsim.load_library()
    for name in ("fs_lattice_actions", "fs_lattice_actions_work_bytes", "fs_probe_panels", "fs_probe_panels_work_bytes"):
        assert hasattr(lib, name) and name in lib._fs_symbols
    assert lib.fs_lattice_actions_work_bytes(0, 4, 2, 64) == 0 and lib.fs_lattice_actions_work_bytes(2, 4, 2, 0) == 0
    assert lib.fs_lattice_actions_work_bytes(2, 4, 3, 100) >= 2 * 4 * 9 * 8 + 3 * 32 + 3 * 100 * 5
    assert lib.fs_probe_panels_work_bytes(3) == 3 * 368 and lib.fs_probe_panels_work_bytes(0) == 0
    # host-side refusals need no device
    assert lib.fs_lattice_actions(None, 1, 1, None, 1, 32, 4, 4, 4, None, None, 48, 1.0, None, None, None, 1.0, 0.3, 0.02,
                                  None, 1, 1, None, None, None, None) == -1
    assert b"fs_lattice_actions" in lib.fs_last_error()
    assert lib.fs_probe_panels(None, 1, 32, 48, 8, None, None, None) == -1 and b"fs_probe_panels" in lib.fs_last_error()
