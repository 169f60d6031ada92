"""The constructed picker cases (tests/picker_cases.py) against tests/golden/picker_edges_golden.npz, which was recorded from
the reference's own Picker / PickerPickPlace classes (tests/golden/make_golden.py picker_edges): the table's hand-derived
answers are the reference's, oracle/picker.py restates the reference bit for bit on them, the library's host planner gives
the reference's iteration and step counts, and no case is vacuous.  No GPU needed."""
import os

import numpy as np
import pytest

import picker_cases as pc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "picker_edges_golden.npz")
NAMES = [c["name"] for c in pc.CASES]


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def test_fixture_is_small_and_covers_the_table(gold):
    assert os.path.getsize(GOLD) < 300 * 1024
    assert gold["names"].tolist() == NAMES
    for case in pc.CASES:
        n, S, steps = case["pos"].shape[0], case["num_picker"], len(case["expected_picked"])
        assert gold[case["name"] + ":picked"].shape == (steps, S)
        assert gold[case["name"] + ":shapes"].shape == (steps, 14 * S)
        assert gold[case["name"] + ":pos"].shape == (steps, n, 4)
        assert gold[case["name"] + ":iters"].shape == (len(case["program"]),)


@pytest.mark.parametrize("name", NAMES)
def test_reference_picks_what_the_construction_implies(gold, name):
    case = pc.BY_NAME[name]
    assert gold[name + ":picked"].tolist() == case["expected_picked"].tolist()


@pytest.mark.parametrize("name", NAMES)
def test_no_case_is_vacuous(name):
    case = pc.BY_NAME[name]
    assert (case["expected_picked"] != case["decoy"]).any(), "the decoy kernel would pass this case"
    assert case["picker_threshold"] + case["picker_radius"] + case["particle_radius"] == 5 * 2.0 ** -8
    assert case["num_picker"] <= 16


def test_every_rule_has_its_cases():
    assert set(pc.RULES) == {"ties", "threshold", "held exclusion", "empty search", "un-pick", "teleport", "particle counts",
                             "picker counts"}
    for rule, names in pc.RULES.items():
        assert names and all(n in pc.BY_NAME for n in names), rule
    assert {c["name"] for c in pc.CASES} == {n for names in pc.RULES.values() for n in names}
    assert sorted({c["pos"].shape[0] for c in pc.CASES}) == [1, 2, 6, 256, 272]        # below, at and above one block
    assert sorted({c["num_picker"] for c in pc.CASES}) == [1, 2, 3, 4, 16]
    # an empty search really occurs and is followed by another search of the same picker
    for name in pc.RULES["empty search"]:
        case = pc.BY_NAME[name]
        assert len(case["program"]) >= 2 and all(m["grasp"][-1] for m in case["program"])
        assert case["expected_picked"][0, -1] == -1


def test_exact_distances_of_the_constructed_ties():
    """The tie and threshold cases rest on float64 distances that are exactly equal (or exactly 5U): check the arithmetic the
    kernel, cdist and the oracle share -- ((dx^2 + dy^2) + dz^2), then sqrt -- on the float32 coordinates."""
    def dist(case, i, centre):
        d = case["pos"][i, :3].astype(np.float64) - np.asarray(centre, np.float32).astype(np.float64)
        return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])

    thr = 5 * pc.U
    for name in ("tie_same_stride", "tie_reduce_128", "tie_reduce_0_255", "tie_reduce_adjacent"):
        case = pc.BY_NAME[name]
        lo, hi = int(case["expected_picked"][0, 0]), int(case["decoy"][0, 0])
        assert lo < hi and dist(case, lo, case["centres"][0]) == dist(case, hi, case["centres"][0]) == thr
        others = [dist(case, i, case["centres"][0]) for i in range(case["pos"].shape[0]) if i not in (lo, hi)]
        assert min(others) > thr
    case = pc.BY_NAME["threshold_inclusive"]
    assert dist(case, 0, case["centres"][0]) == thr
    case = pc.BY_NAME["threshold_one_ulp_out"]
    d = dist(case, 0, case["centres"][0])
    assert thr < d < thr + 2.0 ** -28  # beyond it by about one float32 ulp of the distance
    assert case["pos"][0].view(np.uint32)[0] == pc.BY_NAME["threshold_inclusive"]["pos"][0].view(np.uint32)[0] - 1  # (x < 0)
    case = pc.BY_NAME["float64_distance"]
    near, far = dist(case, 180, case["centres"][0]), dist(case, 50, case["centres"][0])
    assert near < far < thr
    d32 = case["pos"][[180, 50], :3] - case["centres"][0].astype(np.float32)
    sq = (d32[:, 0] * d32[:, 0] + d32[:, 1] * d32[:, 1]) + d32[:, 2] * d32[:, 2]
    assert sq.dtype == np.float32 and sq[0] == sq[1]  # float32 cannot tell them apart


def test_inverse_masses_come_back_bit_for_bit(gold):
    case = pc.BY_NAME["inverse_masses"]
    w0 = case["pos"][:, 3]
    assert len(set(w0[w0 != 0].view(np.uint32).tolist())) == np.count_nonzero(w0) == 270 and w0[31] == 0 and w0[30] == 0
    w = gold["inverse_masses:pos"][:, :, 3]
    held = w[0].copy()
    assert held[31] == 0 and held[262] == 0
    held[262] = w0[262]
    assert np.array_equal(held.view(np.uint32), w0.view(np.uint32))           # while held: only 262 changed
    assert np.array_equal(w[1].view(np.uint32), w0.view(np.uint32))           # released: every particle its own again
    case = pc.BY_NAME["threshold_one_ulp_out"]
    assert np.array_equal(gold["threshold_one_ulp_out:pos"][0, :, 3].view(np.uint32), case["pos"][:, 3].view(np.uint32))
    w = gold["release_and_retake:pos"][:, 100, 3]
    assert w.tolist() == [0.0, 0.0]                                            # re-taken in the step it was released in


def test_teleport_is_left_to_right(gold):
    """(p + new) - old, float32, left to right: on the off-lattice case the other association gives other bits."""
    case = pc.BY_NAME["teleport_association"]
    pos, shapes = gold["teleport_association:pos"], gold["teleport_association:shapes"]
    differ = 0
    for s in range(len(pos)):
        p = (case["pos"] if s == 0 else pos[s - 1])[90, :3]
        new, old = shapes[s][:3], shapes[s][3:6]
        assert np.array_equal(old, (case["centres"][0].astype(np.float32) if s == 0 else shapes[s - 1][:3]))
        left = (p + new) - old
        assert left.dtype == np.float32 and np.array_equal(pos[s][90, :3].view(np.uint32), left.view(np.uint32))
        differ += int(not np.array_equal(left, p + (new - old)))
    assert differ >= 1


@pytest.mark.parametrize("name", NAMES)
def test_restated_picker_matches_the_reference_class(gold, name):
    """oracle/picker.py on the CPU oracle, step by step against the fixture: picked, shape states, positions with w, iterations."""
    from oracle import OracleSim
    from oracle.picker import OraclePicker

    case = pc.BY_NAME[name]
    orc = OracleSim()
    pc.setup(orc, case)
    tool = OraclePicker(orc, num_picker=case["num_picker"], picker_radius=case["picker_radius"],
                        picker_threshold=case["picker_threshold"], particle_radius=case["particle_radius"])
    tool.reset(case["centres"])
    after = pc.step_after_call(case)
    for k, m in enumerate(case["program"]):
        iters = tool.movep(m["targets"], [bool(g) for g in m["grasp"]], speed=m["speed"], min_steps=m["min_steps"])
        assert iters == gold[name + ":iters"][k]
        assert tool.last_sim_steps == m["steps"]
        s = after[k] - 1
        assert [-1 if q is None else q for q in tool.picked_particles] == gold[name + ":picked"][s].tolist()
        assert np.array_equal(orc.get_shape_states().view(np.uint32), gold[name + ":shapes"][s].view(np.uint32))
        assert np.array_equal(orc.get_positions().view(np.uint32), gold[name + ":pos"][s].ravel().view(np.uint32))


@pytest.mark.parametrize("name", NAMES)
def test_host_plan_counts(gold, name):
    """fs_host_plan_movep from the pickers' recorded positions: the reference's iteration count and the simulated steps of
    every movep, the standing one (4 iterations, no step) included, and the float32 positions the pickers end on."""
    from flingbot_amd import sim as fsim

    case = pc.BY_NAME[name]
    after = pc.step_after_call(case)
    cur = case["centres"].astype(np.float32)
    for k, m in enumerate(case["program"]):
        plan = fsim.host_plan_movep(cur, m["targets"], m["speed"], min_steps=m["min_steps"])
        assert (plan["iterations"], plan["steps"], plan["status"]) == (int(gold[name + ":iters"][k]), m["steps"], 1)
        if after[k] > 0:
            cur = gold[name + ":shapes"][after[k] - 1].reshape(-1, 14)[:, :3]
        assert np.array_equal(plan["end_pos"].view(np.uint32), np.ascontiguousarray(cur).view(np.uint32))
    assert pc.BY_NAME["release_while_standing"]["program"][1]["steps"] == 0
