"""The on-device picker (fs_k_picker_step behind fs_movep, fs_movep_batch and fs_advance) on the constructed particle sets of
tests/picker_cases.py: ties, the inclusive threshold, contested / released / already moved particles, empty searches, 1 to 16
pickers, 1 to 272 particles.  The expected states are tests/golden/picker_edges_golden.npz, recorded from the reference's own
Picker classes; every comparison is exact (picked indices, iteration counts) or bit-wise (shape states, positions with w)."""
import os

import numpy as np
import pytest

import picker_cases as pc

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "picker_edges_golden.npz")
NAMES = [c["name"] for c in pc.CASES]


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).ravel().view(np.uint32)


def _start(ctx, e, case):
    """The case's start on episode e: scene, particles, spheres as Picker.reset leaves them on the case's centres, picker reset."""
    env = ctx.env(e)
    pc.setup(env, case)
    for c in case["centres"]:
        env.add_sphere(case["picker_radius"], c, [1, 0, 0, 0])
    env.set_shape_states(env.get_shape_states())
    pc.set_centres(env, case)
    ctx.picker_reset(e, picker_threshold=case["picker_threshold"], particle_radius=case["particle_radius"],
                     picker_radius=case["picker_radius"])
    assert ctx.picked(e).tolist() == [-1] * case["num_picker"]


def _assert_step(ctx, e, gold, name, step, what):
    """Episode e stands where the fixture's case `name` stands after simulated step `step` (0-based)."""
    assert ctx.picked(e).tolist() == gold[name + ":picked"][step].tolist(), what
    assert np.array_equal(_bits(ctx.get_shape_states(e)), _bits(gold[name + ":shapes"][step])), what
    got, want = ctx.get_positions(e).reshape(-1, 4), gold[name + ":pos"][step]
    assert np.array_equal(got[:, 3].view(np.uint32), want[:, 3].view(np.uint32)), what + ": inverse masses"
    assert np.array_equal(_bits(got), _bits(want)), what


def _run_program(ctx, e, case, gold, what):
    after = pc.step_after_call(case)
    for k, m in enumerate(case["program"]):
        iters = ctx.movep(e, m["targets"], m["grasp"], speed=m["speed"], min_steps=m["min_steps"])
        assert iters == gold[case["name"] + ":iters"][k], f"{what}, movep {k}"
        assert ctx.last_movep_steps == m["steps"]
        assert after[k] > 0
        _assert_step(ctx, e, gold, case["name"], after[k] - 1, f"{what}, after movep {k}")


@pytest.mark.parametrize("solver", [0, 1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_case_matches_reference_picker(gpu_required, gold, name, solver):
    """One case, one movep call at a time: after every call the picked indices, the shape states, the positions with w and the
    iteration count are the reference's."""
    from flingbot_amd import sim as fsim

    case = pc.BY_NAME[name]
    ctx = fsim.FlingSim(n_envs=1, solver=solver)
    _start(ctx, 0, case)
    _run_program(ctx, 0, case, gold, f"{name}, solver {solver}")
    ctx.close()


def test_slot_reuse_small_then_large(gpu_required, gold):
    """An episode slot that held a 3 x 2 scene (6 saved inverse masses) gets the 17 x 16 scene and a picker reset: the grasp of
    particle 262 and its release restore 262's own inverse mass, the pinned particle's stays 0."""
    from flingbot_amd import sim as fsim

    ctx = fsim.FlingSim(n_envs=1, solver=0)
    for name in ("small_3x2", "inverse_masses", "small_1x1_two_pickers", "pickers_16"):
        _start(ctx, 0, pc.BY_NAME[name])
        _run_program(ctx, 0, pc.BY_NAME[name], gold, f"slot reuse: {name}")
    ctx.close()


def _oracle_run(case, calls):
    """The restated picker on the CPU oracle through `calls` = [(targets, grasp, speed)]: per call (iterations, picked, shape
    states, positions)."""
    from oracle import OracleSim
    from oracle.picker import OraclePicker

    orc = OracleSim()
    pc.setup(orc, case)
    tool = OraclePicker(orc, num_picker=case["num_picker"], picker_radius=case["picker_radius"],
                        picker_threshold=case["picker_threshold"], particle_radius=case["particle_radius"])
    tool.reset(case["centres"])
    out = []
    for targets, grasp, speed in calls:
        it = tool.movep(targets, [bool(g) for g in grasp], speed=speed)
        out.append((it, [-1 if q is None else q for q in tool.picked_particles], orc.get_shape_states().copy(),
                    orc.get_positions().copy(), tool.last_sim_steps))
    return out


def test_batch_out_of_order_with_unlisted_episode(gpu_required):
    """Four episodes, three of them listed as [2, 0, 1]: ids[slot] and cmds[slot] go by slot, picked_ptrs[e] by episode.  The
    episodes carry different scenes (272, 2 and 6 particles) and their moves take 3, 1 and 2 simulated steps, then 1, 3 and 2, so
    the launch lists shrink at different steps.  Each ends exactly as it does alone on the CPU oracle; the fourth is untouched."""
    from flingbot_amd import sim as fsim

    by_episode = {0: pc.BY_NAME["small_2x1"], 1: pc.BY_NAME["small_3x2"], 2: pc.BY_NAME["tie_same_stride"],
                  3: pc.BY_NAME["small_3x2"]}
    listed = [2, 0, 1]
    ctx = fsim.FlingSim(n_envs=4, solver=0)
    for e, case in by_episode.items():
        _start(ctx, e, case)
    before = (ctx.picked(3).copy(), ctx.get_shape_states(3).copy(), ctx.get_positions(3).copy())
    speed = 1.5 * pc.U
    rise = {2: [4.0, 5.0], 0: [1.0, 5.0], 1: [2.5, 5.0]}     # heights (in U) of the two calls' targets above the centre
    grasp = {2: [[1], [0]], 0: [[1], [1]], 1: [[1], [0]]}
    calls = {e: [(by_episode[e]["centres"] + [0, rise[e][k] * pc.U, 0], grasp[e][k], speed) for k in range(2)] for e in listed}
    want = {e: _oracle_run(by_episode[e], calls[e]) for e in listed}
    for k in range(2):
        iters = ctx.movep(listed, np.array([calls[e][k][0] for e in listed]), [calls[e][k][1] for e in listed], speed=speed)
        assert iters.tolist() == [want[e][k][0] for e in listed]
        assert ctx.last_movep_steps == sum(want[e][k][4] for e in listed)
        for e in listed:
            it, picked, shapes, pos, _ = want[e][k]
            assert ctx.picked(e).tolist() == picked, (k, e)
            assert np.array_equal(_bits(ctx.get_shape_states(e)), _bits(shapes)), (k, e)
            assert np.array_equal(_bits(ctx.get_positions(e)), _bits(pos)), (k, e)
    assert [want[e][0][4] for e in listed] == [3, 1, 2] and [want[e][1][4] for e in listed] == [1, 3, 2]
    assert [want[e][0][1] for e in listed] == [[5], [1], [4]] and [want[e][1][1] for e in listed] == [[-1], [1], [-1]]
    assert ctx.picked(3).tolist() == before[0].tolist()
    assert np.array_equal(_bits(ctx.get_shape_states(3)), _bits(before[1]))
    assert np.array_equal(_bits(ctx.get_positions(3)), _bits(before[2]))
    ctx.close()


@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("name", ["contention_two", "contention_one", "release_and_retake"])
def test_advance_in_chunks_behind_a_waiter(gpu_required, name, cap):
    """The contested cases through fs_advance, at a speed that makes every movep several simulated steps long, in chunks of at
    most `cap` steps, with a wait_until_stable episode listed first in every call (the launch row is [waiters | movers], so the
    picker's id list starts behind it): the mover ends every movep on the bits of the plain movep run, which are the oracle's."""
    from flingbot_amd import sim as fsim

    case = pc.BY_NAME[name]
    speed = 2 * pc.U
    calls = [(m["targets"], m["grasp"], speed) for m in case["program"]]
    want = _oracle_run(case, calls)
    assert want[-1][1] == case["expected_picked"][-1].tolist() and sum(w[4] for w in want) >= 2 * len(calls)
    S = case["num_picker"]

    plain = fsim.FlingSim(n_envs=1, solver=0)
    _start(plain, 0, case)
    ctx = fsim.FlingSim(n_envs=2, solver=0)
    _start(ctx, 0, pc.BY_NAME["small_3x2"])     # the waiter: never stable (tolerance 0), 1000 steps to go
    _start(ctx, 1, case)
    w_start = 0
    for k, (targets, grasp, _) in enumerate(calls):
        it_plain = plain.movep(0, targets, grasp, speed=speed)
        start, n_calls, steps = 0, 0, 0
        while True:
            tg = np.zeros((2, S, 3))
            tg[1] = targets
            prog, status, st = ctx.advance([0, 1], [1, 0], tg, [[0] * S, grasp], [0.0, speed], [1000, 1000], [-1, -1], [0, 0],
                                           [w_start, start], cap_min=1, cap=cap, tolerance=0.0)
            n_calls += 1
            steps += int(st[1])
            assert 0 <= st[1] <= cap and status[0] == 0 and st[0] == max(int(st[1]), 1)
            w_start, start = int(prog[0]), int(prog[1])
            if status[1] != 0:
                break
            assert n_calls < 50
        it, picked, shapes, pos, sim_steps = want[k]
        assert status[1] == 1 and start == it == it_plain and steps == sim_steps
        assert n_calls >= -(-sim_steps // cap)
        for c, e in ((plain, 0), (ctx, 1)):
            assert c.picked(e).tolist() == picked, (k, e)
            assert np.array_equal(_bits(c.get_shape_states(e)), _bits(shapes)), (k, e)
            assert np.array_equal(_bits(c.get_positions(e)), _bits(pos)), (k, e)
    assert ctx.picked(0).tolist() == [-1]
    plain.close()
    ctx.close()
