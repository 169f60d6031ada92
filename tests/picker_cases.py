"""Constructed particle sets for the on-device picker's grasp search (fs_k_picker_step, flingbot_amd/csrc/fs_picker.hip).

Plain numpy, importable without a GPU.  Every case is a small grid cloth whose particles are set to given positions and
inverse masses, some pickers at given centres, and a program of movep calls; `expected_picked` is the picked index per picker
after every simulated step as the construction implies it, `decoy` what a plausibly wrong kernel would hold instead.
tests/golden/make_golden.py (`picker_edges`) runs the same cases through the reference's own PickerPickPlace class and writes
tests/golden/picker_edges_golden.npz; the CPU and GPU tests compare against that file.

How the answers follow from exact arithmetic:
  * picker centres and the particles that matter have coordinates that are multiples of U = 2^-8, so every difference,
    square and left-to-right sum of squares is exact in float64; offsets such as (3,4,0)U, (5,0,0)U, (0,-4,3)U lie at
    exactly 5U and distinct integer offsets give distinct, exactly ordered squared distances;
  * the grasp threshold is picker_threshold + picker_radius + particle_radius = 0 + 5U + 0 = 5U exactly;
  * a movep whose targets differ from the centres and whose speed exceeds the distance takes exactly one simulated step and
    puts the pickers on the (float32-representable) targets, so they stay on the lattice;
  * the search of a step reads the pickers BEFORE their move and the particles as the previous solver step left them.  The
    first step of a program therefore decides on the constructed state itself.  The solver keeps free particles
    collisionDistance (0.005) off a sphere's surface, i.e. out of a reach that equals the sphere's radius, so on any later
    step only particles that never move can be in reach: those pinned at reset (w = 0) and those a picker holds.  Every
    later-step decision of the table is between such particles and is exact as well.
Particles that must not matter stay in the flat rest layout, at least 5.1U from every centre a search is made from.
"""
import numpy as np

from scenarios import cloth_params

U = 2.0 ** -8
PICKER_RADIUS = 5 * U  # 0.01953125
SPACING = 0.00625      # the grid cloth's rest pitch (1.6 U)
SHEET_Y = 4 * U
FAR = 64 * U           # a move that takes a picker away from everything


def _sheet(dimx, dimz):
    """Flat rest layout, index = row * dimx + column, x along the columns; w = the scene's own 1 / (0.5 / n)."""
    xs = (np.arange(dimx) - (dimx - 1) / 2.0) * SPACING
    zs = (np.arange(dimz) - (dimz - 1) / 2.0) * SPACING
    xx, zz = np.meshgrid(xs, zs)
    p = np.zeros((dimx * dimz, 4), np.float32)
    p[:, 0], p[:, 1], p[:, 2] = xx.ravel(), SHEET_Y, zz.ravel()
    p[:, 3] = np.float32(1.0) / (np.float32(0.5) / np.float32(dimx * dimz))
    return p


def _put(pos, index, centre, offset_u):
    pos[index, :3] = np.asarray(centre, np.float64) + np.asarray(offset_u, np.float64) * U


def _move(targets, grasp, speed=1.0, min_steps=None, steps=1):
    """One movep call.  `steps`: the simulated steps it takes by construction."""
    return dict(targets=np.asarray(targets, np.float64).reshape(-1, 3), grasp=[int(g) for g in grasp], speed=float(speed),
                min_steps=min_steps, steps=int(steps))


def _case(name, rule, dims, pos, centres, program, expected, decoy, why):
    centres = np.asarray(centres, np.float64).reshape(-1, 3)
    expected, decoy = np.asarray(expected, np.int64), np.asarray(decoy, np.int64)
    n_steps = sum(m["steps"] for m in program)
    assert pos.shape == (dims[0] * dims[1], 4) and pos.dtype == np.float32
    assert expected.shape == decoy.shape == (n_steps, len(centres)), name
    assert all(m["targets"].shape == centres.shape and len(m["grasp"]) == len(centres) for m in program), name
    return dict(name=name, rule=rule, why=why, dims=dims, scene_params=cloth_params(dims[0], dims[1], pos=(0.0, 0.2, 0.0)),
                pos=pos, num_picker=len(centres), centres=centres, picker_radius=PICKER_RADIUS, picker_threshold=0.0,
                particle_radius=0.0, program=program, expected_picked=expected, decoy=decoy)


ABOVE = np.array([0.0, 12 * U, 0.0])  # 8U above the middle of the sheet: the rest layout is out of reach (5U)
UP = np.array([0.0, 4 * U, 0.0])


def _tie(name, rule, dims, lo, hi, why):
    pos = _sheet(*dims)
    _put(pos, lo, ABOVE, (3, -4, 0))
    _put(pos, hi, ABOVE, (-3, -4, 0))
    return _case(name, rule, dims, pos, [ABOVE], [_move([ABOVE + UP], [1])], [[lo]], [[hi]], why)


def _corner_scene():
    """16 x 16 sheet, one picker up and out from corner particle 0, which alone is in reach: at exactly (3,-4,0)U = 5U."""
    pos = _sheet(16, 16)
    corner = np.array([-12 * U, SHEET_Y, -12 * U])
    pos[0, :3] = corner
    return pos, corner + np.array([-3 * U, 4 * U, 0.0])


def _ranked(name, rule, dims, n_pickers, indices, why):
    """All pickers on one centre; len(indices) > n_pickers particles at distinct distances (1.6U, 1.8U, ...), nearest first
    in the order of `indices` -- which is not the order of the indices.  Picker k must hold the k-th nearest."""
    pos = _sheet(*dims)
    assert len(indices) > n_pickers and len(set(indices)) == len(indices) and sorted(indices) != list(indices)
    for k, i in enumerate(indices):
        r, th = (1.6 + 0.2 * k) * U, 2.4 * k
        off = np.round(np.array([0.8 * np.cos(th), -0.6, 0.8 * np.sin(th)]) * r * 65536) / 65536  # multiples of 2^-16
        pos[i, :3] = ABOVE + off
    d = np.linalg.norm(pos[list(indices), :3].astype(np.float64) - ABOVE, axis=1)
    assert np.all(np.diff(d) > 0.15 * U) and d[-1] < 4.9 * U
    centres = [ABOVE] * n_pickers
    expected = [list(indices[:n_pickers])]
    decoy = [sorted(indices)[:n_pickers]]  # "picker k takes the k-th lowest index in reach"
    return _case(name, rule, dims, pos, centres, [_move([ABOVE + UP] * n_pickers, [1] * n_pickers)], expected, decoy, why)


def _build():
    cases = []

    # ---- ties: the lowest index wins, in each of the three places the kernel decides it
    cases.append(_tie("tie_same_stride", "ties", (17, 16), 5, 261,
                      "5 and 5 + 256 are visited by the same thread; `<=` in its strided loop would keep the later one"))
    cases.append(_tie("tie_reduce_128", "ties", (16, 16), 3, 131,
                      "3 and 3 + 128 meet in the first level of the LDS tree; taking the upper half on a tie picks 131"))
    cases.append(_tie("tie_reduce_0_255", "ties", (16, 16), 0, 255,
                      "255 travels through every level of the tree before it meets 0"))
    pos = _sheet(17, 16)
    _put(pos, 9, ABOVE, (0, -4, 3))
    _put(pos, 10, ABOVE, (5, 0, 0))
    cases.append(_case("tie_reduce_adjacent", "ties", (17, 16), pos, [ABOVE], [_move([ABOVE + UP], [1])], [[9]], [[10]],
                       "9 and 10 are found by neighbouring threads and meet at the last level (offset 1) of the tree"))

    # ---- nearest beats lowest
    pos = _sheet(17, 16)
    _put(pos, 7, ABOVE, (3, -4, 0))
    _put(pos, 260, ABOVE, (0, -3, 0))
    cases.append(_case("nearest_beats_lowest", "ties", (17, 16), pos, [ABOVE], [_move([ABOVE + UP], [1])], [[260]], [[7]],
                       "the nearest particle sits in the second stride (index >= 256); a kernel that stops at the first hit "
                       "or scans one stride takes 7"))

    # ---- threshold: inclusive, float64 on float32 coordinates
    pos, c = _corner_scene()
    cases.append(_case("threshold_inclusive", "threshold", (16, 16), pos, [c], [_move([c + UP], [1])], [[0]], [[-1]],
                       "the only particle in reach is at exactly the threshold; `<` misses it"))
    pos, c = _corner_scene()
    pos[0, 0] = np.nextafter(pos[0, 0], np.float32(1.0))  # one float32 ulp away from the picker (which is at smaller x)
    pos[16, :3] = [-12 * U, SHEET_Y, -10 * U]
    pos[16, 3] = 0.0  # pinned at reset: stays where it is, (3,-4,0)U from where the picker stands after its first move
    t1 = c + np.array([0.0, 0.0, 2 * U])
    cases.append(_case("threshold_one_ulp_out", "threshold+empty", (16, 16), pos, [c],
                       [_move([t1], [1]), _move([t1 + UP], [1])], [[-1], [16]], [[0], [0]],
                       "particle 0 is one ulp beyond the threshold (float32 squares, or a tolerance on the comparison, "
                       "take it); the empty picker searches again on the next step and finds pinned particle 16 at exactly 5U"))

    # float64 distances: 180 is at (-1,-3,0)U, d^2 = 10 U^2; 50 is one float32 ulp of x farther out, d^2 = (10 + 2^-22) U^2.
    # In float32 the extra quarter ulp of the sum is rounded away, the two tie and the lower index wins.
    pos = _sheet(16, 16)
    _put(pos, 180, ABOVE, (-1, -3, 0))
    _put(pos, 50, ABOVE, (1, -3, 0))
    pos[50, 0] = np.nextafter(pos[50, 0], np.float32(1.0))
    cases.append(_case("float64_distance", "threshold", (16, 16), pos, [ABOVE], [_move([ABOVE + UP], [1])], [[180]], [[50]],
                       "the nearer particle is nearer by less than float32 arithmetic resolves; distances in float32 tie and "
                       "give the lower index"))

    # ---- contention
    pos = _sheet(16, 16)
    _put(pos, 120, ABOVE, (0, -3, 0))
    _put(pos, 40, ABOVE, (3, -4, 0))
    cases.append(_case("contention_two", "held", (16, 16), pos, [ABOVE, ABOVE], [_move([ABOVE + UP] * 2, [1, 1])],
                       [[120, 40]], [[120, 120]], "picker 1 must skip the particle picker 0 took in this very step"))
    pos = _sheet(16, 16)
    _put(pos, 120, ABOVE, (0, -3, 0))
    cases.append(_case("contention_one", "held+empty", (16, 16), pos, [ABOVE, ABOVE],
                       [_move([ABOVE + UP, ABOVE + [0, FAR, 0]], [1, 1]), _move([ABOVE + 2 * UP, ABOVE + [0, FAR, 4 * U]], [1, 1])],
                       [[120, -1], [120, -1]], [[120, 120], [120, 120]],
                       "one particle, two pickers: the second finds nothing, stays empty and still finds nothing a step later"))

    # ---- taken earlier in the step, and already moved in place
    pos = _sheet(16, 16)
    c0, c1 = ABOVE + [-8 * U, 0, 0], ABOVE + [8 * U, 0, 0]
    _put(pos, 100, c0, (0, -3, 0))   # A: picker 0's; its move (+16U in x) carries it to 3U below picker 1
    _put(pos, 140, c1, (3, -4, 0))   # B: in picker 1's reach, farther than the moved A
    cases.append(_case("taken_then_moved", "held", (16, 16), pos, [c0, c1], [_move([c0 + [16 * U, 0, 0], c1 + UP], [1, 1])],
                       [[100, 140]], [[100, 100]],
                       "the kernel moves A in place before picker 1 searches: A is now nearest to picker 1 and only the "
                       "held test keeps it from being taken twice"))

    # ---- released and re-taken in one step
    pos = _sheet(16, 16)
    c0, c1 = ABOVE + [-8 * U, 0, 0], ABOVE + [8 * U, 0, 0]
    _put(pos, 100, c0, (0, -3, 0))
    # step 1 carries A to c0 + (13,-3,0)U = c1 + (-3,-3,0)U and picker 1 (not grasping) to c1 + (0,-1,0)U: A is then at
    # (-3,-2,0)U from picker 1, |.|^2 = 13 U^2, in reach; held (w = 0), so the solver leaves it there
    t0, t1 = c0 + [13 * U, 0, 0], c1 + [0, -1 * U, 0]
    cases.append(_case("release_and_retake", "held", (16, 16), pos, [c0, c1],
                       [_move([t0, t1], [1, 0]), _move([t0 + UP, t1 + UP], [0, 1])],
                       [[100, -1], [-1, 100]], [[100, -1], [-1, -1]],
                       "picker 0 lets go of A in the step in which the empty picker 1 searches next to it: a held test "
                       "against the list as it was at entry would leave A free"))

    # ---- inverse masses: every particle its own; a pinned one can be grasped; release restores the particle's own bits
    pos = _sheet(17, 16)
    pos[:, 3] = (pos[:, 3] * (np.float32(1.0) + np.arange(272, dtype=np.float32) / np.float32(1024.0))).astype(np.float32)
    c0, c1 = ABOVE + [-8 * U, 0, 0], ABOVE + [8 * U, 0, 0]
    _put(pos, 30, c0, (0, -4, 3))
    pos[30, 3] = 0.0                    # pinned at reset
    _put(pos, 31, c0, (0, -3, 0))
    pos[31, 3] = 0.0                    # pinned too, nearer: taken by picker 0; 30 stays where it is
    _put(pos, 262, c1, (0, -3, 0))      # free, index >= 256, w = w0 * (1 + 262 / 1024)
    cases.append(_case("inverse_masses", "unpick", (17, 16), pos, [c0, c1],
                       [_move([c0 + UP, c1 + UP], [1, 1]), _move([c0 + 2 * UP, c1 + 2 * UP], [0, 0])],
                       [[31, 262], [-1, -1]], [[-1, 262], [-1, -1]],
                       "a pinned particle (w = 0) is a candidate like any other; the release writes back saved_w[31] = 0 and "
                       "saved_w[262], not a common value or another particle's"))

    # ---- release while standing: a movep onto the current centres takes no simulated step and so releases nothing
    pos = _sheet(16, 16)
    _put(pos, 77, ABOVE, (0, -3, 0))
    t = ABOVE + 2 * UP                  # A is carried to t + (0,-3,0)U
    _put(pos, 78, t, (0, -2, 0))        # B pinned, 6U from ABOVE (out of reach at step 1), 2U from t: nearer than A
    pos[78, 3] = 0.0
    cases.append(_case("release_while_standing", "unpick", (16, 16), pos, [ABOVE],
                       [_move([t], [1]), _move([t], [0], min_steps=3, steps=0), _move([t + UP], [1])],
                       [[77], [77]], [[77], [78]],
                       "the standing movep (4 iterations, no step) must not release A: had it, the next search would take the "
                       "nearer pinned B"))

    # ---- teleport association: full-mantissa coordinates, (p + new) - old in float32, left to right
    rng = np.random.RandomState(5)
    pos = _sheet(16, 16)
    c = (ABOVE + rng.uniform(-0.3, 0.3, 3) * U).astype(np.float32).astype(np.float64)
    pos[90, :3] = c + rng.uniform(-1.0, 1.0, 3) * 2.5 * U      # within 4.4U
    pos[20, :3] = c + np.array([0.0, -4.7 * U, 0.3 * U])       # lower index, in reach, farther
    prog, cur = [], c
    for _ in range(6):
        cur = cur + rng.uniform(-1.0, 1.0, 3) * 3 * U + [0, 1.5 * U, 0]
        prog.append(_move([cur], [1]))
    cases.append(_case("teleport_association", "teleport", (16, 16), pos, [c], prog, [[90]] * 6, [[20]] * 6,
                       "off-lattice coordinates: p + (new - old) differs from (p + new) - old in the last bit on some step"))

    # ---- small sets: fewer particles than threads, fewer than pickers
    pos = _sheet(1, 1)
    pos[0, :3] = [0.0, SHEET_Y, 0.0]
    c = pos[0, :3].astype(np.float64) + np.array([0, 4, 3]) * U
    cases.append(_case("small_1x1", "counts", (1, 1), pos.copy(), [c], [_move([c + UP], [1])], [[0]], [[-1]],
                       "n = 1: 255 threads have nothing to offer to the reduction"))
    cases.append(_case("small_1x1_two_pickers", "counts+held", (1, 1), pos.copy(), [c, c], [_move([c + UP] * 2, [1, 1])],
                       [[0, -1]], [[0, 0]], "more pickers than particles: the second stays empty"))
    pos = _sheet(2, 1)
    pos[0, :3], pos[1, :3] = [-1 * U, SHEET_Y, 0.0], [1 * U, SHEET_Y, 0.0]
    c = np.array([1 * U, SHEET_Y + 3 * U, 0.0])
    cases.append(_case("small_2x1", "counts", (2, 1), pos, [c], [_move([c + UP], [1])], [[1]], [[0]],
                       "n = 2: the nearer particle has the higher index"))
    pos = _sheet(3, 2)
    for i in range(6):
        pos[i, :3] = [(i % 3 - 1) * 2 * U, SHEET_Y, (i // 3) * 2 * U - U]
    c = pos[4, :3].astype(np.float64) + np.array([0, 3, 0]) * U
    cases.append(_case("small_3x2", "counts", (3, 2), pos, [c], [_move([c + UP], [1])], [[4]], [[0]],
                       "n = 6: all six in reach, the nearest is not the first"))

    # ---- picker counts other than 2
    cases.append(_ranked("pickers_3", "counts+held", (16, 16), 3, [200, 17, 90, 3],
                         "three pickers on one centre take the three nearest, nearest first"))
    cases.append(_ranked("pickers_4", "counts+held", (17, 16), 4, [270, 8, 259, 100, 2],
                         "four pickers, candidates on both sides of index 256"))
    cases.append(_ranked("pickers_16", "counts+held", (17, 16), 16,
                         [271, 3, 256, 130, 15, 264, 77, 0, 200, 258, 31, 129, 268, 64, 1, 255, 16],
                         "FS_MAX_SHAPES pickers on one centre, 17 candidates: picker k holds the k-th nearest"))
    return cases


CASES = _build()
BY_NAME = {c["name"]: c for c in CASES}

# every rule of the grasp search, and the cases that pin it
RULES = {
    "ties": ["tie_same_stride", "tie_reduce_128", "tie_reduce_0_255", "tie_reduce_adjacent", "nearest_beats_lowest"],
    "threshold": ["threshold_inclusive", "threshold_one_ulp_out", "float64_distance"],
    "held exclusion": ["contention_two", "contention_one", "taken_then_moved", "release_and_retake", "small_1x1_two_pickers"],
    "empty search": ["threshold_one_ulp_out", "contention_one"],
    "un-pick": ["inverse_masses", "release_while_standing"],
    "teleport": ["teleport_association"],
    "particle counts": ["small_1x1", "small_1x1_two_pickers", "small_2x1", "small_3x2", "tie_reduce_0_255", "tie_same_stride"],
    "picker counts": ["small_1x1", "pickers_3", "pickers_4", "pickers_16"],
}


def step_after_call(case):
    """For every movep of the program: how many simulated steps have been taken once it returns."""
    return np.cumsum([m["steps"] for m in case["program"]])


def setup(sim, case):
    """Bring a pyflex-shaped `sim` (OracleSim, EnvView, the reference's stub) to the case's start, pickers excluded."""
    sim.set_scene(case["scene_params"])
    sim.step(1)
    sim.set_positions(case["pos"].ravel())
    sim.set_velocities(np.zeros(3 * case["pos"].shape[0], np.float32))


def set_centres(sim, case):
    """What follows Picker.reset: the spheres exist; their current and previous positions become the case's centres."""
    st = np.array(sim.get_shape_states()).reshape(-1, 14)
    for i, c in enumerate(case["centres"]):
        st[i] = np.hstack([c, c, [1, 0, 0, 0], [1, 0, 0, 0]])
    sim.set_shape_states(st)
