"""Constructed particle sets for the episode-steering kernels of flingbot_amd/csrc/fs_loops.hip: fs_k_cloth_stats,
fs_k_stretch_probe, fs_k_max_displacement, fs_k_stable_check (and the same rule in fs_k_wait_check, fs_picker.hip) and
fs_k_set_particles.

Plain numpy, importable without a GPU.  Every case has a `name`, an `op` (stats / probe / disp / stable), a `rule` (what it
pins), a `why`, its inputs and its `decoy`s: the named mistakes a plausibly wrong kernel makes that this very case notices.
The names are the mutation switches of the restatements below; tests/test_steering_edges_cpu.py asserts that every named
decoy changes the case's expected output and that every mutation is named somewhere.  Inputs are float32 positions [n, 4]
(`pos`), velocities [n, 3] (`vel`) and per operation: `mid` (float32[2]) and `thr` (float32) for the probe, `pre` (the
snapshot, float32[n, 4]) for the displacement, `tol` (a Python float) and `max_steps` for the stable check.  `at` is the
index of the particle that decides the case, where one does.

The restatements are the reference's expressions one element at a time, in float32, with no library reduction:
    stats   (y.min(), y.max(), np.abs(v).max())                      numpy's min / max hand a NaN on
    probe   high = pos[y > thr];  single = (high.x < 0).all() or (high.x > 0).all();  nearest = the FIRST index of the
            minimum of sqrt(dx * dx + dz * dz): the reference sorts a list with Python's stable sort (simEnv.py:155-168)
    disp    max_i sqrt((dx * dx + dy * dy) + dz * dz) of |post - pre| (simEnv.py:470-472)
    stable  float(m) < float(tol) before the step, m = the stats velocity maximum (flex_utils.py:430-441 under NumPy 1.x)
Expected values are not stored in the table: they are what the unmutated restatement returns, and the CPU test ties the
restatement to the vectorised numpy expressions of tests/fling_helpers.py and to a float64 evaluation.

All coordinates of the lattice cases are small multiples of a power of two, so every difference, square and sum that decides
a case is exact in float32 (and therefore the same whether or not a compiler fuses the sum).

Where this table departs from the list it was written from: `tail_dropped` is two switches, `tail_dropped` (the tail beyond
a multiple of 64) and `tail_dropped_block` (beyond a multiple of 256); `component_dropped` is three, one per component, so
that each of the x, y and z cases names the switch that it alone notices; `nan_is_high` (`!(y <= thr)` for `y > thr`) and
`thr_ignored` (every particle counts as high) were added for the probe; `disp_abs_missing` is carried by the restatement
but is no mistake (EQUIVALENT_MUTATIONS).
"""
import numpy as np

from coverage_cases import grid_for  # noqa: F401  (re-exported: the GPU test builds every set on grid_for(n))

F = np.float32
COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1025)
BIG = 16512                     # above the snapshot buffer's first capacity (16384 particles): the regrow path
FLT_MAX = F(3.4028234663852886e38)
MUTATIONS = ("tail_dropped", "tail_dropped_block", "first_block_only", "first_wave_only", "abs_missing",
             "component_dropped_x", "component_dropped_y", "component_dropped_z", "max_init_zero", "min_init_zero",
             "fmax_drops_nan", "zero_is_negative", "zero_is_positive", "thr_inclusive", "nan_is_high", "thr_ignored",
             "tie_by_thread", "tie_last", "dist_3d", "other_slot_params", "ids_ignored", "squared_returned", "l1_norm",
             "disp_abs_missing", "compare_in_f32")
# disp_abs_missing (post - pre without the np.abs) is no mistake: IEEE multiplication gives (-d) * (-d) == d * d bit for
# bit, NaN included, so the norm cannot see the sign.  tests/test_steering_edges_cpu.py asserts that equality on the table.
EQUIVALENT_MUTATIONS = ("disp_abs_missing",)
PLACEMENT = ("tail_dropped", "tail_dropped_block", "first_block_only", "first_wave_only")
# One call over episodes of different sizes, listed out of order: row k belongs to episode BATCH_ORDER[k].
BATCH_SIZES = (2, 257, 64, 1025)
BATCH_ORDER = (2, 0, 3, 1)
BATCH_DECOYS = ("other_slot_params", "ids_ignored")


# ---------------------------------------------------------------------------------------------------------------------
# restatements
def _limit(n, mut):
    """How many particles a kernel with the placement mistakes in `mut` looks at."""
    lim = n
    if "tail_dropped" in mut:
        lim = min(lim, n // 64 * 64)
    if "tail_dropped_block" in mut:
        lim = min(lim, n // 256 * 256)
    if "first_block_only" in mut:
        lim = min(lim, 256)
    if "first_wave_only" in mut:
        lim = min(lim, 64)
    return lim


def _nanmax(m, v, mut):
    """np.max's step: a NaN on either side is the result (`fmax_drops_nan`: C's fmax, which returns the other operand)."""
    if "fmax_drops_nan" in mut:
        return m if v != v else (v if m != m else (v if v > m else m))
    return m if m != m else (v if (v != v or v > m) else m)


def stats(pos, vel, mut=()):
    """(min height, max height, max |velocity component|) as float32 scalars."""
    assert all(m in MUTATIONS for m in mut) and pos.dtype == F and vel.dtype == F
    lim = _limit(pos.shape[0], mut)
    lo = F(0) if "min_init_zero" in mut else None
    hi = F(0) if "max_init_zero" in mut else None
    vm = None
    comps = [c for c, k in enumerate("xyz") if f"component_dropped_{k}" not in mut]
    for i in range(lim):
        y = pos[i, 1]
        lo = y if lo is None else -_nanmax(-lo, -y, mut)
        hi = y if hi is None else _nanmax(hi, y, mut)
        for c in comps:
            a = vel[i, c] if "abs_missing" in mut else (-vel[i, c] if vel[i, c] < 0 else vel[i, c])
            a = a + F(0) if a == 0 else a                       # |-0.0| is +0.0
            vm = a if vm is None else _nanmax(vm, a, mut)
    if lim == 0:                                                # nothing looked at: what a kernel starts from
        lo, hi, vm = FLT_MAX, -FLT_MAX, F(0)
    return F(lo), F(hi), F(vm)


def distances(pos, mid, mut=(), reading="f32"):
    """The probe's distance of every particle from `mid` on the ground plane, in one of three readings: "f32" (every product
    and the sum rounded to float32: numpy elementwise and the kernel), "fused" (float32 inputs, one rounding of the exact sum
    of squares, then a float32 sqrt: what a dot product with fused multiply-adds may give) and "f64"."""
    out = []
    for i in range(pos.shape[0]):
        if reading == "f32":
            dx, dz = F(pos[i, 0] - mid[0]), F(pos[i, 2] - mid[1])
            s = F(F(dx * dx) + F(dz * dz))
            if "dist_3d" in mut:
                s = F(s + F(pos[i, 1] * pos[i, 1]))
            out.append(F(np.sqrt(s)))
        elif reading == "fused":
            dx, dz = float(F(pos[i, 0] - mid[0])), float(F(pos[i, 2] - mid[1]))
            out.append(F(np.sqrt(F(dx * dx + dz * dz))))        # float64 holds the sum of two float32 squares to 2^-53
        else:
            dx, dz = float(pos[i, 0]) - float(mid[0]), float(pos[i, 2]) - float(mid[1])
            out.append(np.sqrt(dx * dx + dz * dz))
    return out


def probe(pos, mid, thr, mut=(), reading="f32"):
    """(single grasp, index of the nearest particle)."""
    assert all(m in MUTATIONS for m in mut) and pos.dtype == F
    n = pos.shape[0]
    lim = _limit(n, mut)
    all_neg = all_pos = True
    for i in range(lim):
        y, x = pos[i, 1], pos[i, 0]
        high = (y >= thr) if "thr_inclusive" in mut else (y > thr)
        if "nan_is_high" in mut:
            high = not (y <= thr)
        if "thr_ignored" in mut:
            high = True
        if high:
            all_neg = all_neg and bool((x <= 0) if "zero_is_negative" in mut else (x < 0))
            all_pos = all_pos and bool((x >= 0) if "zero_is_positive" in mut else (x > 0))
    d = distances(pos, mid, mut, reading)
    best = None
    for i in range(lim):
        if best is None or d[i] < d[best]:
            best = i
        elif d[i] == d[best]:
            if "tie_last" in mut or ("tie_by_thread" in mut and i % 256 < best % 256):
                best = i
    return bool(all_neg or all_pos), (0 if best is None else best)


def displacement(pos, pre, mut=()):
    """max_i || |post_i - pre_i| ||_2 as a float32 scalar."""
    assert all(m in MUTATIONS for m in mut) and pos.dtype == F and pre.dtype == F
    lim = _limit(pos.shape[0], mut)
    m = None
    for i in range(lim):
        d = [F(pos[i, c] - pre[i, c]) for c in range(3)]
        if "disp_abs_missing" not in mut:
            d = [(-x if x < 0 else x) for x in d]
        if "l1_norm" in mut:
            v = F(F(d[0] + d[1]) + d[2])
        else:
            s = F(F(F(d[0] * d[0]) + F(d[1] * d[1])) + F(d[2] * d[2]))
            v = s if "squared_returned" in mut else F(np.sqrt(s))
        m = v if m is None else _nanmax(m, v, mut)
    return F(0) if m is None else F(m)


def stable(vel, tol, max_steps, mut=()):
    """wait_until_stable with max_steps <= 1 -> (stable, steps): the test comes before the step."""
    assert max_steps in (0, 1) and all(m in MUTATIONS for m in mut)
    if max_steps == 0:
        return False, 0
    m = stats(np.zeros((vel.shape[0], 4), F), vel, mut)[2]
    ok = bool(F(m) < F(tol)) if "compare_in_f32" in mut else (float(m) < float(tol))
    return (True, 0) if ok else (False, 1)


def batch(fn, episodes, ids, args, mut=()):
    """One call over the episodes ids[k] with per-slot arguments args[k]: row k = fn(episodes[ids[k]], *args[k])."""
    rows = []
    for k, e in enumerate(ids):
        ep = episodes[k if "ids_ignored" in mut else e]
        rows.append(fn(ep, *(args[0] if "other_slot_params" in mut else args[k])))
    return rows


def set_particle(pos, vel, pid, pos4, zero_velocity):
    """fs_set_particles on one episode -> (pos, vel): position and w of one particle, its velocity optionally zeroed."""
    pos, vel = pos.copy(), vel.copy()
    assert 0 <= pid < pos.shape[0]
    for c in range(4):
        pos[pid, c] = F(pos4[c])
    if zero_velocity:
        for c in range(3):
            vel[pid, c] = F(0)
    return pos, vel


# ---------------------------------------------------------------------------------------------------------------------
# the table
def placements(n):
    """Where the decisive particle sits: the first and last lane of a wave and of a block, the last index, 256 k + 255."""
    idx = {0, 63, 64, 255, 256, n - 1} | {256 * k + 255 for k in range(n // 256 + 1)}
    return sorted(i for i in idx if 0 <= i < n)


def placement_decoys(n, at):
    """The placement mistakes that do not look at index `at` of n particles."""
    return tuple(m for m in PLACEMENT if _limit(n, (m,)) <= at)


def base(n):
    """n particles on a lattice: heights in (0.125, 0.15), x and z on both sides of 0 (multiples of 2^-6), velocity components
    of both signs, multiples of 2^-5 up to 0.125; w = 1."""
    i = np.arange(n)
    p = np.ones((n, 4), F)
    p[:, 0] = (((5 * i) % 17) - 8) * 2.0 ** -6
    p[:, 1] = 0.125 + (((7 * i) % 11) + 1) * 2.0 ** -9
    p[:, 2] = (((3 * i) % 13) - 6) * 2.0 ** -6
    v = np.empty((n, 3), F)
    v[:, 0] = (((3 * i) % 7) - 3) * 2.0 ** -5
    v[:, 1] = (((5 * i) % 9) - 4) * 2.0 ** -5
    v[:, 2] = (((2 * i) % 5) - 2) * 2.0 ** -5
    return p, v


def far(n, mid):
    """n particles at least 1.5 m from `mid` on the ground plane, all with x > 0 and below every probe threshold: the probe
    cases put their few deciding particles into this set."""
    i = np.arange(n)
    p = np.ones((n, 4), F)
    p[:, 0] = float(mid[0]) + 1.5 + i * 2.0 ** -10
    p[:, 1] = 0.03125 + ((7 * i) % 11) * 2.0 ** -9
    p[:, 2] = float(mid[1]) + (((37 * i) % 64) - 32) * 2.0 ** -8
    return p


def _case(name, op, rule, why, decoy=(), **kw):
    assert all(d in MUTATIONS and d not in EQUIVALENT_MUTATIONS for d in decoy), name
    for k in ("pos", "vel", "pre"):
        if k in kw:
            kw[k] = np.ascontiguousarray(kw[k], F)
            assert kw[k].shape == (kw["pos"].shape[0], 3 if k == "vel" else 4), (name, k)
    if "mid" in kw:
        kw["mid"], kw["thr"] = np.asarray(kw["mid"], F), F(kw["thr"])
    return dict(name=name, op=op, rule=rule, why=why, decoy=tuple(dict.fromkeys(decoy)), n=kw["pos"].shape[0], **kw)


def _stats_cases():
    out = []
    for n in COUNTS:
        for at in placements(n):
            for q, y in (("min", -0.0625), ("max", 0.75)):
                p, v = base(n)
                c = (at + (q == "max")) % 3
                p[at, 1] = y
                v[at, c] = -0.75 if q == "min" else 0.75
                dec = placement_decoys(n, at) + (f"component_dropped_{'xyz'[c]}",) + (("abs_missing",) if q == "min" else ())
                out.append(_case(f"stats_{q}_n{n}_at{at}", "stats", "placement",
                                 f"index {at} of {n} alone has the {q} height {y} and the velocity {'xyz'[c]} = {v[at, c]}; every "
                                 "other height lies in (0.125, 0.15), every other |velocity| is at most 0.125",
                                 dec, pos=p, vel=v, at=at))
    for c, k in enumerate("xyz"):                               # the extreme velocity negative, in each component
        p, v = base(257)
        v[256, c] = -0.5
        out.append(_case(f"stats_velocity_negative_{k}", "stats", "abs",
                         f"the largest |velocity| is {k} = -0.5 at the last index of 257; the largest positive component is 0.125",
                         ("abs_missing", f"component_dropped_{k}") + placement_decoys(257, 256), pos=p, vel=v, at=256))
    p, v = base(65)
    p[:, 1] = -p[:, 1]
    out.append(_case("stats_all_heights_negative", "stats", "initial values", "every height lies in (-0.15, -0.125): a maximum started "
                     "at 0 stays 0", ("max_init_zero",), pos=p, vel=v))
    p, v = base(65)
    p[:, 1] += F(1.0)
    out.append(_case("stats_all_heights_above_one", "stats", "initial values", "every height lies in (1.125, 1.15): a minimum started at "
                     "0 stays 0", ("min_init_zero",), pos=p, vel=v))
    p, v = base(65)
    v[:] = 0.0
    v[::3] = -0.0
    out.append(_case("stats_zero_velocities", "stats", "initial values", "every velocity is +0.0 or -0.0: the maximum is 0.0", (), pos=p, vel=v))
    p, v = base(1)
    p[0, 1], v[0] = -0.25, (-0.5, 0.25, 0.125)
    out.append(_case("stats_one_particle", "stats", "initial values", "n = 1, a negative height, the largest |velocity| negative",
                     ("abs_missing", "max_init_zero", "component_dropped_x"), pos=p, vel=v, at=0))
    for k, n in enumerate(BATCH_SIZES):                         # the batch: every episode has its own three values
        p, v = base(n)
        p[:, 1] += F(k * 2.0 ** -4)
        v[n - 1, k % 3] = -(0.5 + k * 2.0 ** -4)
        out.append(_case(f"stats_batch_n{n}", "stats", "batch", f"n = {n}: heights raised by {k} / 16, the largest |velocity| "
                         f"{0.5 + k / 16} at the last index", placement_decoys(n, n - 1), pos=p, vel=v, at=n - 1))
    for at in (0, 257, 512):                                    # NaN: the affected output is NaN, the others are not
        p, v = base(513)
        p[at, 1] = np.nan
        out.append(_case(f"stats_nan_height_at{at}", "stats", "nan", f"the height of index {at} of 513 is NaN: min and max are NaN, the "
                         "velocity maximum is untouched", ("fmax_drops_nan",), pos=p, vel=v, at=at))
        p, v = base(513)
        v[at, at % 3] = np.nan
        out.append(_case(f"stats_nan_velocity_at{at}", "stats", "nan", f"one velocity component of index {at} of 513 is NaN: the velocity "
                         "maximum is NaN, min and max height are untouched", ("fmax_drops_nan",), pos=p, vel=v, at=at))
    return out


def _put(p, i, mid, ax, az, y=None, x=None):
    """Particle i at mid + (ax, az) * 2^-8 on the ground plane (or at x), optionally at height y."""
    p[i, 0] = F(mid[0]) + F(ax * 2.0 ** -8) if x is None else x
    p[i, 2] = F(mid[1]) + F(az * 2.0 ** -8)
    if y is not None:
        p[i, 1] = y


def _probe_cases():
    out = []
    mid, thr, n = (0.5, 0.25), 0.25, 513
    up = 0.5                                                    # a height above the threshold

    def single(name, why, xs, decoy=(), extra=None, n=n, thr=thr):
        """`xs`: index -> x of the high particles (x about 0.5 m from mid: never the nearest); index 40 is the nearest."""
        p = far(n, mid)
        _put(p, min(40, n - 1), mid, 1, 2)
        for i, x in xs.items():
            _put(p, i, mid, 0, 3 + (i % 5), y=up, x=x)
        if extra:
            extra(p)
        out.append(_case(name, "probe", "single grasp", why, decoy, pos=p, vel=base(n)[1], mid=mid, thr=thr,
                         at=min(40, n - 1), tie=()))

    single("probe_all_negative", "the four high particles all have x < 0 (every low particle has x > 0): single",
           {5: -0.01, 70: -0.02, 300: -0.015, 512: -0.03}, ("thr_ignored",))
    single("probe_all_positive", "the four high particles all have x > 0: single", {5: 0.01, 70: 0.02, 300: 0.015, 512: 0.03})
    single("probe_mixed", "high particles on both sides: not single", {5: -0.01, 70: 0.02, 300: -0.015, 512: 0.03})
    single("probe_dissenter_last", "the one high particle with x > 0 is the last index: not single",
           {5: -0.01, 20: -0.02, 50: -0.015, 512: 0.03}, placement_decoys(n, 512))
    single("probe_dissenter_beyond_256", "the one high particle with x > 0 is index 300, the others lie below 64: not single",
           {5: -0.01, 20: -0.02, 50: -0.015, 300: 0.03}, placement_decoys(n, 300))
    for zname, zero in (("plus", 0.0), ("minus", -0.0)):
        single(f"probe_zero_{zname}_among_negative", f"one high particle at x == {zero!r} among high particles with x < 0: neither "
               "all x < 0 nor all x > 0", {5: -0.01, 70: zero, 300: -0.015}, ("zero_is_negative",))
        single(f"probe_zero_{zname}_among_positive", f"one high particle at x == {zero!r} among high particles with x > 0: not single",
               {5: 0.01, 70: zero, 300: 0.015}, ("zero_is_positive",))
    single("probe_on_threshold", "a particle with x > 0 at exactly y == thr is not high; the high ones have x < 0: single",
           {5: -0.01, 70: -0.02}, ("thr_inclusive",), lambda p: _put(p, 300, mid, 0, 4, y=F(thr), x=0.03))
    single("probe_just_below_threshold", "the particle with x > 0 lies one float32 below thr: single",
           {5: -0.01, 70: -0.02}, (), lambda p: _put(p, 300, mid, 0, 4, y=np.nextafter(F(thr), F(0)), x=0.03))
    single("probe_just_above_threshold", "the particle with x > 0 lies one float32 above thr: not single",
           {5: -0.01, 70: -0.02}, (), lambda p: _put(p, 300, mid, 0, 4, y=np.nextafter(F(thr), F(1)), x=0.03))
    single("probe_none_high", "no particle above thr = 10: (empty).all() is True, single", {5: -0.01, 70: 0.02}, (), thr=10.0)
    single("probe_nan_height", "a particle with x > 0 and a NaN height is not high (NaN > thr is False); the nearest particle is "
           "what it is without it", {5: -0.01, 70: -0.02}, ("nan_is_high",), lambda p: _put(p, 300, mid, 0, 4, y=np.nan, x=0.03))

    def nearest(name, why, puts, at, decoy=(), tie=(), n=n, mid=mid, thr=thr):
        p = far(n, mid)
        for i, (ax, az, y) in puts.items():
            _put(p, i, mid, ax, az, y=y)
        out.append(_case(name, "probe", "nearest", why, decoy, pos=p, vel=base(n)[1], mid=mid, thr=thr, at=at, tie=tuple(tie)))

    nearest("probe_tie_1_256", "indices 1 and 256 (threads 1 and 0) are both 5 * 2^-8 from mid, at (3, 4) and (-5, 0): index 1",
            {1: (3, 4, None), 256: (-5, 0, None)}, 1, ("tie_by_thread", "tie_last"), (1, 256))
    nearest("probe_tie_3_259", "indices 3 and 259 (both thread 3) tie at (0, 5) and (4, -3): index 3",
            {3: (0, 5, None), 259: (4, -3, None)}, 3, ("tie_last",), (3, 259))
    nearest("probe_tie_four", "indices 7, 130, 258 and 512 tie at (3, 4), (-4, 3), (5, 0), (0, -5): the lowest index",
            {7: (3, 4, None), 130: (-4, 3, None), 258: (5, 0, None), 512: (0, -5, None)}, 7, ("tie_by_thread", "tie_last"),
            (7, 130, 258, 512))
    nearest("probe_distance_ignores_height", "index 300 is 4 * 2^-8 from mid at height 0.75, index 10 is 8 * 2^-8 away at height 0: "
            "nearer in 3-D, farther on the ground plane", {300: (4, 0, 0.75), 10: (8, 0, 0.0)}, 300,
            ("dist_3d",) + placement_decoys(n, 300), thr=1.0)
    nearest("probe_winner_last", "the nearest particle is the last index", {512: (1, 0, None), 10: (2, 0, None)}, 512,
            placement_decoys(n, 512))
    nearest("probe_one_particle", "n = 1", {0: (3, -2, None)}, 0, n=1)
    # the batch: four sizes, each with its own midpoint (the corners of a 4 m square) and threshold.  The last index sits
    # next to the episode's own midpoint and is its only particle above its own threshold; index 0 sits next to the origin,
    # on the other side of x = 0, at height 0.1875: above the lowest threshold of the four only.  With another episode's
    # midpoint the last index is 4 m away and index 0 nearer; with the lowest threshold index 0 is high and dissents.
    for n_b, mid_b, thr_b in zip(BATCH_SIZES, ((2.0, 2.0), (-2.0, 2.0), (2.0, -2.0), (-2.0, -2.0)), (0.25, 0.375, 0.125, 0.5)):
        p = far(n_b, mid_b)
        p[:, 0] = np.copysign(p[:, 0], mid_b[0])
        _put(p, n_b - 1, mid_b, 1, 1, y=thr_b + 0.0625)
        p[0, :3] = (-np.sign(mid_b[0]) * 0.03125, 0.1875, 0.0)
        out.append(_case(f"probe_batch_n{n_b}", "probe", "batch", f"n = {n_b}, mid {mid_b}, thr {thr_b}: the last index is nearest "
                         "and alone above the threshold", (), pos=p, vel=base(n_b)[1], mid=mid_b, thr=thr_b, at=n_b - 1, tie=()))
    return out


def _moved(n, at, move):
    """(pre, post): every particle moves by a small multiple of 2^-10 per axis, index `at` by `move` (multiples of 2^-7)."""
    pre = base(n)[0]
    i = np.arange(n)
    post = pre.copy()
    post[:, 0] += ((i % 5) - 2) * F(2.0 ** -10)
    post[:, 1] += (((3 * i) % 7) - 3) * F(2.0 ** -10)
    post[:, 2] += (((2 * i) % 3) - 1) * F(2.0 ** -10)
    if at is not None:
        post[at, :3] = pre[at, :3] + np.asarray(move, F) * F(2.0 ** -7)
    return pre, post


def _disp_cases():
    out = []
    for n in COUNTS + (BIG,):
        for at in (placements(n) if n != BIG else [n - 1]):
            pre, post = _moved(n, at, (-8, 12, -24))
            out.append(_case(f"disp_n{n}_at{at}", "disp", "placement" if n != BIG else "regrow",
                             f"index {at} of {n} moves by (-8, 12, -24) * 2^-7, length 28 * 2^-7 exactly; no other particle moves "
                             "more than 4 * 2^-10", placement_decoys(n, at) + ("squared_returned", "l1_norm"),
                             pos=post, pre=pre, vel=base(n)[1], at=at, exact=28 * 2.0 ** -7))
    for name, move, length in (("disp_quadruple_3", (1, -2, 2), 3), ("disp_quadruple_7", (-2, 3, -6), 7)):
        pre, post = _moved(65, 20, move)
        post[np.arange(65) != 20] = pre[np.arange(65) != 20]
        out.append(_case(name, "disp", "values", f"one particle moves by {move} * 2^-7, signs mixed: {length} * 2^-7 exactly",
                         ("squared_returned", "l1_norm"), pos=post, pre=pre, vel=base(65)[1], at=20, exact=length * 2.0 ** -7))
    for k, n in enumerate(BATCH_SIZES):                         # the batch: every episode has its own snapshot and length
        pre, post = _moved(n, n - 1, (-2 * (k + 1), 3 * (k + 1), -6 * (k + 1)))
        pre[:, :3] += F(k * 2.0 ** -3)
        post[:, :3] += F(k * 2.0 ** -3)
        out.append(_case(f"disp_batch_n{n}", "disp", "batch", f"n = {n}: everything shifted by {k} / 8, the last index moves by "
                         f"{7 * (k + 1)} * 2^-7", placement_decoys(n, n - 1), pos=post, pre=pre, vel=base(n)[1], at=n - 1,
                         exact=7 * (k + 1) * 2.0 ** -7))
    pre, post = _moved(65, None, None)
    out.append(_case("disp_nothing_moved", "disp", "values", "post == pre bit for bit: 0.0", (), pos=pre.copy(), pre=pre,
                     vel=base(65)[1], exact=0.0))
    rs = np.random.RandomState(20)
    pre = np.ones((1025, 4), F)
    pre[:, :3] = (rs.rand(1025, 3) * (0.6, 0.3, 0.4) - (0.3, 0.0, 0.2)).astype(F)
    post = pre.copy()
    post[:, :3] += (rs.randn(1025, 3) * 0.02).astype(F)
    out.append(_case("disp_cloud", "disp", "values", "1025 seeded particles, each moved by a normal step of 2 cm per axis: the "
                     "kernel equals the float32 elementwise expression bit for bit", ("squared_returned", "l1_norm"),
                     pos=post, pre=pre, vel=base(1025)[1]))
    for at in (0, 257, 512):
        pre, post = _moved(513, 300, (-8, 12, -24))
        pre[at, at % 3] = np.nan
        out.append(_case(f"disp_nan_snapshot_at{at}", "disp", "nan", f"the snapshot of index {at} of 513 holds one NaN coordinate: NaN",
                         ("fmax_drops_nan",), pos=post, pre=pre, vel=base(513)[1], at=at))
    return out


TOL = 1e-2
T32 = F(TOL)                    # float32(0.01) = 0.00999999977648...: below 1e-2 as a double, equal to it as a float32


def _stable_cases():
    """Velocities only: the positions are the ones set_scene gives a grid_for(n) cloth, which the unstable cases step once."""
    out = []

    def add(name, n, why, m, want, decoy=(), at=None, comp=1, max_steps=1, tol=TOL):
        v = np.zeros((n, 3), F)
        i = np.arange(n)
        v[:, 0] = (((3 * i) % 7) - 3) * F(2.0 ** -10)           # at most 3 * 2^-10 = 0.0029 everywhere else
        v[:, 2] = (((2 * i) % 5) - 2) * F(2.0 ** -10)
        if at is not None:
            v[at, comp] = m
        out.append(dict(name=name, op="stable", rule="stable check", why=why, decoy=tuple(decoy), n=n, vel=v, tol=tol,
                        max_steps=max_steps, at=at, want=want))

    n = 255
    v0 = dict(name="stable_zero", op="stable", rule="stable check", why="all velocities zero: stable at entry", decoy=(), n=64,
              vel=np.zeros((64, 3), F), tol=TOL, max_steps=1, at=None, want=(True, 0))
    out.append(v0)
    add("stable_one_below", n, "max |v| one float32 below float32(tol), negative, at the last index: stable",
        -np.nextafter(T32, F(0)), (True, 0), (), n - 1, 2)
    add("stable_at_float32_tol", n, "max |v| == float32(0.01), which is below 1e-2 as a double: stable", T32, (True, 0),
        ("compare_in_f32",), n - 1, 0)
    add("stable_one_above", n, "max |v| the float32 above float32(tol), negative, at the last index: one step, not stable",
        -np.nextafter(T32, F(1)), (False, 1), ("abs_missing", "component_dropped_y") + placement_decoys(n, n - 1), n - 1, 1)
    add("stable_nan", 1024, "one NaN velocity component: never below the tolerance", np.nan, (False, 1), ("fmax_drops_nan",), 700, 1)
    add("stable_no_budget", n, "max_steps = 0: not stable, no step, whatever the velocities", 0.5, (False, 0), (), 3, 1, max_steps=0)
    return out


CASES = _stats_cases() + _probe_cases() + _disp_cases() + _stable_cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)

BATCH = {op: tuple(f"{op}_batch_n{n}" for n in BATCH_SIZES) for op in ("stats", "probe", "disp")}

# The mixed wait_until_stable call: episodes in this order, stable at entry or not.
STABLE_MIX = ("stable_one_above", "stable_zero", "stable_at_float32_tol", "stable_nan", "stable_one_below")

# fs_set_particles: three episodes of different sizes in one call, pid 0 and pid n - 1.
SET_SIZES = (64, 257, 1025)
SET_PIDS = (0, 256, 1024)
SET_POS4 = np.array([[0.5, -0.25, 0.125, 0.0], [-1.5, 2.0, 0.0625, 1.0], [0.03125, 0.75, -3.0, 0.5]], F)
