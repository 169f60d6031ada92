"""Constructed particle sets for the coverage reward (fs_k_coverage, flingbot_amd/csrc/fs_render.hip).

Plain numpy, importable without a GPU.  Every case is a float32[n, 4] position array (x, y, z, w = 1; y varies and never
matters) built deterministically: exact lattices where a rule needs exact arithmetic, np.random.RandomState(seed) where it
needs a cloud.  `rule` says what the case pins, `why` how, `decoy` names the mistakes a plausibly wrong kernel makes that this
very case notices (the mutation switches of the scalar restatement in tests/test_coverage_edges_cpu.py).  The expected areas
are not in this table: tests/golden/make_golden.py (`coverage_edges`) runs the cases through the reference's own
get_current_covered_area and writes tests/golden/coverage_edges_golden.npz, which stores per case the float64 area, n and
the SHA-256 of the position bytes; the CPU and GPU tests compare against that file.

The operation (reference environment/flex_utils.py:358-395), in float32 up to the slots:
    span = (max - min) / 100 per axis;  lo = max(round((p - min - r) / span), 0), hi = min(round((p - min + r) / span), 100)
    with round = half-to-even and r = float32(0.00625);  N = max(hi - lo) + 1 per axis over all particles;  every particle
    marks the cells (floor(k * (hi - lo) / N + lo))_{k < N} on x times the same on z, i.e. lo .. hi - 1, or lo alone when
    hi == lo;  flat index x * 100 + z clipped to [0, 9999];  area = cells * span_x * span_z in float64.
A slot can reach 100 only as lo == hi == 100, which needs r / span < 0.5: an extent above 1.25 m.  Then x == 100 collapses
onto cell 9999 and z == 100 aliases onto (x + 1, 0).  Below that extent the count of cells is invariant under a transpose
of the grid, so `swap_axes` can only be seen by the cases that reach slot 100.

Spans used by the lattice cases, all exact in float32 and exactly 1/100 of their (exact) extent:
    2^-6 (extent 1.5625, 2r/span = 0.8: ranges 0 or 1 wide)      2^-7 (0.78125, 1.6: 1 or 2)      2^-8 (0.390625, 3.2: 3 or 4)
    2^-9 (0.1953125, 6.4: 6 or 7)      3 * 2^-9 (0.5859375, 2.13: 2 or 3)
ties_rounded_division alone uses spans with a full mantissa (float32(0.6) / 100, float32(0.9) / 100): there the division rounds.

Where this table departs from the list it was written from: `clip_before_round` names no case because it is no mistake (see
EQUIVALENT_MUTATIONS); `swap_axes` is named by alias_x100 alone, not by the anisotropic pair or alias_z100, because a
transposed grid has the same count of cells unless slot 100 is reached, and in alias_z100 the transposed index happens to
collapse as many cells as the true one aliases; `f64div` is the whole quotient in float64, double-precision radius included
(with a span of 2^-7 the division itself is exact in either precision), and `f64quot`, the division alone, has a case of its own.
"""
import hashlib

import numpy as np

R32 = np.float32(0.00625)
MUTATIONS = ("roundf", "f64div", "f64quot", "noalias", "inclusive_end", "swapN", "swap_axes", "clip_before_round",
             "f32_product")
# clip_before_round (clip the float quotient to [0, 100], then round) is carried by the restatement but names no case: the
# bounds are integers and rounding is monotonic, so it commutes with the reference's round-then-clip on every input, and on
# a zero or NaN span the area is 0 or NaN either way.  tests/test_coverage_edges_cpu.py asserts that equality on the table.
EQUIVALENT_MUTATIONS = ("clip_before_round",)
SIZES = (2, 63, 64, 65, 1023, 1024, 1025, 2049, 16512)


def _pos(xz, shift=(0.0, 0.0)):
    """float32[n, 4] from n (x, z) pairs: the coordinates are rounded to float32 first, then shifted in float32."""
    xz = np.asarray(xz, np.float64).reshape(-1, 2).astype(np.float32)
    n = xz.shape[0]
    p = np.ones((n, 4), np.float32)
    p[:, 0] = xz[:, 0] + np.float32(shift[0])
    p[:, 2] = xz[:, 1] + np.float32(shift[1])
    p[:, 1] = (0.01 + 0.003 * ((7 * np.arange(n)) % 11) - 0.004 * (np.arange(n) % 3)).astype(np.float32)  # some below 0
    return p


def _case(name, rule, pos, why, decoy=()):
    assert pos.dtype == np.float32 and pos.ndim == 2 and pos.shape[1] == 4 and (pos[:, 3] == 1).all(), name
    assert np.isfinite(pos[:, 1]).all() or name == "nan_y_only", name
    assert all(d in MUTATIONS and d not in EQUIVALENT_MUTATIONS for d in decoy), name
    return dict(name=name, rule=rule, why=why, pos=np.ascontiguousarray(pos), decoy=tuple(decoy))


def sha256(pos):
    return hashlib.sha256(np.ascontiguousarray(pos, np.float32).tobytes()).hexdigest()


def quotients(pos):
    """The four float32 slot quotients of every particle, as the reference forms them: (x lo, x hi, z lo, z hi)[n]."""
    x, z = pos[:, 0], pos[:, 2]
    ox, oz = x - x.min(), z - z.min()
    sx, sz = (x.max() - x.min()) / np.float32(100), (z.max() - z.min()) / np.float32(100)
    q = np.stack([(ox - R32) / sx, (ox + R32) / sx, (oz - R32) / sz, (oz + R32) / sz])
    assert q.dtype == np.float32
    return q


# ---- ties: span 2^-7 on both axes; x-axis ties live in z rows below slot 50, z-axis ties in z slots from 51 up.  The k of the
# quotients k + 0.5, per group.  Half-even and half-away differ on even k only: a low slot then loses a cell, a high slot gains
# one.  The low-slot groups are mostly even, the high-slot groups mostly odd and shorter, so that neither the two rounding modes nor
# the two one-ulp neighbours of the tie can cancel out in the count of cells.
TIE_KS_X_LO, TIE_KS_X_HI = (2, 8, 24, 62, 36, 90, 5, 11), (37, 97, 13, 51, 75, 20)
TIE_KS_Z_LO, TIE_KS_Z_HI = (52, 58, 66, 84, 72, 96, 55, 61), (53, 97, 73, 65, 85, 60)


def _tie_members(step):
    """28 particles: 8 whose x low slot, 6 whose x high slot, 8 whose z low slot, 6 whose z high slot has the quotient k + 0.5
    (`step` = 0), or its float32 neighbour below / above (`step` = -1 / +1, by np.nextafter on the coordinate)."""
    def tied(k, sign):          # coordinate c with float32(c -/+ r) == (k + 0.5) / 128 (sign = -1: low slot, +1: high slot)
        a = np.float32((k + 0.5) / 128)
        c = np.float32(a - np.float32(sign) * R32)
        if step:                # the first coordinate on that side whose float32(c -/+ r) is a's neighbour
            a = np.nextafter(a, np.float32(step * 4.0))
            for _ in range(4):
                c = np.nextafter(c, np.float32(step * 4.0))
                if np.float32(c + np.float32(sign) * R32) == a:
                    break
        return c

    xz = []
    for j, k in enumerate(TIE_KS_X_LO):
        xz.append((tied(k, -1), (3 * j + 2) / 128))            # rows 3j+1, 3j+2: one particle per pair of rows
    for j, k in enumerate(TIE_KS_X_HI):
        xz.append((tied(k, +1), (3 * (j + 8) + 2) / 128))
    for j, k in enumerate(TIE_KS_Z_LO):
        xz.append(((3 * j + 2) / 128, tied(k, -1)))
    for j, k in enumerate(TIE_KS_Z_HI):
        xz.append(((3 * (j + 8) + 2) / 128, tied(k, +1)))
    return xz


def _ties(name, step, why, decoy):
    pos = _pos([(0.0, 0.0)] + _tie_members(step) + [(0.78125, 0.78125)])
    q = quotients(pos)
    assert (pos[:, 0].max() - pos[:, 0].min()) / np.float32(100) == np.float32(2.0 ** -7) == \
        (pos[:, 2].max() - pos[:, 2].min()) / np.float32(100), name
    ks = np.array(TIE_KS_X_LO + TIE_KS_X_HI + TIE_KS_Z_LO + TIE_KS_Z_HI, np.float32) + np.float32(0.5)
    mine = np.concatenate([q[0, 1:9], q[1, 9:15], q[2, 15:23], q[3, 23:29]])
    if step == 0:
        assert np.array_equal(mine, ks), name                   # exactly on the tie
    else:
        assert np.array_equal(mine, np.nextafter(ks, np.float32(step * 1000.0))), name  # its float32 neighbour
    others = np.concatenate([q[2:, 1:15].ravel(), q[:2, 15:29].ravel(), q[1, 1:9], q[0, 9:15], q[3, 15:23], q[2, 23:29]])
    assert (np.abs(others - np.floor(others) - 0.5) > 0.05).all(), name     # no other quotient is anywhere near a tie
    return _case(name, "rounding", pos, why, decoy)


def _rounded_division():
    """Spans that are no power of two (extents float32(0.6) and float32(0.9)): 16 low-slot quotients that the correctly rounded
    float32 division puts exactly on k + 0.5, k odd, so half-even takes k + 1, while the exact quotient of the same two
    float32 numbers lies below the tie.  A division in float64, or one that is an ulp off downwards, takes k."""
    ex, ez = np.float32(0.6), np.float32(0.9)
    sx, sz = ex / np.float32(100), ez / np.float32(100)
    ks_x, ks_z = (3, 11, 19, 25, 29, 35, 45, 57), (53, 65, 67, 69, 71, 81, 83, 85)

    def tied(k, s):
        a = np.float32((k + 0.5) * float(s))
        c = np.float32(a + R32)
        assert np.float32(c - R32) == a and np.float32(a / s) == np.float32(k + 0.5) and k % 2 == 1
        assert float(a) / float(s) < k + 0.5       # float64 sees that the quotient is not a tie
        return c

    xz = [(0.0, 0.0)]
    xz += [(tied(k, sx), (3 * j + 2) * float(sz)) for j, k in enumerate(ks_x)]
    xz += [((3 * j + 2) * float(sx), tied(k, sz)) for j, k in enumerate(ks_z)]
    pos = _pos(xz + [(ex, ez)])
    q = quotients(pos)
    assert np.array_equal(q[0, 1:9], np.array(ks_x, np.float32) + np.float32(0.5))
    assert np.array_equal(q[2, 9:17], np.array(ks_z, np.float32) + np.float32(0.5))
    others = np.concatenate([q[1:, 1:9].ravel(), q[:2, 9:17].ravel(), q[3, 9:17]])
    assert (np.abs(others - np.floor(others) - 0.5) > 0.05).all()
    return pos


def _spread(n, seed, box, shift):
    """Seeded cloud of n particles in box = (x, y, z) extents; index 0 holds the x maximum and the z minimum, index n - 1 the x
    minimum and the z maximum, each alone and 1 cm outside the cloud."""
    rs = np.random.RandomState(seed)
    p = np.ones((n, 4), np.float64)
    p[:, :3] = rs.rand(n, 3) * box
    p[:, 1] -= 0.3 * box[1]
    p[0, 0], p[0, 2] = box[0] + 0.01, -0.01
    p[n - 1, 0], p[n - 1, 2] = -0.01, box[2] + 0.01
    p[:, 0] += shift[0]
    p[:, 2] += shift[1]
    return p.astype(np.float32)


def _build():
    cases = []

    # ---- rounding mode and the float32 quotient
    cases.append(_ties("ties_half_even", 0,
                       "28 quotients are exactly k + 0.5, k even and odd, on the low and the high slot of both axes: half-even "
                       "takes the even neighbour, half-away the upper one; a double-precision radius (0.00625 without the f) "
                       "moves every one of them off the tie, downwards",
                       ("roundf", "f64div")))
    cases.append(_ties("ties_one_ulp_below", -1,
                       "the same particles one float32 step below the tie: every quotient is the float32 neighbour of k + 0.5 "
                       "and rounds to k, so neither rounding mode may see a tie", ()))
    cases.append(_ties("ties_one_ulp_above", +1, "one float32 step above the tie: every quotient rounds to k + 1", ()))

    cases.append(_case("ties_rounded_division", "rounding", _rounded_division(),
                       "spans 0.006 and 0.009: 16 quotients are k + 0.5 only after the float32 division has rounded them",
                       ("f64quot", "f64div")))

    # ---- the flat-index quirk (extent 2 m: span 0.02, r / span = 0.3125)
    cases.append(_case("alias_x100", "flat index", _pos([(0, 0), (2, 2), (2, 0.5), (2, 1.0)]),
                       "three particles at the x maximum have lo == hi == 100: 100 * 100 + z is clipped to 9999 for all of them",
                       ("noalias", "swap_axes")))
    cases.append(_case("alias_z100", "flat index", _pos([(0, 0), (2, 2), (0.5, 2), (0.52, 0)]),
                       "the particle at the z maximum with x slot 25 writes 25 * 100 + 100 = cell (26, 0), which (0.52, 0) holds "
                       "(the transposed index collapses that particle onto 9999 instead: the same count)", ("noalias",)))

    # ---- [lo, hi): x span 2^-7, z span 3 * 2^-9; isolated particles with ranges 1 or 2 wide on x and 2 or 3 wide on z
    sx, sz = 2.0 ** -7, 3 * 2.0 ** -9
    xz = [(0.0, 0.0), (100 * sx, 100 * sz)]
    for cx, cz in ((10.5, 10.0), (20.5, 20.5), (30.0, 30.0), (40.0, 40.5), (50.5, 61.0), (71.0, 50.5)):
        xz.append((cx * sx, cz * sz))
    pos = _pos(xz, shift=(-3.0, 1.5))            # exact: every coordinate is a multiple of 2^-10 below 4
    q = quotients(pos)
    assert np.allclose(q[:, 2], [9.7, 11.3, 10 - 16 / 15, 10 + 16 / 15], atol=1e-4)
    cases.append(_case("end_exclusive", "range ends", pos,
                       "six isolated particles, ranges 1 x 2, 1 x 3, 2 x 2, 2 x 3, 1 x 2, 2 x 3 slots: hi itself is never marked",
                       ("inclusive_end",)))
    # x span 2^-6 (ranges 0 or 1 wide): a particle on a slot centre has hi == lo and still marks lo
    xz = [(0.0, 0.0), (1.5625, 0.78125)]
    for cx, cz in ((10.0, 10.5), (20.0, 20.0), (30.5, 30.5), (40.5, 40.0), (55.0, 70.0)):
        xz.append((cx * 2.0 ** -6, cz * sx))
    cases.append(_case("end_exclusive_empty_range", "range ends", _pos(xz),
                       "x span 2^-6: particles on a slot centre have hi == lo on x and mark that one column; the others 1 wide",
                       ("inclusive_end",)))

    # ---- N = max(hi - lo) + 1 comes from the last particle: x span 2^-8 (last 4 wide, the clipped corners 2), z span 2^-9
    # (last 7 wide, the corners 3).  Without the last particle N is 3 and 4 and its own range gets holes; with Nx and Nz
    # swapped the 7-wide z range is sampled 5 times.
    for name, n in (("n_from_last_particle", 66), ("n_from_last_particle_1026", 1026)):
        ex, ez = 100 * 2.0 ** -8, 100 * 2.0 ** -9
        corners = [(0.0, 0.0), (ex, ez), (0.0, ez), (ex, 0.0)]
        xz = [corners[i % 4] for i in range(n - 1)] + [(41 * 2.0 ** -8, 57.5 * 2.0 ** -9)]
        pos = _pos(xz, shift=(0.25, -0.5))       # exact: multiples of 2^-10 below 1
        cases.append(_case(name, "sample count", pos,
                           f"index {n - 1} alone has the widest range on both axes (4 on x, 7 on z); all others sit in the "
                           "corners, where the clip at 0 and at 100 cuts their ranges to 2 and 3", ("swapN",)))

    # ---- Nx and Nz an order of magnitude apart
    rs = np.random.RandomState(11)
    cloud = rs.rand(300, 2) * [0.9, 0.03]
    cases.append(_case("anisotropic_x", "sample count", _pos(cloud, shift=(-3.7, 12.25)),
                       "300 particles in 0.9 m x 0.03 m: Nx = 3, Nz = 43", ("swapN",)))
    cases.append(_case("anisotropic_z", "sample count", _pos(cloud[:, ::-1], shift=(7.5, -0.4)), "the transpose", ("swapN",)))

    # ---- every range is [0, 100]
    xz = np.array([(0.0, 0.0), (0.004, 0.001), (0.001, 0.004), (0.002, 0.002), (0.003, 0.0035)])
    cases.append(_case("tiny_cluster", "sample count", _pos(xz, shift=(40.0, -17.0)),
                       "5 particles within 4 mm, 40 m from the origin: N = 101 on both axes, all 10000 cells", ()))

    # ---- zero extent: the reference divides by a zero span; what it returns is in the fixture
    cases.append(_case("one", "zero extent", _pos([(0.3, -0.2)]), "n = 1", ()))
    cases.append(_case("two_coincident", "zero extent", _pos([(-1.25, 0.5), (-1.25, 0.5)]), "n = 2, the same point", ()))
    t = np.linspace(0.0, 0.4, 7)
    cases.append(_case("line_x", "zero extent", _pos(np.stack([t - 0.1, np.full(7, 0.25)], 1)), "all z equal", ()))
    cases.append(_case("line_z", "zero extent", _pos(np.stack([np.full(7, -0.75), t + 2.0], 1)), "all x equal", ()))

    # ---- particle counts around the wave (64) and the block (1024); the bounding box is owned by index 0 and index n - 1
    for n in SIZES:
        cases.append(_case(f"sizes_{n}", "particle counts", _spread(n, 100 + n, (0.6, 0.1, 0.4), (-0.9, 3.1)),
                           f"n = {n}: the x minimum and the z maximum come from the last index", ("f32_product",)))

    # ---- NaN: np.min / np.max propagate it
    clean = _spread(66, 7, (0.5, 0.1, 0.3), (0.2, -0.2))
    cases.append(_case("nan_clean", "nan", clean, "the set the next three are made from", ()))
    for name, col in (("nan_x", 0), ("nan_z", 2), ("nan_y_only", 1)):
        p = clean.copy()
        p[65 if col != 1 else 40, col] = np.nan
        cases.append(_case(name, "nan", p, "one NaN coordinate, in the second wave" if col != 1 else
                           "a NaN height changes nothing", ()))
    return cases


CASES = _build()
BY_NAME = {c["name"]: c for c in CASES}
NAN_CASES = ("nan_clean", "nan_x", "nan_z", "nan_y_only")   # kept in a simulator context of their own, never stepped

def grid_for(n):
    """A (dimx, dimz) grid cloth with exactly n particles."""
    for dx in range(int(np.sqrt(n)), 0, -1):
        if n % dx == 0:
            return dx, n // dx
    raise AssertionError(n)
