"""Inputs of the fs_sample_actions tests: the shapes and the generator of tests/test_transform_winners_gpu.py restated (values on
a grid of 1 / 64 with planted maxima, 10 % NaN, depth with a blob, zero holes and 2.0 background), plus planted +-inf, one
observation whose two small discs of cloth admit fewer than 16 on-cloth candidates and one without a valid candidate; and,
once per process, every candidate's validity and pretransform pixels through ActionSelector._candidate."""
import functools

import numpy as np

PRIMS, ROTATIONS, D, G, S, REACH, DRAG, PLACE = ["fling", "place"], [-35.0, 0.0, 35.0], 32, 4, 48, 0.62, 6, 5
SCALES = [np.array([0.5, 1.0]), np.array([1.0, 1.5]), np.array([0.75, 2.0]), np.array([1.0, 1.5]), np.array([1.0, 1.5])]
N, FEW, NONE = len(SCALES), 3, 4          # observation FEW: a tiny blob; observation NONE: zero depth everywhere
T, W = len(ROTATIONS) * 2, D - 2 * G
TOTAL = len(PRIMS) * T * W * W
BLOCK = 1024                              # threads of fs_k_sample_rounds; each takes 4 consecutive candidates per trip


def selector():
    from flingbot_amd.action import ActionSelector

    return ActionSelector(PRIMS, ROTATIONS, D, G, DRAG, PLACE, REACH)


def make_case():
    """(values float32 [N, P, T, D, D], depth float32 [N, S, S])."""
    rng = np.random.default_rng(11)
    values = (np.round(rng.random((N, len(PRIMS), T, D, D)) * 64) / 64).astype(np.float32)
    for e in range(N):
        for p in range(len(PRIMS)):
            for t in range(T):
                m = values[e, p, t]
                ys, zs = rng.integers(G, D - G, 2), rng.integers(G, D - G, 2)
                m[ys, zs] = m.max()          # exact ties for the best value inside the cropped region
    values[rng.random(values.shape) < 0.1] = np.nan
    for e in range(N):                       # infinities inside the cropped region, a handful per observation
        for sign in (np.inf, -np.inf):
            p, t = rng.integers(0, len(PRIMS), 6), rng.integers(0, T, 6)
            values[e, p, t, rng.integers(G, D - G, 6), rng.integers(G, D - G, 6)] = sign
    yy, xx = np.mgrid[0:S, 0:S]
    depth = np.full((N, S, S), 2.0, np.float32)
    for e in range(3):
        cx, cy, r = S * (0.45 + 0.05 * e), S * (0.55 - 0.05 * e), S * (0.22 + 0.03 * e)
        blob = (xx - cx) ** 2 + (yy - cy) ** 2 < r * r
        depth[e][blob] = (1.97 - 0.04 * rng.random(int(blob.sum()))).astype(np.float32)
        holes = rng.random((S, S)) < 0.04
        depth[e][holes] = 0.0
    # FEW: nothing but a patch of ground -- a few dozen flings with one point in reach of either arm are valid there, no
    # place -- and on it two discs of cloth 14 pixels apart: fewer than ten flings have both points on them
    depth[FEW] = 0.0
    depth[FEW, 14:34, 14:34] = 2.0
    blob = ((xx - 31) ** 2 + (yy - 24) ** 2 < 4.2 ** 2) | ((xx - 17) ** 2 + (yy - 24) ** 2 < 4.2 ** 2)
    depth[FEW][blob] = (1.97 - 0.04 * rng.random(int(blob.sum()))).astype(np.float32)
    depth[NONE] = 0.0
    return values, depth


def cropped(values):
    """[N, TOTAL]: values[:, :, :, g:-g, g:-g] flattened per observation (the candidates' order)."""
    return np.ascontiguousarray(values[:, :, :, G:-G, G:-G]).reshape(len(values), -1)


def candidate_table(sel, e, depth):
    """dict(valid bool [TOTAL], pixels int32 [TOTAL, 4]) of observation e: ActionSelector._candidate as a predicate.  A zero
    depth under a grasp pixel raises there; the device skips such a candidate, and so does this."""
    valid, pixels = np.zeros(TOTAL, bool), np.zeros((TOTAL, 4), np.int32)
    if not depth[e].any():
        return dict(valid=valid, pixels=pixels)
    for c in range(TOTAL):
        p, t, yy, zz = np.unravel_index(c, (len(PRIMS), T, W, W))
        try:
            got = sel._candidate(PRIMS[p], int(t), int(yy) + G, int(zz) + G, SCALES[e], depth[e])
        except ValueError:
            got = None
        if got is not None:
            valid[c], pixels[c] = True, np.ravel(got["pretransform_pixels"])
    return dict(valid=valid, pixels=pixels)


@functools.lru_cache(maxsize=None)
def case():
    """The inputs and every observation's candidate table, computed once and shared (nobody writes to them)."""
    sel = selector()
    values, depth = make_case()
    return dict(sel=sel, values=values, depth=depth, crop=cropped(values),
                tables=[candidate_table(sel, e, depth) for e in range(N)])


def four_level_table():
    """(i & 3) / 4: four noise levels on the values' own grid, so that perturbed keys tie exactly."""
    return ((np.arange(65536) & 3) / 4).astype(np.float32)


def key_of(e, salt=0):
    return np.array([0x1234567 * (e + 1) + salt, 0x9ABCDEF0 ^ (e * 77)], np.uint64).astype(np.uint32)
