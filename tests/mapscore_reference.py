"""fs_map_score (include/flingsim.h) restated in float64 numpy, image by image and pair by pair ([n, n] comparisons and explicit
loops; nothing shared with trainops.map_score_host, which ranks by sorting), and the constructed inputs of the map-score tests."""
import math

import numpy as np

import maploss_reference as mref

COLUMNS = ("n", "chosen", "best", "chosen_rank", "pairs", "concordant", "Sab", "Saa", "Sbb", "spearman", "regret", "se")
EMPTY = [0.0, -1.0, -1.0, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0, math.nan, math.nan, 0.0]


def first_largest(v):
    """The lowest index of the largest value, by an explicit loop."""
    at = 0
    for k in range(1, len(v)):
        if v[k] > v[at]:
            at = k
    return at


def centred_ranks(v):
    """a_i = 2 #{v_j < v_i} + #{v_j == v_i} + 1 - (n + 1) as int64: the centred doubled average ranks."""
    below = (v[None, :] < v[:, None]).sum(axis=1).astype(np.int64)
    equal = (v[None, :] == v[:, None]).sum(axis=1).astype(np.int64)
    return 2 * below + equal + 1 - (len(v) + 1)


def score_image(p, y, min_gap=0.0):
    """(row [12], se_addends): the row of one image from its float32 predictions and labels in list order."""
    p, y = np.asarray(p, np.float32), np.asarray(y, np.float32)
    where = np.flatnonzero(np.isfinite(p) & np.isfinite(y))
    n = len(where)
    if n == 0:
        return list(EMPTY), 0.0
    P, Y = p[where].astype(np.float64), y[where].astype(np.float64)
    chosen, best = first_largest(P), first_largest(Y)
    wins = Y[:, None] > Y[None, :] + float(min_gap)               # [i, j]: (i, j) is a pair
    a, b = centred_ranks(P), centred_ranks(Y)
    sab, saa, sbb = int((a * b).sum()), int((a * a).sum()), int((b * b).sum())
    spearman = math.nan if n < 2 or saa == 0 or sbb == 0 else float(sab) / math.sqrt(float(saa) * float(sbb))
    addends = [(float(P[k]) - float(Y[k])) ** 2 for k in range(n)]
    row = [float(n), float(where[chosen]), float(where[best]), float(int((Y > Y[chosen]).sum())), float(int(wins.sum())),
           float(int((wins & (P[:, None] > P[None, :])).sum())), float(sab), float(saa), float(sbb), spearman,
           float(Y[best]) - float(Y[chosen]), math.fsum(addends)]
    return row, math.fsum(addends)


def score_rows(value, offsets, pix, label, min_gap=0.0):
    """(rows float64 [G, 12], se_addends [G]) of dense maps value [G, S]: offsets clamped as the kernel clamps them, pixels into
    [0, S)."""
    value = np.asarray(value, np.float32)
    pix, label = np.clip(np.asarray(pix, np.int64), 0, value.shape[1] - 1), np.asarray(label, np.float32)
    rows, sums = [], []
    for b, (begin, count) in enumerate(mref.clamp_offsets(offsets, len(label))):
        row, A = score_image(value[b, pix[begin:begin + count]], label[begin:begin + count], min_gap)
        rows.append(row)
        sums.append(A)
    return np.array(rows, np.float64).reshape(-1, len(COLUMNS)), np.array(sums, np.float64)


def has_ties(v):
    v = np.asarray(v)
    v = v[np.isfinite(v)]
    return len(np.unique(v)) < len(v)


def values(n, seed, quantised):
    """(p, y) float32 [n].  quantised: normal draws snapped to quarters, so that ranks tie on both sides.  Otherwise distinct by
    construction -- a random permutation of a grid of spacing 1/64 (1/128), each point moved by less than 0.4 of the spacing:
    n <= 4096 keeps |v| <= 32, where float32 resolves 4e-6."""
    rng = np.random.default_rng([int(seed), int(n), int(bool(quantised))])
    if quantised:
        p, y = np.round(rng.standard_normal(n) * 4) / 4, np.round(rng.standard_normal(n) * 2) / 4
    else:
        p = (rng.permutation(n) - n // 2 + 0.4 * rng.random(n)) / 64
        y = (rng.permutation(n) - n // 2 + 0.4 * rng.random(n)) / 128
    return p.astype(np.float32), y.astype(np.float32)


def scattered(lengths, seed, quantised):
    """A batch for the kernel: (value [G, 4096] zero-filled with the predictions at distinct random pixels -- the first listed
    pixel of an image is 0 or 4095, alternating, and an image of two or more lists both --, offsets int64 [G + 1], pix int32 [L],
    label float32 [L], pred float32 [L] = the predictions in list order)."""
    rng = np.random.default_rng([int(seed), 77])
    offsets = mref.offsets_of(lengths)
    value = np.zeros((len(lengths), 4096), np.float32)
    pix, label, pred = [], [], []
    for b, n in enumerate(lengths):
        p, y = values(n, seed + b, quantised)
        where = rng.permutation(np.arange(1, 4095))[:max(n - 2, 0)]
        corners = [0, 4095] if b % 2 == 0 else [4095, 0]
        where = np.concatenate([corners, where]).astype(np.int64)[:n] if n else np.zeros(0, np.int64)
        if n >= 3:
            where[1:] = where[1:][rng.permutation(n - 1)]         # the second corner anywhere in the list
        value[b, where] = p
        pix.append(where)
        label.append(y)
        pred.append(p)
    cat = lambda parts, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)   # noqa: E731
    return value, offsets, cat(pix, np.int32), cat(label, np.float32), cat(pred, np.float32)


def ulps(a, b):
    """The distance of two finite doubles in units of the last place (0 for equal bits; NaN against NaN is 0)."""
    if math.isnan(a) or math.isnan(b):
        return 0 if math.isnan(a) and math.isnan(b) else math.inf
    ia, ib = (int(np.float64(v).view(np.int64)) for v in (a, b))
    ia, ib = (v if v >= 0 else -(v & 0x7fffffffffffffff) for v in (ia, ib))
    return abs(ia - ib)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))
