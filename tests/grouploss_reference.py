"""fs_group_loss (include/flingsim.h) restated in float64 numpy, sample by sample and pair by pair, for the tests of the kernel
and of trainops.group_loss_torch.  Besides every output it returns what an error bound needs: the number n of addends the output
is a sum of and A, the sum of their absolute values.  Summing n fp32 addends in any order is off by at most (n - 1) 2^-24 A."""
import numpy as np

U = 2.0 ** -24          # the unit roundoff of fp32


def softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def sigma(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0.0, 1.0 / (1.0 + e), e / (1.0 + e))


def group_loss_f64(pred, label, bounds, weight, temperature, min_gap, scale=1.0):
    """pred, label: [B] (their values are taken as they are, in float64); bounds int [B, 2].  Returns a dictionary:
    'loss', 'mse', 'rank': (value, n, A);  'dpred': (values [B], n [B], A [B]);  'pairs', 'concordant': integers."""
    p, y = np.asarray(pred, np.float64), np.asarray(label, np.float64)
    B = len(p)
    b = np.asarray(bounds, np.int64)
    assert b.shape == (B, 2)
    w, tau, gap, s = float(weight), float(temperature), float(min_gap), float(scale)
    sq = (p - y) ** 2 / B
    rank_terms = 0.0                       # sum of softplus over the pairs
    pairs = concordant = 0
    up = np.zeros(B)                       # per sample: sum over the pairs it loses of sigma
    down = np.zeros(B)                     # per sample: sum over the pairs it wins of sigma
    count = np.zeros(B, np.int64)          # per sample: the pairs it is part of
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(B):
            lo, hi = int(b[i, 0]), int(b[i, 1])
            pj, yj = p[lo:hi], y[lo:hi]
            wins = y[i] > yj + gap                       # (i, j) is a pair
            loses = yj > y[i] + gap                      # (j, i) is a pair
            if wins.any():
                x = -(p[i] - pj[wins]) / tau
                rank_terms += float(softplus(x).sum())
                down[i] = float(sigma(x).sum())
                pairs += int(wins.sum())
                concordant += int((p[i] > pj[wins]).sum())
            if loses.any():
                up[i] = float(sigma(-(pj[loses] - p[i]) / tau).sum())
            count[i] = int(wins.sum()) + int(loses.sum())
    mse = float(sq.sum())
    rank = rank_terms / pairs if pairs else 0.0
    out = {"pairs": pairs, "concordant": concordant,
           "mse": (mse, B, float(np.abs(sq).sum())),
           "rank": (rank, pairs, abs(rank)),                                 # (every addend is positive)
           "loss": (mse + w * rank, B + pairs, float(np.abs(sq).sum()) + w * abs(rank))}
    base = 2.0 * (p - y) / B
    if pairs and w > 0.0:
        coef = w / (pairs * tau)
        d, n, A = s * (base + coef * (up - down)), 1 + count, abs(s) * (np.abs(base) + coef * (up + down))
    else:
        d, n, A = s * base, np.ones(B, np.int64), abs(s) * np.abs(base)
    out["dpred"] = (d, n, A)
    return out


def bound(n, A):
    """The issue's tolerance for an output that sums n addends of absolute sum A: (n + 16) 2^-24 A -- the worst case of the
    summation in any order plus 16 units for the arithmetic of one addend (a subtraction / division, expf, log1pf and a
    reciprocal at up to 4 each; assumed, not measured)."""
    return (np.asarray(n, np.float64) + 16.0) * U * np.asarray(A, np.float64)


def host_pairs(label, bounds, min_gap=0.0):
    """P alone, from labels and bounds."""
    y = np.asarray(label, np.float64)
    total = 0
    for i, (lo, hi) in enumerate(np.asarray(bounds, np.int64)):
        total += int((y[i] > y[lo:hi] + float(min_gap)).sum())
    return total


def layout(B, kind, seed=0):
    """Segment tables [B, 2] by name: 'singletons', 'whole', 'mixed' (lengths 1..5 at random, the last cut to what is left),
    'fours' (groups of 4, the last cut), or a tuple (begin, end): that one segment among singletons."""
    if kind == "singletons":
        lengths = [1] * B
    elif kind == "whole":
        lengths = [B]
    elif kind == "fours":
        lengths = [4] * (B // 4) + ([B % 4] if B % 4 else [])
    elif kind == "mixed":
        rng, lengths = np.random.default_rng(seed), []
        while sum(lengths) < B:
            lengths.append(min(int(rng.integers(1, 6)), B - sum(lengths)))
    else:
        lo, hi = kind
        assert 0 <= lo < hi <= B
        lengths = [1] * lo + [hi - lo] + [1] * (B - hi)
    out, at = np.empty((B, 2), np.int32), 0
    for n in lengths:
        out[at:at + n] = (at, at + n)
        at += n
    assert at == B
    return out


def batch(B, seed, spread=0.3, grid=0.05):
    """(pred, label) float32 [B]: predictions N(0, spread), labels N(0, 0.1) snapped to multiples of `grid` so that ties occur."""
    rng = np.random.default_rng(seed)
    pred = (rng.standard_normal(B) * spread).astype(np.float32)
    label = (np.round(rng.standard_normal(B) * 0.1 / grid) * grid).astype(np.float32)
    return pred, label
