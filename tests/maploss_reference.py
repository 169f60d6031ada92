"""fs_map_loss (include/flingsim.h) restated in float64 numpy, image by image, sample by sample and pair by pair, in both
normalisations, for the tests of the kernels and of trainops.map_loss_torch.  Like grouploss_reference.py it returns with every
output what an error bound needs: the number n of addends the output is a sum of and A, the sum of their absolute values; the
tolerance is grouploss_reference.bound(n, A).  The offsets are clamped as the header states, so a malformed table has a defined
answer here as well."""
import numpy as np

from grouploss_reference import sigma, softplus

MAX_IMAGE = 4096


def clamp_offsets(offsets, labels):
    """[(begin, count)] per image: begin = clamp(off[b], 0, L), end = clamp(off[b + 1], begin, L), end = min(end, begin + 4096)."""
    off, L, out = np.asarray(offsets, np.int64), int(labels), []
    for b in range(len(off) - 1):
        begin = min(max(int(off[b]), 0), L)
        end = min(max(int(off[b + 1]), begin), L)
        out.append((begin, min(end, begin + MAX_IMAGE) - begin))
    return out


def expanded_bounds(offsets):
    """The [L, 2] segment table fs_group_loss takes for the same images (a well-formed table)."""
    off = np.asarray(offsets, np.int64)
    return np.repeat(np.stack([off[:-1], off[1:]], axis=1), np.diff(off), axis=0).astype(np.int32)


def map_loss_f64(pred, label, offsets, weight, temperature, min_gap, per_image, scale=1.0):
    """image_terms and normalise in one call."""
    return normalise(image_terms(pred, label, offsets, temperature, min_gap), weight, per_image, scale)


def image_terms(pred, label, offsets, temperature, min_gap):
    """The pair-by-pair part, which does not depend on weight, normalisation and scale: what normalise takes."""
    p, y = np.asarray(pred, np.float64), np.asarray(label, np.float64)
    L = len(p)
    tau, gap = float(temperature), float(min_gap)
    images = clamp_offsets(offsets, L)
    S, R, P, C = [], [], [], []
    up, down, count = np.zeros(L), np.zeros(L), np.zeros(L, np.int64)   # per sample: sigma over lost pairs, over won pairs
    with np.errstate(invalid="ignore", over="ignore"):
        for begin, K in images:
            pb, yb = p[begin:begin + K], y[begin:begin + K]
            S.append(float(((pb - yb) ** 2).sum()) if K else 0.0)
            r, n_pairs, conc = 0.0, 0, 0
            for i in range(K):
                wins = yb[i] > yb + gap                      # (i, j) is a pair
                loses = yb > yb[i] + gap                     # (j, i) is a pair
                d = u = 0.0
                if wins.any():
                    x = -(pb[i] - pb[wins]) / tau
                    r += float(softplus(x).sum())
                    d = float(sigma(x).sum())
                    n_pairs += int(wins.sum())
                    conc += int((pb[i] > pb[wins]).sum())
                if loses.any():
                    u = float(sigma(-(pb[loses] - pb[i]) / tau).sum())
                up[begin + i], down[begin + i], count[begin + i] = u, d, int(wins.sum()) + int(loses.sum())
            R.append(r), P.append(n_pairs), C.append(conc)
    return dict(p=p, y=y, tau=tau, images=images, S=np.array(S), R=np.array(R), P=np.array(P, np.int64), C=np.array(C, np.int64),
                up=up, down=down, count=count)


def normalise(terms, weight, per_image, scale=1.0):
    """Returns a dictionary:
    'loss', 'mse', 'rank': (value, n, A);  'dpred': (values [L], n [L], A [L]) -- entries no image owns are NaN with A = NaN;
    'pairs', 'concordant', 'filled' (G'), 'ranked' (G''): integers;  'table': per image a dictionary 'mse': (S_b / K_b, K_b, A),
    'rank': (R_b / P_b, P_b, A), 'pairs', 'concordant'."""
    p, y, tau, images, S, R, P, C = (terms[k] for k in ("p", "y", "tau", "images", "S", "R", "P", "C"))
    up, down, count = terms["up"], terms["down"], terms["count"]
    L, w, s = len(p), float(weight), float(scale)
    counts = np.array([K for _, K in images], np.int64)
    pairs, filled, ranked = int(P.sum()), int((counts > 0).sum()), int((P > 0).sum())
    image_mse = np.where(counts > 0, S / np.maximum(counts, 1), 0.0)
    image_rank = np.where(P > 0, R / np.maximum(P, 1), 0.0)
    if per_image:
        mse = float(image_mse.sum()) / filled if filled else 0.0
        rank = float(image_rank.sum()) / ranked if ranked else 0.0
    else:
        mse = float(S.sum()) / L
        rank = float(R.sum()) / pairs if pairs else 0.0
    n_sq = int(counts.sum())
    out = {"pairs": pairs, "concordant": int(C.sum()), "filled": filled, "ranked": ranked,
           "mse": (mse, n_sq, abs(mse)),                                     # (every addend is positive)
           "rank": (rank, pairs, abs(rank)),
           "loss": (mse + w * rank, n_sq + pairs, abs(mse) + w * abs(rank)),
           "table": [{"mse": (float(image_mse[b]), int(counts[b]), abs(float(image_mse[b]))),
                      "rank": (float(image_rank[b]), int(P[b]), abs(float(image_rank[b]))),
                      "pairs": int(P[b]), "concordant": int(C[b])} for b in range(len(images))]}
    d, n, A = np.full(L, np.nan), np.ones(L, np.int64), np.full(L, np.nan)
    for b, (begin, K) in enumerate(images):
        if not K:
            continue
        at = slice(begin, begin + K)
        base = 2.0 * (p[at] - y[at]) / (filled * K if per_image else L)
        if P[b] and w > 0.0:
            coef = w / ((ranked * P[b] if per_image else pairs) * tau)
            d[at], n[at], A[at] = s * (base + coef * (up[at] - down[at])), 1 + count[at], abs(s) * (np.abs(base) + coef * (up[at] + down[at]))
        else:
            d[at], n[at], A[at] = s * base, 1, abs(s) * np.abs(base)
    out["dpred"] = (d, n, A)
    return out


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))]).astype(np.int64)
