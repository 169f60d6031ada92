"""fs_map_list_loss (include/flingsim.h) restated in float64 numpy, image by image, in both normalisations, for the tests of the
kernels and of trainops.map_list_torch.  Like maploss_reference.py it returns with every output what an error bound needs: the
number n of addends the output is a sum of and A, the sum of their absolute values.  The tolerances are the tree's own: a float32
output lies within grouploss_reference.bound(n, A) = (n + 16) 2^-24 A, a double output within bound64(n, A) = (n + 16) 2^-53 A (what
test_mapscore_gpu.py uses for `se`); integer-valued outputs are exact.  Both are relative bounds, and a relative bound cannot hold
below a format's normal range: there one rounding is half a unit of 2^-149 (float32) or 2^-1074 (double) whatever A is -- a
gradient of 1e-51 rounds to the float32 0.0, as it must -- and a spread of 10^4 temperatures puts outputs there.  bound32 and
bound64 therefore add the same (n + 16) of those units: an absolute 1e-43 or 1e-321 at the most, nothing a wrong result hides in.
The offsets are clamped as the header states, so a malformed table has a defined answer here as well.

What counts as an addend, output by output:
  D_b            = sum_i q_i lq_i - sum_i q_i ls_i: 2 K_b addends, A = sum_i q_i (|lq_i| + |ls_i|) -- the negative entropy of q and
                   its cross-entropy with s, which cancel to the small D_b; the rounding of lq_i and of ls_i is relative to each;
  list, term     the coef_b-weighted sum of the D_b: n = G_l + the 2 K_b of the listed images, A = sum_b coef_b A_b (times weight);
  dpred_i        n = K_b (the sum of exp behind s_i and q_i), A = grad_scale weight coef_b (s_i + q_i) / T_p;
  q at an index  n = K_b, A = q (1 + |lq|): exp turns an absolute error of lq into a relative error of q, |lq| units of it;
  the two means  n = G_l + the longest listed K_b, A = the mean of the A above (every addend is positive).
The log-sum-exp is formed as the header forms it: the maximum's own addend (exactly 1) stays out of the sum, which goes through
log1p, so ls_i = (a_i - max a) - log1p(...) has two terms of one sign."""
import numpy as np

from maploss_reference import clamp_offsets, offsets_of  # noqa: F401  (offsets_of: for the tests)

U64 = 2.0 ** -53


def bound32(n, A):
    """grouploss_reference.bound, (n + 16) 2^-24 A, plus (n + 16) units of float32's subnormal spacing 2^-149."""
    return (np.asarray(n, np.float64) + 16.0) * (2.0 ** -24 * np.asarray(A, np.float64) + 2.0 ** -149)


def bound64(n, A):
    """(n + 16) 2^-53 A, the same bound for an output formed in double, plus (n + 16) units of double's subnormal spacing."""
    return (np.asarray(n, np.float64) + 16.0) * (U64 * np.asarray(A, np.float64) + 2.0 ** -1074)


def arg_max(v):
    """The lowest index among the largest values; a NaN never wins (an array of NaNs names index 0)."""
    v = np.asarray(v)
    with np.errstate(invalid="ignore"):
        return int(np.argmax(np.where(np.isnan(v), -np.inf, v)))


def log_softmax(x, top):
    """x - logsumexp(x) with x[top] the maximum: (x - x[top]) - log1p(sum of exp(x - x[top]) without index top), in index order."""
    shifted = x - x[top]
    rest = np.exp(np.delete(shifted, top))
    return shifted - np.log1p(float(np.sum(rest)))


def image_terms(pred, label, offsets, pred_temperature, label_temperature=None):
    """The per-image part, which does not depend on weight, normalisation and scale: what normalise takes.  pred and label are
    taken as they are, in float64."""
    p, y = np.asarray(pred, np.float64), np.asarray(label, np.float64)
    tp = float(pred_temperature)
    ty = tp if label_temperature is None else float(label_temperature)
    images = clamp_offsets(offsets, len(p))
    rows = []
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for begin, K in images:
            if K < 2:
                rows.append(None)
                continue
            pb, yb = p[begin:begin + K], y[begin:begin + K]
            chosen, best = arg_max(pb), arg_max(yb)
            ls, lq = log_softmax(pb / tp, chosen), log_softmax(yb / ty, best)
            s, q = np.exp(ls), np.exp(lq)
            addend = np.where(q == 0.0, 0.0, q * (lq - ls))
            rows.append(dict(K=K, begin=begin, chosen=chosen, best=best, s=s, q=q, ls=ls, lq=lq, D=float(addend.sum()),
                             A=float(np.where(q == 0.0, 0.0, q * (np.abs(lq) + np.abs(ls))).sum()), g=(s - q) / tp))
    return dict(L=len(p), tp=tp, images=images, rows=rows)


def normalise(terms, weight, per_image, scale=1.0):
    """Returns a dictionary:
    'term', 'list', 'chosen_mass', 'best_mass': (value, n, A);  'listed' (G_l), 'labels' (L_l), 'hits' (H): integers;
    'dpred': (values [L], n [L], A [L]) -- entries no image owns are NaN with A = NaN;
    'coef': [G] (0 for an image that is not listed);
    'table': per image a dictionary 'D': (D_b, 2 K_b, A_b), 'q_chosen': (q, K_b, A), 'chosen', 'best' -- (0, 0, 0), (0, 0, 0), -1, -1
    for an image that is not listed."""
    L, tp, images, rows = terms["L"], terms["tp"], terms["images"], terms["rows"]
    w, sc = float(weight), float(scale)
    listed = [r for r in rows if r is not None]
    G_l, L_l = len(listed), sum(r["K"] for r in listed)
    coef = np.array([0.0 if r is None else (1.0 / G_l if per_image else r["K"] / L_l) for r in rows])
    total = sum(coef[b] * r["D"] for b, r in enumerate(rows) if r is not None) if G_l else 0.0
    total_A = sum(coef[b] * r["A"] for b, r in enumerate(rows) if r is not None) if G_l else 0.0
    n_list = G_l + 2 * L_l
    mass = lambda v: v * (1.0 + abs(np.log(v))) if v > 0.0 else 0.0   # noqa: E731
    q_c = [float(r["q"][r["chosen"]]) for r in listed]
    q_b = [float(r["q"][r["best"]]) for r in listed]
    n_mean = G_l + max([r["K"] for r in listed], default=0)
    out = {"listed": G_l, "labels": L_l, "hits": sum(r["chosen"] == r["best"] for r in listed), "coef": coef,
           "list": (float(total), n_list, float(total_A)), "term": (w * float(total), n_list, w * float(total_A)),
           "chosen_mass": (float(np.mean(q_c)) if G_l else 0.0, n_mean, float(np.mean([mass(v) for v in q_c])) if G_l else 0.0),
           "best_mass": (float(np.mean(q_b)) if G_l else 0.0, n_mean, float(np.mean([mass(v) for v in q_b])) if G_l else 0.0),
           "table": []}
    d, n, A = np.full(L, np.nan), np.ones(L, np.int64), np.full(L, np.nan)
    for b, ((begin, K), r) in enumerate(zip(images, rows)):
        at = slice(begin, begin + K)
        if r is None:
            d[at], n[at], A[at] = 0.0, 1, 0.0
            out["table"].append({"D": (0.0, 0, 0.0), "q_chosen": (0.0, 0, 0.0), "chosen": -1, "best": -1})
            continue
        if w > 0.0:
            d[at], n[at], A[at] = sc * w * coef[b] * r["g"], K, abs(sc) * w * coef[b] * (r["s"] + r["q"]) / tp
        else:
            d[at], n[at], A[at] = 0.0, 1, 0.0
        qc = float(r["q"][r["chosen"]])
        out["table"].append({"D": (r["D"], 2 * K, r["A"]), "q_chosen": (qc, K, mass(qc)), "chosen": r["chosen"], "best": r["best"]})
    out["dpred"] = (d, n, A)
    return out


def map_list_f64(pred, label, offsets, weight, pred_temperature, label_temperature=None, per_image=False, scale=1.0):
    """image_terms and normalise in one call."""
    return normalise(image_terms(pred, label, offsets, pred_temperature, label_temperature), weight, per_image, scale)
