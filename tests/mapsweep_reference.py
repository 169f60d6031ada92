"""fs_map_list_sweep (include/flingsim.h) restated in float64 numpy, image by image and temperature by temperature, for the tests
of the kernels, of trainops.map_list_sweep_torch and of trainops.fit_temperature.  Every quantity is formed DIRECTLY from its
definition -- D_b as sum_i q_i (lq_i - ls_i) with both log-softmaxes from maplist_reference.log_softmax, the moments of s about
zero -- not from the temperature-free sums the kernel and the torch statement factor it into: the two routes share the inputs and
nothing else.  The offsets are clamped as the header states."""
import numpy as np

from maplist_reference import arg_max, log_softmax
from maploss_reference import clamp_offsets, offsets_of  # noqa: F401  (offsets_of: for the tests)


def image_sweep(p, y, temperatures, label_temperature):
    """One listed image: (rows [S, 4], image [4], draws [S, 2] = s at the arg-max of y and at the arg-max of p)."""
    p, y = np.asarray(p, np.float64), np.asarray(y, np.float64)
    chosen, best = arg_max(p), arg_max(y)
    lq = log_softmax(y / float(label_temperature), best)
    q = np.exp(lq)
    rows, draws = np.zeros((len(temperatures), 4)), np.zeros((len(temperatures), 2))
    for k, t in enumerate(temperatures):
        ls = log_softmax(p * (1.0 / float(t)), chosen)
        s = np.exp(ls)
        mean = float((s * p).sum())
        rows[k] = (float(np.where(q == 0.0, 0.0, q * (lq - ls)).sum()), mean - float((q * p).sum()),
                   float((s * (p - mean) ** 2).sum()), float((s * y).sum()))
        draws[k] = (s[best], s[chosen])
    return rows, np.array([len(p), y[best], y[chosen], float((q * p).sum())]), draws


def map_list_sweep_f64(pred, label, offsets, temperatures, label_temperature, per_image=False):
    """(curve [S, 8], rows [G, S, 4], images [G, 4]) as float64 numpy."""
    pred, label = np.asarray(pred, np.float64), np.asarray(label, np.float64)
    temperatures = np.asarray(temperatures, np.float64)
    spans = clamp_offsets(offsets, len(pred))
    S, G = len(temperatures), len(spans)
    rows, images, draws = np.zeros((G, S, 4)), np.zeros((G, 4)), np.zeros((G, S, 2))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for b, (begin, K) in enumerate(spans):
            if K >= 2:
                rows[b], images[b], draws[b] = image_sweep(pred[begin:begin + K], label[begin:begin + K], temperatures, label_temperature)
        K = images[:, 0]
        listed = K >= 2
        G_l, L_l = int(listed.sum()), int(K.sum())
        curve = np.zeros((S, 8))
        curve[:, 6], curve[:, 7] = G_l, L_l
        if G_l:
            coef = (listed / G_l if per_image else K / L_l)[:, None]
            for k in range(3):
                curve[:, k] = (coef * rows[:, :, k])[listed].sum(axis=0)
            curve[:, 3] = (images[listed, 1][:, None] - rows[listed, :, 3]).mean(axis=0)
            curve[:, 4], curve[:, 5] = draws[listed, :, 0].mean(axis=0), draws[listed, :, 1].mean(axis=0)
    return curve, rows, images


def list_at(pred, label, offsets, temperature, label_temperature, per_image=False):
    """The term at one temperature."""
    return float(map_list_sweep_f64(pred, label, offsets, [temperature], label_temperature, per_image)[0][0, 0])


def dense_minimum(pred, label, offsets, label_temperature, per_image, lo, hi, points=4001):
    """The temperature of the smallest term on a dense logarithmic grid over [lo, hi], and the grid's ratio of neighbours."""
    grid = np.exp(np.linspace(np.log(lo), np.log(hi), points))
    values = np.empty(points)
    for first in range(0, points, 64):
        values[first:first + 64] = map_list_sweep_f64(pred, label, offsets, grid[first:first + 64], label_temperature, per_image)[0][:, 0]
    return float(grid[int(np.argmin(values))]), float(grid[1] / grid[0])


def noisy_set(sign=1.0):
    """The issue's set with an interior minimum: K = 2, 63, 64, 65, 255, 256, 257, 1000; all labels first, then all predictions."""
    rng = np.random.default_rng(0)
    lengths = [2, 63, 64, 65, 255, 256, 257, 1000]
    ys = [(rng.random(K) * 0.3).astype(np.float32) for K in lengths]
    ps = [(0.5 * y + 0.05 * rng.standard_normal(len(y))).astype(np.float32) for y in ys]
    return np.float32(sign) * np.concatenate(ps), np.concatenate(ys), offsets_of(lengths)


def affine_set(a=0.5):
    """p = a y + c per image, a different c per image, formed in float64 and rounded once: the fit is a T_y."""
    rng = np.random.default_rng(1)
    lengths = [2, 7, 64, 65, 300]
    ys = [np.round(rng.random(K) * 0.3 * 64) / 64 for K in lengths]     # multiples of 1/64: a y + c is exact in float32
    ps = [a * y + c for y, c in zip(ys, (0.25, -1.0, 0.5, 2.0, -0.125))]
    return np.concatenate(ps).astype(np.float32), np.concatenate(ys).astype(np.float32), offsets_of(lengths)
