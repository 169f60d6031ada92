"""The rules of fs_value_range / fs_action_panels (include/flingsim.h) restated in numpy -- the reference the kernels are
compared with byte for byte (tests/test_report_gpu.py).  Not a test module.

The code has another shape than the kernel on purpose: a whole image at a time, one boolean mask per primitive over the
source image, np.float32 arrays for the colour index, integer index vectors for the sampling."""
import numpy as np

RING, SEGMENT = 0, 1
_f32 = np.float32


def value_range(values):
    """(vmin, vmax) as float32 over the finite entries of `values`; (0, 0) when there is none; zeros as +0.0."""
    v = np.asarray(values, _f32).ravel()
    v = v[np.isfinite(v)]
    if v.size == 0:
        return np.zeros(2, _f32)
    return np.array([v.min(), v.max()], _f32) + _f32(0.0)


def quantize(planes):
    """trunc(clamp(x * 255, 0, 255)) in float32; a NaN gives 0 (fmax / fmin return the number)."""
    x = np.asarray(planes, _f32) * _f32(255.0)
    return np.trunc(np.fmin(np.fmax(x, _f32(0.0)), _f32(255.0))).astype(np.uint8)


def image_of(planes):
    """float32 [>= 3, H, W] -> uint8 [H, W, 3]"""
    return quantize(np.asarray(planes)[:3]).transpose(1, 2, 0)


def jet(table, value_map, vmin, vmax):
    """uint8 [D, D, 3]: entry clamp(int(t * 256), 0, 255) of `table`, t = (v - vmin) / (vmax - vmin) in float32; entry 0 where
    vmax == vmin, v is not finite or t is NaN."""
    v = np.asarray(value_map, _f32)
    vmin, vmax = _f32(vmin), _f32(vmax)
    with np.errstate(all="ignore"):
        t = (v - vmin) / (vmax - vmin)          # float32 arrays: one rounding per operation
        f = t * _f32(256.0)
    index = np.zeros(v.shape, np.int64)
    inside = (f > 0) & (f < 255)
    index[inside] = np.trunc(f[inside]).astype(np.int64)
    index[f >= 255] = 255
    if vmax == vmin:
        index[:] = 0
    index[~np.isfinite(v)] = 0
    return np.asarray(table, np.uint8)[index]


def mask_of(prim, size):
    """bool [size, size]: the source pixels one primitive covers (python integers / int64 throughout)."""
    kind, y0, x0, y1, x1, t = (int(c) for c in prim[:6])
    py, px = np.meshgrid(np.arange(size, dtype=np.int64), np.arange(size, dtype=np.int64), indexing="ij")
    if kind == RING:
        d4 = 4 * ((py - y0) ** 2 + (px - x0) ** 2)
        return ((2 * y1 - t) ** 2 <= d4) & (d4 <= (2 * y1 + t) ** 2)
    assert kind == SEGMENT
    vy, vx = y1 - y0, x1 - x0
    wy, wx = py - y0, px - x0
    length = vy * vy + vx * vx
    along = wy * vy + wx * vx
    near_a = 4 * (wy ** 2 + wx ** 2) <= t * t
    near_b = 4 * ((py - y1) ** 2 + (px - x1) ** 2) <= t * t
    beside = 4 * (wy * vx - wx * vy) ** 2 <= t * t * length
    return np.where(along <= 0, near_a, np.where(along >= length, near_b, beside))


def draw(image, prims):
    """uint8 [H, H, 3] with the primitives on it: the last primitive that covers a pixel gives its colour, blended once,
    (9 * colour + base + 5) // 10."""
    size = image.shape[0]
    colour = np.zeros((size, size, 3), np.int64)
    covered = np.zeros((size, size), bool)
    for prim in prims:
        m = mask_of(prim, size)
        colour[m] = np.asarray(prim[6:9], np.int64)
        covered |= m
    out = image.astype(np.int64)
    out[covered] = (9 * colour[covered] + out[covered] + 5) // 10
    return out.astype(np.uint8)


def sample(image, panel):
    """nearest sampling of a square image to panel x panel: source index = (dst * size) // panel per axis"""
    idx = (np.arange(panel, dtype=np.int64) * image.shape[0]) // panel
    return image[idx][:, idx]


def strip(table, stack, value_map, vrange, before, after, small, large, panel):
    """uint8 [panel, 5 * panel, 3]: before | value map | transformed RGB + action | before + action | after"""
    b = image_of(before)
    last = np.zeros_like(b) if after is None else image_of(after)
    parts = [b, jet(table, value_map, vrange[0], vrange[1]), draw(image_of(stack), small), draw(b, large), last]
    return np.concatenate([sample(p, panel) for p in parts], axis=1)
