"""fs_observe_frames (csrc/fs_observe.hip) on synthetic frames against oracle/observe.py, bit for bit.

Through fs_observe the stage only ever sees what the rasteriser draws: a cloth-coloured blob on a uniform floor, square
frames, a nearly constant depth plane.  Here the frames are made in the test -- every 8-bit colour, full-range noise and
stripes at sizes that are neither square nor multiples of anything, depth over sixty orders of magnitude, and mask shapes
chosen against the labelling passes (long paths, diagonal-only contacts, ties between equally large components).  Compared,
with uint32 views for the floats: obs[:3], obs[3], the whole label plane (include/flingsim.h: -1 or the raster index of the
component's first pixel; the reference is scipy.ndimage.label with the full 3 x 3 structure, every component mapped to its
first raster index), the mask, the bounding box and the pixel count.

The oracle itself is held against exact float64 definitions by the tests that carry no gpu mark."""
import numpy as np
import pytest
from scipy import ndimage

from conftest import cloth_params

gpu = pytest.mark.gpu

BG, FG = (30, 30, 30), (255, 255, 255)   # v = 30: inside inRange, not cloth; v = 255: cloth


# ---------------------------------------------------------------- references
def _canonical_labels(raw):
    """-1 where raw == 0, else the raster index of the first pixel of the pixel's 8-connected component."""
    lab, n = ndimage.label(raw, structure=np.ones((3, 3), int))
    u, first = np.unique(lab.ravel(), return_index=True)
    table = np.full(n + 1, -1, np.int64)
    table[u] = first
    table[0] = -1
    return table[lab].astype(np.int32)


def _reference(rgba, depth, S):
    """(obs, labels, mask, bbox) of one bottom-up frame rgba uint8 [H, W, 4], depth float32 [H, W]."""
    from oracle import observe as oo

    h, w = depth.shape
    obs, rgb, d, mask, crop = oo.get_obs(rgba.ravel(), depth.ravel(), (h, w), S)
    labels = _canonical_labels(oo.cloth_mask_raw(rgb))
    if mask is None:
        return obs, labels, np.zeros((S, S), np.uint8), [-1, -1, -1, -1, 0]
    x, y = np.where(mask)
    return obs, labels, mask, [int(x.min()), int(x.max()), int(y.min()), int(y.max()), int(mask.sum())]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _observe(ctx, frames, S, want_mask=True):
    """frames: list of (rgba [H, W, 4] uint8, depth [H, W] float32) numpy arrays -> numpy (obs, bbox, mask, labels)."""
    import torch

    # (a fresh copy: a flipped view with one row counts as contiguous and keeps its negative stride, which torch refuses)
    rgba = [torch.from_numpy(np.array(c, np.uint8, order="C")).cuda() for c, _ in frames]
    depth = [torch.from_numpy(np.array(d, np.float32, order="C")).cuda() for _, d in frames]
    out = ctx.observe_frames(rgba, depth, S, want_mask=want_mask)
    labels = ctx.observe_labels(len(frames), S).cpu().numpy()
    return out[0].cpu().numpy(), out[1], (out[2].cpu().numpy() if want_mask else None), labels


def _assert_frame(tag, got_obs, got_bbox, got_mask, got_labels, frame, S):
    ref_obs, ref_labels, ref_mask, ref_bbox = _reference(frame[0], frame[1], S)
    assert got_obs.shape == (4, S, S)
    assert np.array_equal(_bits(got_obs[:3]), _bits(ref_obs[:3])), (tag, "rgb planes")
    assert np.array_equal(_bits(got_obs[3]), _bits(ref_obs[3])), (tag, "depth plane")
    assert np.array_equal(got_labels, ref_labels), (tag, "labels", int((got_labels != ref_labels).sum()))
    if got_mask is not None:
        assert np.array_equal(got_mask, ref_mask), (tag, "mask")
    assert list(got_bbox) == ref_bbox, (tag, "bbox / count", list(got_bbox), ref_bbox)


def _check(ctx, frames, S, tags):
    obs, bbox, mask, labels = _observe(ctx, frames, S)
    assert obs.shape[0] == bbox.shape[0] == mask.shape[0] == labels.shape[0] == len(frames)
    for k, f in enumerate(frames):
        _assert_frame((tags[k], S), obs[k], bbox[k], mask[k], labels[k], f, S)


# ---------------------------------------------------------------- inputs
def _colour_frame(k):
    """Frame k of 16: the colours k * 2^20 ... (k + 1) * 2^20 - 1 (0xRRGGBB) in raster order of a 1024 x 1024 frame."""
    idx = (np.arange(1 << 20, dtype=np.uint32) + (np.uint32(k) << 20)).reshape(1024, 1024)
    rgba = np.stack([(idx >> 16) & 255, (idx >> 8) & 255, idx & 255, np.full_like(idx, 255)], -1).astype(np.uint8)
    return rgba


def _depth(rng, h, w):
    """finite float32: a depth-like plane with exact zeros, negatives and magnitudes from 1e-10 to 1e30 of either sign"""
    d = 1.9 + 0.1 * rng.rand(h, w)
    kind = rng.rand(h, w)
    d[kind < 0.1] = 0.0
    neg = (kind >= 0.1) & (kind < 0.2)
    d[neg] = -d[neg]
    big = kind >= 0.7
    d[big] = (10.0 ** rng.uniform(-10, 30, (h, w)) * rng.choice([-1.0, 1.0], (h, w)))[big]
    d = d.astype(np.float32)
    assert np.isfinite(d).all()
    return d


def _noise_frame(rng, h, w):
    return rng.randint(0, 256, (h, w, 4)).astype(np.uint8), _depth(rng, h, w)


def _stripe_frame(rng, h, w):
    """0 / 255 stripes one and two pixels wide, along both axes and crossed"""
    y, x = np.mgrid[:h, :w]
    chans = [(x % 2) ^ ((y // 2) % 2), (x // 2) % 2, y % 2, np.ones_like(x)]
    return (np.stack(chans, -1) * 255).astype(np.uint8), _depth(rng, h, w)


def _threshold_frame(rng, h, w):
    """smooth colour ramps around the h, s, v <= 100 thresholds: big regions on either side of the cloth test"""
    y, x = np.mgrid[:h, :w]
    v = 80 + (40 * x) // max(w - 1, 1)                       # 80 .. 120
    lo = (v * (120 + (80 * y) // max(h - 1, 1))) // 255      # saturation ~ 0.2 .. 0.53 -> s ~ 55 .. 135
    rgb = np.stack([v, lo + rng.randint(0, 3, (h, w)), lo, np.full_like(v, 7)], -1)
    return np.clip(rgb, 0, 255).astype(np.uint8), _depth(rng, h, w)


def _frame_of_mask(mask, rng=None, size=None):
    """The bottom-up two-colour frame whose observation shows `mask` (rows top-down); size (H, W): nearest-enlarged first."""
    m = np.asarray(mask, bool)
    if size is not None:
        h, w = size
        m = m[(np.arange(h) * m.shape[0]) // h][:, (np.arange(w) * m.shape[1]) // w]
    rgba = np.where(m[:, :, None], np.array(FG + (255,), np.uint8), np.array(BG + (0,), np.uint8)).astype(np.uint8)
    d = _depth(rng, *m.shape) if rng is not None else np.full(m.shape, 1.95, np.float32)
    return rgba[::-1].copy(), d[::-1].copy()


def _serpentine(S):
    m = np.zeros((S, S), bool)
    m[0::2] = True
    for k, r in enumerate(range(1, S - 1, 2)):
        m[r, S - 1 if k % 2 == 0 else 0] = True
    return m


def _spiral(S):
    """a rectangular spiral, one pixel wide, one pixel between its arms, from the top-left corner inwards"""
    m = np.zeros((S, S), bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    turns = 0
    while turns < 2:
        ny, nx = y + dy, x + dx
        ay, ax = y + 2 * dy, x + 2 * dx
        if not (0 <= ny < S and 0 <= nx < S) or m[ny, nx] or (0 <= ay < S and 0 <= ax < S and m[ay, ax]):
            dy, dx = dx, -dy
            turns += 1
            continue
        y, x = ny, nx
        m[y, x] = True
        turns = 0
    return m


def _blocks(S, boxes):
    m = np.zeros((S, S), bool)
    for (y0, x0, h, w) in boxes:
        assert 0 <= y0 and y0 + h <= S and 0 <= x0 and x0 + w <= S
        m[y0:y0 + h, x0:x0 + w] = True
    return m


def _label_shapes(S):
    """{name: mask [S, S]} of the shapes that fit into S x S"""
    yy, xx = np.mgrid[:S, :S]
    out = {
        "serpentine": _serpentine(S),
        "serpentine_flipped": _serpentine(S)[::-1],      # the root is at the far end of the path
        "spiral": _spiral(S),
        "spiral_flipped": _spiral(S)[::-1, ::-1],
        "checkerboard": (yy + xx) % 2 == 0,              # ONE component under 8-connectivity
        "diagonal": yy == xx,
        "antidiagonal": yy + xx == S - 1,
        "border_ring": (yy == 0) | (xx == 0) | (yy == S - 1) | (xx == S - 1),
        "corners": ((yy == 0) | (yy == S - 1)) & ((xx == 0) | (xx == S - 1)),
        "all_foreground": np.ones((S, S), bool),
        "all_background": np.zeros((S, S), bool),
    }
    if S >= 9:
        # 2 x 2 blobs on a pitch of 3 (17 689 of them at S = 400); the last one in raster order is 2 x 3 and must win
        nb = (S - 1) // 3
        m = np.zeros((S, S), bool)
        for dy in (0, 1):
            for dx in (0, 1):
                m[dy:3 * nb:3, dx:3 * nb:3] = True
        m[3 * (nb - 1):3 * (nb - 1) + 2, 3 * (nb - 1) + 2] = True
        out["blobs_last_wins"] = m
    if S >= 15:
        # equally large components: the first in raster order wins
        out["tie_two"] = _blocks(S, [(1, 8, 3, 3), (6, 2, 3, 3)])
        out["tie_three"] = _blocks(S, [(5, 9, 2, 4), (1, 3, 4, 2), (10, 0, 1, 8)])
        # ... also when the later one has the smaller column range in every row it occupies (a line far right, then a
        # square far left), and when both start in the same row
        out["tie_later_is_left"] = _blocks(S, [(2, S - 9, 1, 9), (5, 0, 3, 3)])
        out["tie_same_row"] = _blocks(S, [(3, 1, 2, 3), (3, S - 4, 3, 2)])
        # two 3 x 3 blobs that touch at one corner only make one component of 18; a lone 2 x 5 comes first in raster order
        out["diagonal_contact"] = _blocks(S, [(0, S - 5, 2, 5), (4, 1, 3, 3), (7, 4, 3, 3)])
        out["antidiagonal_contact"] = _blocks(S, [(0, 0, 2, 5), (4, 6, 3, 3), (7, 3, 3, 3)])
    return out


# ---------------------------------------------------------------- the oracle against exact definitions (CPU)
def test_oracle_hsv_against_the_exact_definition_for_every_colour():
    """oracle/observe.py rgb2hsv_u8 (OpenCV's 12-bit fixed-point tables) against HSV in float64, for all 2^24 colours.
    Measured: max |s - exact| 0.53, max circular |h - exact| 0.64, 50 classifications differ from the one made with
    exactly rounded h, s (round half to even)."""
    from oracle import observe as oo

    worst_s = worst_h = 0.0
    differ = 0
    for k in range(16):
        rgb = _colour_frame(k)[:, :, :3].reshape(-1, 3)
        hsv = oo.rgb2hsv_u8(rgb).astype(np.float64)
        r, g, b = (rgb[:, c].astype(np.float64) for c in range(3))
        v = np.maximum(np.maximum(r, g), b)
        diff = v - np.minimum(np.minimum(r, g), b)
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.where(v > 0, 255.0 * diff / v, 0.0)
            h = np.where(v == r, (g - b) / diff, np.where(v == g, 2.0 + (b - r) / diff, 4.0 + (r - g) / diff)) * 30.0
        h = np.where(diff > 0, h, 0.0)
        h = np.where(h < 0, h + 180.0, h)
        assert np.array_equal(hsv[:, 2], v)
        worst_s = max(worst_s, float(np.abs(hsv[:, 1] - s).max()))
        dh = np.abs(hsv[:, 0] - h)
        worst_h = max(worst_h, float(np.minimum(dh, 180.0 - dh).max()))
        exact = ~((np.rint(h) % 180 <= 100) & (np.rint(s) <= 100) & (v <= 100))
        differ += int((exact != (oo.cloth_mask_raw(rgb[None])[0] == 1)).sum())
    print(f"hsv oracle: max |s - exact| {worst_s:.3f}, max circular |h - exact| {worst_h:.3f}, {differ} classifications differ")
    assert worst_s < 1.0        # measured 0.53
    assert worst_h < 1.0        # measured 0.64
    assert differ <= 64         # measured 50 of 16 777 216


RESIZE_SHAPES = [(720, 720, 400), (720, 480, 400), (480, 720, 128), (400, 400, 200), (200, 200, 400), (97, 211, 64),
                 (64, 300, 64), (5, 3, 77), (1, 1, 9), (4096, 16, 33), (300, 300, 1)]   # (W, H, S)


def _resize_frames(W, H, seed):
    rng = np.random.RandomState(seed)
    return [_noise_frame(rng, H, W), _stripe_frame(rng, H, W), _threshold_frame(rng, H, W)], ["noise", "stripes", "thresholds"]


@pytest.mark.parametrize("W,H,S", RESIZE_SHAPES)
def test_oracle_resize_against_float64_bilinear(W, H, S):
    """oracle/observe.py's resizes against bilinear interpolation in float64 with the same taps: the 11-bit fixed-point
    path within 1 grey level (measured 0.80), the float path within 4 float32 ulps of the largest tap (measured 2.1)."""
    from oracle import observe as oo

    sx, fx = oo._linear_taps(S, W)
    sy, fy = oo._linear_taps(S, H)
    sx1, sy1 = np.minimum(sx + 1, W - 1), np.minimum(sy + 1, H - 1)
    fx, fy = fx.astype(np.float64)[None, :], fy.astype(np.float64)[:, None]

    def exact(a):   # a [H, W] float64
        top = a[sy][:, sx] * (1 - fx) + a[sy][:, sx1] * fx
        bot = a[sy1][:, sx] * (1 - fx) + a[sy1][:, sx1] * fx
        return top * (1 - fy) + bot * fy

    worst8 = worstf = 0.0
    for (rgba, depth), tag in zip(*_resize_frames(W, H, seed=W * 7 + H * 3 + S)):
        got = oo.resize_linear_u8(rgba[:, :, :3], S).astype(np.float64)
        for c in range(3):
            worst8 = max(worst8, float(np.abs(got[:, :, c] - exact(rgba[:, :, c].astype(np.float64))).max()))
        d64 = depth.astype(np.float64)
        gotd = oo.resize_linear_f32(depth, S)
        assert gotd.dtype == np.float32 and np.isfinite(gotd).all()
        mag = np.abs(d64)
        tapmax = np.maximum(np.maximum(mag[sy][:, sx], mag[sy][:, sx1]), np.maximum(mag[sy1][:, sx], mag[sy1][:, sx1]))
        ulp = np.spacing(np.maximum(tapmax, np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
        worstf = max(worstf, float((np.abs(gotd.astype(np.float64) - exact(d64)) / ulp).max()))
    print(f"resize oracle {W}x{H}->{S}: u8 max |diff| {worst8:.3f}, depth max {worstf:.2f} ulp of the largest tap")
    assert worst8 <= 1.0
    assert worstf <= 4.0


def test_oracle_get_obs_takes_a_size_pair():
    from oracle import observe as oo

    rng = np.random.RandomState(5)
    rgba, depth = _noise_frame(rng, 12, 12)
    a, b = oo.get_obs(rgba.ravel(), depth.ravel(), 12, 8), oo.get_obs(rgba.ravel(), depth.ravel(), (12, 12), 8)
    assert all(np.array_equal(p, q) for p, q in zip(a[:4], b[:4])) and a[4] == b[4]
    rgba, depth = _noise_frame(rng, 5, 9)
    obs = oo.get_obs(rgba.ravel(), depth.ravel(), (5, 9), 5)[0]
    assert obs.shape == (4, 5, 5)
    assert np.array_equal(obs[0, 0], oo.resize_linear_u8(rgba[::-1, :, :3].copy(), 5)[0, :, 0].astype(np.float32) / np.float32(255))


def test_label_shapes_are_what_they_claim():
    """The masks the labelling cases are built from, checked with scipy alone: component counts, sizes and winners."""
    from oracle import observe as oo

    eight = np.ones((3, 3), int)
    for S in (15, 16, 63, 65, 77, 257, 400):
        sh = _label_shapes(S)
        for name in ("serpentine", "serpentine_flipped", "spiral", "spiral_flipped", "checkerboard", "diagonal",
                     "antidiagonal", "border_ring", "all_foreground"):
            assert ndimage.label(sh[name], eight)[1] == 1, (S, name)
        assert ndimage.label(sh["checkerboard"])[1] == (S * S + 1) // 2      # 4-connectivity: every pixel on its own
        assert ndimage.label(sh["diagonal"])[1] == S
        assert sh["serpentine"].sum() > S * S // 2 and sh["spiral"].sum() > S * S // 2 - 2 * S
        assert ndimage.label(sh["corners"], eight)[1] == 4
        lab, n = ndimage.label(sh["blobs_last_wins"], eight)
        sizes = np.bincount(lab.ravel())[1:]
        assert n == ((S - 1) // 3) ** 2 and sizes[-1] == 6 and (sizes[:-1] == 4).all()
        for name, k in (("tie_two", 2), ("tie_three", 3), ("tie_later_is_left", 2), ("tie_same_row", 2)):
            lab, n = ndimage.label(sh[name], eight)
            sizes = np.bincount(lab.ravel())[1:]
            assert n == k and len(set(sizes.tolist())) == 1, (S, name)
            assert np.array_equal(oo.largest_component(sh[name]), lab == 1), (S, name)
        for name in ("diagonal_contact", "antidiagonal_contact"):
            lab, n = ndimage.label(sh[name], eight)
            assert n == 2 and np.bincount(lab.ravel())[1:].tolist() == [10, 18], (S, name)
            assert ndimage.label(sh[name])[1] == 3                           # 4-connectivity would let the 10 win
    later = _label_shapes(40)["tie_later_is_left"]
    rows = np.where(later.any(1))[0]
    assert later[rows[-1]].nonzero()[0].max() < later[rows[0]].nonzero()[0].min()


# ---------------------------------------------------------------- the device path
@pytest.fixture(scope="module")
def ctx(gpu_required):
    from flingbot_amd import sim as fsim

    c = fsim.FlingSim(n_envs=1, solver=0)
    yield c
    c.close()


@gpu
def test_every_colour(ctx):
    """All 2^24 colours through the identity-size path, 16 frames of 1024 x 1024 in one call: the label plane is >= 0 exactly
    where the oracle's colour test says cloth, and everything else equals the reference too."""
    from oracle import observe as oo

    rng = np.random.RandomState(24)
    frames = [(_colour_frame(k), _depth(rng, 1024, 1024)) for k in range(16)]
    obs, bbox, mask, labels = _observe(ctx, frames, 1024)
    for k, f in enumerate(frames):
        raw = oo.cloth_mask_raw(f[0][::-1, :, :3])
        assert np.array_equal(labels[k] >= 0, raw == 1), k
        _assert_frame(("colours", k), obs[k], bbox[k], mask[k], labels[k], f, 1024)


@gpu
@pytest.mark.parametrize("W,H,S", RESIZE_SHAPES)
def test_resize_arithmetic(ctx, W, H, S):
    frames, tags = _resize_frames(W, H, seed=W * 7 + H * 3 + S)
    assert (W == S and H == S) is False
    _check(ctx, frames, S, tags)


@gpu
@pytest.mark.parametrize("S", [1, 2, 15, 16, 63, 65, 77, 257, 400])
def test_labelling_shapes(ctx, S):
    """Every shape of _label_shapes at identity size, and once enlarged 1.8 times so that it comes back through the resize
    (grey edges on both sides of the v <= 100 threshold; the oracle says what the mask is then)."""
    shapes = _label_shapes(S)
    rng = np.random.RandomState(S)
    names = list(shapes)
    _check(ctx, [_frame_of_mask(shapes[n], rng) for n in names], S, names)
    big = max(int(round(1.8 * S)), S + 1)
    _check(ctx, [_frame_of_mask(shapes[n], rng, size=(big, big)) for n in names], S, [n + "/1.8x" for n in names])
    if S >= 15:  # the winner of a tie, spelled out rather than left to the reference: the first in raster order
        obs, bbox, mask, labels = _observe(ctx, [_frame_of_mask(shapes[n]) for n in ("tie_two", "tie_later_is_left")], S)
        assert bbox[0].tolist() == [1, 3, 8, 10, 9] and bbox[1].tolist() == [2, 2, S - 9, S - 1, 9]


def _batch_frames(S=200):
    rng = np.random.RandomState(12)
    frames, tags = [], []

    def add(tag, f):
        frames.append(f)
        tags.append(tag)

    add("empty", _frame_of_mask(np.zeros((S, S), bool), rng))
    add("serpentine", _frame_of_mask(_serpentine(S), rng))
    add("colours7", (_colour_frame(7), _depth(rng, 1024, 1024)))
    add("spiral_big", _frame_of_mask(_spiral(S), rng, size=(330, 410)))
    add("noise_wide", _noise_frame(rng, 120, 640))
    add("noise_tall", _noise_frame(rng, 333, 77))
    add("thresholds", _threshold_frame(rng, 256, 300))
    add("stripes", _stripe_frame(rng, 200, 201))
    add("blobs", _frame_of_mask(_label_shapes(S)["blobs_last_wins"], rng))
    add("checkerboard", _frame_of_mask(_label_shapes(S)["checkerboard"], rng))
    add("serpentine_flipped_small", _frame_of_mask(_serpentine(61)[::-1], rng, size=(150, 180)))
    add("one_pixel", _frame_of_mask(np.ones((1, 1), bool), rng))
    assert len(frames) == 12
    return frames, tags


@gpu
def test_batch_mixed_sizes_permutation_and_single_calls(ctx):
    S = 200
    frames, tags = _batch_frames(S)
    obs, bbox, mask, labels = _observe(ctx, frames, S)
    for k, f in enumerate(frames):
        _assert_frame((tags[k], S), obs[k], bbox[k], mask[k], labels[k], f, S)
    assert bbox[0].tolist() == [-1, -1, -1, -1, 0] and (bbox[1:, 4] > 0).all()
    perm = [7, 2, 11, 0, 5, 9, 1, 10, 3, 8, 6, 4]
    pobs, pbbox, pmask, plabels = _observe(ctx, [frames[p] for p in perm], S)
    for k, p in enumerate(perm):
        assert np.array_equal(_bits(pobs[k]), _bits(obs[p])) and np.array_equal(pmask[k], mask[p]), tags[p]
        assert np.array_equal(plabels[k], labels[p]) and pbbox[k].tolist() == bbox[p].tolist(), tags[p]
    for k, f in enumerate(frames):
        o1, b1, m1, l1 = _observe(ctx, [f], S)
        assert np.array_equal(_bits(o1[0]), _bits(obs[k])) and np.array_equal(m1[0], mask[k]), tags[k]
        assert np.array_equal(l1[0], labels[k]) and b1[0].tolist() == bbox[k].tolist(), tags[k]


@gpu
def test_batch_of_192_small_frames(ctx):
    import torch

    S, n = 64, 192
    rng = np.random.RandomState(192)
    shapes = list(_label_shapes(S).values())
    frames = []
    for k in range(n):
        if k % 3 == 0:
            frames.append(_frame_of_mask(shapes[(k // 3) % len(shapes)], rng))
        elif k % 3 == 1:
            m = ndimage.uniform_filter(rng.rand(S, S), 5) > 0.5 + 0.02 * rng.randn()     # blobs of all sizes
            frames.append(_frame_of_mask(m, rng))
        else:
            frames.append(_noise_frame(rng, 50 + k % 31, 40 + k % 47))
    obs, bbox, mask, labels = _observe(ctx, frames, S)
    for k, f in enumerate(frames):
        _assert_frame((k, S), obs[k], bbox[k], mask[k], labels[k], f, S)
    obs2, bbox2, _, labels2 = _observe(ctx, frames, S, want_mask=False)
    assert np.array_equal(bbox2, bbox) and np.array_equal(labels2, labels) and np.array_equal(_bits(obs2), _bits(obs))
    # the stacked-tensor form of the same call (equal sizes)
    same = [f for f in frames if f[1].shape == (S, S)]
    rgba = torch.from_numpy(np.stack([f[0] for f in same])).cuda()
    depth = torch.from_numpy(np.stack([f[1] for f in same])).cuda()
    obs3, bbox3 = ctx.observe_frames(rgba, depth, S)
    pick = [k for k, f in enumerate(frames) if f[1].shape == (S, S)]
    assert np.array_equal(bbox3, bbox[pick]) and np.array_equal(_bits(obs3.cpu().numpy()), _bits(obs[pick]))


@gpu
@pytest.mark.parametrize("render_dim,image_dim", [(300, 77), (256, 256)])
def test_rendered_frame_gives_what_observe_gives(gpu_required, render_dim, image_dim):
    """observe(e, S) equals observe_frames on ctx.render(e) uploaded again: the new entry and the old one are one path."""
    import torch
    from flingbot_amd import sim as fsim

    c = fsim.FlingSim(n_envs=1, solver=0)
    env = c.env(0)
    env.set_scene(cloth_params(40, 30, pos=(0.0, 0.3, 0.0)))
    rng = np.random.RandomState(0)
    p = env.get_positions().reshape(-1, 4)
    p[:, :3] += rng.randn(*p[:, :3].shape).astype(np.float32) * 0.004
    env.set_positions(p.ravel())
    c.step(25)
    cp = c.get_camera_params(0)
    c.set_camera_params(0, [*cp[2:8], render_dim, render_dim])
    rgba, depth = c.render(0)
    obs, bbox, mask = c.observe(0, image_dim, want_mask=True)
    lab = c.observe_labels(1, image_dim).cpu().numpy()
    assert bbox[4] > 0
    fr = torch.from_numpy(rgba.reshape(1, render_dim, render_dim, 4)).cuda()
    fd = torch.from_numpy(depth.reshape(1, render_dim, render_dim)).cuda()
    obs2, bbox2, mask2 = c.observe_frames(fr, fd, image_dim, want_mask=True)
    assert np.array_equal(_bits(obs2[0].cpu().numpy()), _bits(obs.cpu().numpy()))
    assert np.array_equal(mask2[0].cpu().numpy(), mask.cpu().numpy()) and bbox2[0].tolist() == bbox.tolist()
    assert np.array_equal(c.observe_labels(1, image_dim).cpu().numpy(), lab)
    c.close()


@gpu
def test_argument_errors(ctx):
    import ctypes as C
    import torch

    FS_ERR_ARG = -1   # include/flingsim.h
    rng = np.random.RandomState(1)
    rgba, depth = _noise_frame(rng, 8, 8)
    c, d = torch.from_numpy(rgba).cuda(), torch.from_numpy(depth).cuda()
    obs = torch.empty((4, 8, 8), device="cuda")
    work = torch.empty(int(ctx.lib.fs_observe_work_bytes(8)), dtype=torch.uint8, device="cuda")
    bbox = np.zeros(5, np.int32)
    torch.cuda.synchronize()
    pc, pd = (C.c_void_p * 1)(c.data_ptr()), (C.c_void_p * 1)(d.data_ptr())
    null = (C.c_void_p * 1)(None)
    ip = C.POINTER(C.c_int)

    def call(n=1, pc=pc, pd=pd, w=8, h=8, S=8, o=obs.data_ptr(), b=bbox, wk=work.data_ptr(), sizes=True):
        ws, hs = np.array([w], np.int32), np.array([h], np.int32)
        return ctx.lib.fs_observe_frames(ctx.h, n, pc, pd, ws.ctypes.data_as(ip) if sizes else None, hs.ctypes.data_as(ip),
                                         S, C.c_void_p(o), None, b.ctypes.data_as(ip) if b is not None else None,
                                         C.c_void_p(wk))

    assert call() == 0
    for bad in (dict(n=0), dict(n=-1), dict(pc=None), dict(pd=None), dict(pc=null), dict(pd=null), dict(sizes=False),
                dict(w=0), dict(h=0), dict(w=4097), dict(h=4097), dict(S=0), dict(S=4097), dict(o=None), dict(b=None),
                dict(wk=None)):
        assert call(**bad) == FS_ERR_ARG, bad
        assert b"fs_observe_frames" in ctx.lib.fs_last_error(), bad
    with pytest.raises(AssertionError):
        ctx.observe_frames([c], [d[:4]], 8)
