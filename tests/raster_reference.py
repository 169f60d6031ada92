"""Independent reference of the software rasteriser (TEST INFRASTRUCTURE; numpy and Python only).

Written from the rules stated in the header of csrc/fs_raster_kernels.h, not from its code:

  * pixel centres at (px + 1/2, py + 1/2), rows bottom-up; window coordinates snapped to 1/256 pixel (round to nearest even);
  * a centre is covered when it lies inside the snapped triangle; a centre ON an edge belongs to the triangle that contains
    the point an infinitesimal step to +x and then an infinitesimally smaller step to -y away from it (that IS the top-left
    rule: left edges and top edges own their centres) -- formulated on the sample, so it does not care about the winding;
  * cloth is two-sided, sphere meshes are culled when they face away from the camera (not in the light's pass);
  * a triangle with a vertex at clip w <= 1e-6 (or a window coordinate beyond 1e6) is dropped whole: no near clipping;
  * depth is the barycentric (affine in window space) mix of the vertices' window depths, discarded outside [0, 1],
    quantised to 24 bits with floor(d (2^24 - 1) + 1/2); the pixel goes to the smallest (depth24, id), ids in draw order
    (ground 0, sphere triangles, cloth triangles);
  * the shadow map is the same raster at 2048^2 through the light's matrix with the polygon offset
    8 max(|dz/dx|, |dz/dy|) + 8 2^-24 of the triangle's depth plane, clamped at 1, dropped below 0;
  * shading as in the reference's solid shader (see shade()).

Two things ARE restated, because their float32 rounding decides integers: the vertex stage (clip coordinates, window x / y,
window depth, in float32 in the kernel's operation order; numpy float32 reproduces a build without contraction) and the
ground plane's per-pixel ray (same reason: its window depth sits where float32 has a resolution of one depth24 step).
tests/test_raster_reference_cpu.py bounds both against float64.

Everything after the vertex stage is EXACT: edge functions in int64 (|coordinates| < 2^28, products < 2^58), depths as Python
integers over a power-of-two denominator.  The kernel evaluates the same rationals in double, which can move a depth by
about 1e-9 of a depth24 step; every pixel therefore reports how far (in steps) the nearest exact candidate value lies from
a rounding or discard boundary (`margin`), and a comparison may leave out pixels below MARGIN_LSB.
"""
from fractions import Fraction

import numpy as np

SHADOW_RES = 2048
DEPTH_MAX = (1 << 24) - 1
CLEARED_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
CLEARED_TEXEL = np.uint32(0xFFFFFFFF)
MARGIN_LSB = 1e-6  # three orders above what double rounding moves; the smallest margin on the committed scenes is 2e-6
ZNEAR, ZFAR, FOG = np.float32(0.01), np.float32(3.0), np.float32(0.005)
F32 = np.float32

PCF_TAPS = np.array([[-0.326212, -0.40581], [-0.840144, -0.07358], [-0.695914, 0.457137], [-0.203345, 0.620716],
                     [0.96234, -0.194983], [0.473434, -0.480026], [0.519456, 0.767022], [0.185461, -0.893124],
                     [0.507431, 0.064425], [0.89642, 0.412458], [-0.32194, -0.932615], [-0.791559, -0.59771]])
COL_PLANE = np.array([0.001, 0.001, 0.001])
COL_SHAPE = np.array([0.9, 0.9, 0.9])
COL_CLOTH = np.array([0.612 * 1.5, 0.194 * 1.5, 0.394 * 1.5])
BIAS_SHAPE = 0.05


# ------------------------------------------------------------------------------------------------ vertex stage (float32)
def mat_mul32(a, b):
    """a b for row-major 4x4 float32, each entry summed over k = 0..3 from 0 (the order the frame set-up uses)."""
    a, b = np.asarray(a, F32).reshape(4, 4), np.asarray(b, F32).reshape(4, 4)
    o = np.zeros((4, 4), F32)
    for k in range(4):
        o = o + a[:, k:k + 1] * b[k:k + 1, :]
    return o


def xform32(m, p):
    """clip = m (p, 1), each row m0 x + m1 y + m2 z + m3 from left to right in float32.  p: [n, 3] -> [n, 4]."""
    m, p = np.asarray(m, F32).reshape(4, 4), np.asarray(p, F32)
    x, y, z = p[:, 0:1], p[:, 1:2], p[:, 2:3]
    return ((m[:, 0] * x + m[:, 1] * y) + m[:, 2] * z) + m[:, 3]


def vertex_stage(m, W, H, p):
    """The float32 vertex stage: dict(ok, X, Y (int64, 1/256 pixel), d (float32 window depth), w (float32 clip w), fx, fy)."""
    with np.errstate(all="ignore"):
        c = xform32(m, p)
        w = c[:, 3]
        ok = w > F32(1e-6)
        inv = F32(1.0) / np.where(ok, w, F32(1.0))
        half = F32(0.5)
        fx = (c[:, 0] * inv * half + half) * F32(W)
        fy = (c[:, 1] * inv * half + half) * F32(H)
        ok = ok & (np.abs(fx) < F32(1.0e6)) & (np.abs(fy) < F32(1.0e6))
        d = c[:, 2] * inv * half + half
        X = np.rint(np.where(ok, fx, 0) * F32(256.0)).astype(np.int64)
        Y = np.rint(np.where(ok, fy, 0) * F32(256.0)).astype(np.int64)
    return dict(ok=ok, X=X, Y=Y, d=d.astype(F32), w=w.astype(F32), fx=fx, fy=fy)


def vertex_stage64(m, W, H, p):
    """The same stage in float64 from the same float32 inputs, with the bound its float32 form must keep.

    Per clip coordinate c = m0 x + m1 y + m2 z + m3: three products and three sums, each rounded once (u = 2^-24 relative
    to its own result, every partial result <= S = |m0 x| + |m1 y| + |m2 z| + |m3|), so |dc| <= 6 u S.  Then
    ndc = cx * (1 / cw): the reciprocal, and the product, round once each, and cw carries 6 u Sw:
    |d ndc| <= 6 u Sx / |cw| + |ndc| (6 u Sw / |cw| + 2 u).  f = (ndc / 2 + 1 / 2) * W: halving is exact, the sum and the
    product round once each on a value <= (|ndc| + 1) / 2: |df| <= W (|d ndc| / 2 + 2 u (|ndc| + 1) / 2).  First order in u;
    the caller allows 2^-10 on top for the higher orders.  The window depth is the same expression with W = 1."""
    m = np.asarray(m, F32).reshape(4, 4).astype(np.float64)
    p = np.asarray(p, F32).astype(np.float64)
    u = 2.0 ** -24
    terms = np.concatenate([m[None, :, :3] * p[:, None, :], np.broadcast_to(m[None, :, 3:4], (p.shape[0], 4, 1))], axis=2)
    c, S = terms.sum(axis=2), np.abs(terms).sum(axis=2)
    w = c[:, 3]
    out = {}
    for name, k, scale in (("fx", 0, float(W)), ("fy", 1, float(H)), ("d", 2, 1.0)):
        ndc = c[:, k] / w
        dndc = 6 * u * S[:, k] / np.abs(w) + np.abs(ndc) * (6 * u * S[:, 3] / np.abs(w) + 2 * u)
        out[name] = (ndc * 0.5 + 0.5) * scale
        out[name + "_bound"] = scale * (dndc / 2 + u * (np.abs(ndc) + 1)) * (1 + 2.0 ** -10)
    out["w"] = w
    return out


# ------------------------------------------------------------------------------------------------ exact raster
def _exact_dyadic(vals):
    """float32 values -> (Python integers n_k, shift s) with value_k = n_k / 2^s exactly."""
    fr = [Fraction(float(v)) for v in vals]
    s = max(f.denominator for f in fr).bit_length() - 1
    return [int(f * (1 << s)) for f in fr], s


def raster_exact(vs, tris, W, H, first_id=1, cull_back=None, shadow=False, keys=None, margin=None):
    """Rasterise `tris` (int [T, 3] into the vertex stage `vs`) exactly.

    Camera form (shadow = False): returns (keys uint64 [H, W] = depth24 << 32 | id, margin float64 [H, W]); triangle t has
    id first_id + t; cull_back[t] drops triangle t when it faces away.  Shadow form: keys is uint32 [H, W] = smallest
    depth24 after the polygon offset.  Pass keys / margin of an earlier call to go on drawing into them."""
    if keys is None:
        keys = np.full((H, W), CLEARED_TEXEL if shadow else CLEARED_KEY, np.uint32 if shadow else np.uint64)
        margin = np.full((H, W), np.inf)
    X, Y, ok = vs["X"], vs["Y"], vs["ok"]
    M = DEPTH_MAX
    for t, (a, b, c) in enumerate(np.asarray(tris).reshape(-1, 3)):
        if not (ok[a] and ok[b] and ok[c]):
            continue
        x = [int(X[a]), int(X[b]), int(X[c])]
        y = [int(Y[a]), int(Y[b]), int(Y[c])]
        area2 = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
        if area2 == 0:
            continue
        s = 1 if area2 > 0 else -1
        if cull_back is not None and cull_back[t] and s < 0:
            continue
        # pixels whose centre 256 p + 128 lies within the bounding box, inside the image
        px0, px1 = max(0, -((128 - min(x)) // 256)), min(W - 1, (max(x) - 128) // 256)
        py0, py1 = max(0, -((128 - min(y)) // 256)), min(H - 1, (max(y) - 128) // 256)
        if px0 > px1 or py0 > py1:
            continue
        cx = (np.arange(px0, px1 + 1, dtype=np.int64) * 256 + 128)[None, :]
        cy = (np.arange(py0, py1 + 1, dtype=np.int64) * 256 + 128)[:, None]
        inside = np.ones((py1 - py0 + 1, px1 - px0 + 1), bool)
        E = []
        for k in range(3):  # the edge opposite vertex k, in the triangle's own winding; s turns it counter-clockwise
            i, j = (k + 1) % 3, (k + 2) % 3
            dx, dy = x[j] - x[i], y[j] - y[i]
            e = s * (dx * (cy - y[i]) - dy * (cx - x[i]))  # > 0 on the inner side
            # on the edge: the sign of e at (cx + eps, cy - eps^2) = sign of (-s dy, then -s dx)
            owns = (-s * dy > 0) or (dy == 0 and -s * dx > 0)
            inside &= (e > 0) | ((e == 0) & owns)
            E.append(e)
        if not inside.any():
            continue
        n, sh = _exact_dyadic([vs["d"][a], vs["d"][b], vs["d"][c]])
        den = abs(area2) << sh  # depth = num / den
        e0, e1, e2 = (E[k][inside].astype(object) for k in range(3))
        num = e0 * n[0] + e1 * n[1] + e2 * n[2]
        off = Fraction(0)
        if shadow:
            # gradient of the plane through (x_k / 256, y_k / 256, d_k), per pixel
            d = [Fraction(v, 1 << sh) for v in n]
            gx = Fraction(256) * ((d[1] - d[0]) * (y[2] - y[0]) - (d[2] - d[0]) * (y[1] - y[0])) / area2
            gy = Fraction(256) * ((d[2] - d[0]) * (x[1] - x[0]) - (d[1] - d[0]) * (x[2] - x[0])) / area2
            off = 8 * max(abs(gx), abs(gy)) + Fraction(8, 1 << 24)
            num, den = num * off.denominator + off.numerator * den, den * off.denominator
        num = np.asarray(num, object)
        # how far from a discard threshold (in depth24 steps), then discard
        lo_gap = np.array([abs(v) for v in num], object)
        hi_gap = np.array([abs(den - v) for v in num], object)
        if shadow:
            keep = np.array([v >= 0 for v in num], bool)
            num = np.array([min(v, den) for v in num], object)  # clamped at 1
        else:
            keep = np.array([0 <= v <= den for v in num], bool)
        two = 2 * den
        full = np.array([2 * v * M + den for v in num], object)
        q = np.array([v // two for v in full], object)
        rem = np.array([v % two for v in full], object)
        mg = np.array([float(Fraction(min(r, two - r), two)) for r in rem])
        thr = np.array([float(Fraction(min(l_, h_) * M, den)) for l_, h_ in zip(lo_gap, hi_gap)])
        if shadow:
            clamped = np.array([v == den for v in num], bool)
            mg = np.where(clamped, np.inf, mg)  # at the clamp every nearby value quantises to 2^24 - 1
            thr = np.array([float(Fraction(l_ * M, den)) for l_ in lo_gap])
        mg = np.minimum(mg, thr)
        ys, xs = np.nonzero(inside)
        ys, xs = ys + py0, xs + px0
        margin[ys, xs] = np.minimum(margin[ys, xs], mg)
        ys, xs, q = ys[keep], xs[keep], q[keep]
        if shadow:
            val = q.astype(np.uint32)
        else:
            val = (q.astype(np.uint64) << np.uint64(32)) | np.uint64(first_id + t)
        keys[ys, xs] = np.minimum(keys[ys, xs], val)
    return keys, margin


# ------------------------------------------------------------------------------------------------ frame set-up
class Frame:
    """Matrices of one frame: view / proj / light (row-major 4x4 float32), light_dir, cam_pos, W, H.  vp = proj view in
    float32.  tan(fov / 2) is the float32 nearest to the tangent of the float32 half angle (the set-up's tanf)."""

    def __init__(self, view, proj, light, light_dir, cam_pos, W, H):
        self.view, self.proj = np.asarray(view, F32).reshape(4, 4), np.asarray(proj, F32).reshape(4, 4)
        self.light = np.asarray(light, F32).reshape(4, 4)
        self.light_dir, self.cam_pos = np.asarray(light_dir, F32), np.asarray(cam_pos, F32)
        self.W, self.H = int(W), int(H)
        self.vp = mat_mul32(self.proj, self.view)
        k_pi = F32(3.141592653589)
        fov = k_pi * F32(39.5978) / F32(180.0)
        half = (fov * (F32(180.0) / k_pi) * F32(0.5)) * (k_pi / F32(180.0))
        self.tan_half_fov = F32(np.tan(np.float64(half)))
        self.aspect = F32(self.W) / F32(self.H)


def ground_keys(fr):
    """The ground plane y = 0 per pixel: (keys uint64 [H, W] = depth24 << 32 | 0 or all ones, hit float32 [H, W, 3]).
    float32 in the kernel's order (see the module docstring); only the plane's front face, only in front of the camera."""
    W, H = fr.W, fr.H
    one, two, half = F32(1.0), F32(2.0), F32(0.5)
    px, py = np.meshgrid(np.arange(W, dtype=F32), np.arange(H, dtype=F32))
    with np.errstate(all="ignore"):
        xn = ((px + half) / F32(W)) * two - one
        yn = ((py + half) / F32(H)) * two - one
        ex, ey, ez = xn * fr.tan_half_fov * fr.aspect, yn * fr.tan_half_fov, F32(-1.0)
        R = fr.view[:3, :3].T.astype(F32)  # eye -> world
        dirs = [(R[r, 0] * ex + R[r, 1] * ey) + R[r, 2] * ez for r in range(3)]
        pl = np.array([0.0, 1.0, 0.0, 0.0], F32)
        denom = (pl[0] * dirs[0] + pl[1] * dirs[1]) + pl[2] * dirs[2]
        num = -(((pl[0] * fr.cam_pos[0] + pl[1] * fr.cam_pos[1]) + pl[2] * fr.cam_pos[2]) + pl[3])
        tpar = num / denom
        hit = np.stack([fr.cam_pos[k] + dirs[k] * tpar for k in range(3)], axis=-1).astype(F32)
        c = xform32(fr.vp, hit.reshape(-1, 3)).reshape(H, W, 4)
        d = (c[..., 2] / c[..., 3]).astype(np.float64) * 0.5 + 0.5  # exact in double: 24 bits halved plus 1/2
        good = (denom < 0) & (tpar > 0) & (c[..., 3] > 0) & (d >= 0.0) & (d <= 1.0)
        q = np.floor(np.where(good, d, 0.0) * float(DEPTH_MAX) + 0.5)  # 49-bit product: exact in double too
    keys = np.where(good, q.astype(np.uint64) << np.uint64(32), CLEARED_KEY)
    return keys, hit


def linear_depth(depth24, cleared):
    """The float32 depth plane from depth24 (pyflex.cpp:1053): window depth = depth24 / (2^24 - 1) rounded to float32 (1 where
    cleared), then 2 f n / (f + n - (2 d - 1) (f - n))."""
    dw = np.where(cleared, 1.0, depth24.astype(np.float64) / float(DEPTH_MAX)).astype(F32)
    return F32(2.0) * ZFAR * ZNEAR / (ZFAR + ZNEAR - (F32(2.0) * dw - F32(1.0)) * (ZFAR - ZNEAR))


# ------------------------------------------------------------------------------------------------ normals (float64)
def vertex_normals64(pos, tris):
    """Area-weighted sum of the incident triangles' normals, normalised; (0, 1, 0) where the sum vanishes.  Returns
    (normals [n, 3], bound [n]): bound is what a float32 evaluation may deviate by per component.

    Worst case: a cross-product component ay bz - az by has two differences (u = 2^-24 each), two products and one
    subtraction behind it, 4 u |a| |b| at most; up to six running additions add 6 u sum_t |a_t| |b_t|; over three components
    that is 16 u sum_t |a_t| |b_t| / |sum_t a_t x b_t| after normalising, plus 2^-22 for the squared length, the root, the
    reciprocal and the final product.  That needs ten roundings of one sign on each component; the largest deviation measured
    (these tests' inputs, oracle and HIP kernel alike: they agree bit for bit) is 0.073 of it, so the tests use a quarter of
    the worst case, 4 u sum |a| |b| / |sum a x b| + 2^-22, of which the measured maximum is 0.20."""
    p = np.asarray(pos, F32).reshape(-1, 4)[:, :3].astype(np.float64)
    tris = np.asarray(tris).reshape(-1, 3)
    a, b = p[tris[:, 1]] - p[tris[:, 0]], p[tris[:, 2]] - p[tris[:, 0]]
    cr = np.cross(a, b)
    mag = np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1)
    s, sm = np.zeros_like(p), np.zeros(p.shape[0])
    for k in range(3):
        np.add.at(s, tris[:, k], cr)
        np.add.at(sm, tris[:, k], mag)
    ln = np.linalg.norm(s, axis=1)
    nz = ln > 0
    nrm = np.where(nz[:, None], s / np.where(nz, ln, 1.0)[:, None], np.array([0.0, 1.0, 0.0]))
    bound = np.where(nz, 4 * 2.0 ** -24 * sm / np.where(nz, ln, 1.0) + 2.0 ** -22, np.inf)
    return nrm, bound


# ------------------------------------------------------------------------------------------------ shading (float64)
def _pcf(shadow, u, v, ref):
    """12-tap PCF, each tap a bilinear mix of four depth compares (ref <= texel) with clamp-to-edge; cleared texels are 1.
    Also returns how close (in shadow depth24 steps) the nearest of the 48 compares came to its threshold."""
    tex = np.where(shadow == CLEARED_TEXEL, 1.0, shadow.astype(np.float64) / float(DEPTH_MAX))
    acc, gap = np.zeros_like(u), np.full_like(u, np.inf)
    for tx, ty in PCF_TAPS:
        x, y = (u + tx * 0.002) * SHADOW_RES - 0.5, (v + ty * 0.002) * SHADOW_RES - 0.5
        x0, y0 = np.floor(x), np.floor(y)
        ax, ay = x - x0, y - y0
        for dy in (0, 1):
            for dx in (0, 1):
                ix = np.clip(x0.astype(np.int64) + dx, 0, SHADOW_RES - 1)
                iy = np.clip(y0.astype(np.int64) + dy, 0, SHADOW_RES - 1)
                lit = (ref <= tex[iy, ix]).astype(np.float64)
                acc += lit * (ax if dx else 1.0 - ax) * (ay if dy else 1.0 - ay)
                gap = np.minimum(gap, np.abs(ref - tex[iy, ix]) * DEPTH_MAX)
    return acc / 12.0, gap


def shade(fr, shadow, p, n, color, bias):
    """The solid shader (shadersGL.cpp:795-839) at world points p with normals n (not renormalised), all float64:
    max(PCF shadow, 0.5); spot attenuation max(smoothstep(1, 0.5, |light ndc xy|^2), 0.05); Lambert x shadow x attenuation +
    wrap ambient; fog towards black by exp(eye z * density); gamma 1 / 2.2."""
    L, V = fr.light.astype(np.float64), fr.view.astype(np.float64)
    q = p + n * bias[:, None]
    lc = q @ L[:, :3].T + L[:, 3]
    lx, ly, lz = lc[:, 0] / lc[:, 3], lc[:, 1] / lc[:, 3], lc[:, 2] / lc[:, 3]
    u, v, wz = lx * 0.5 + 0.5, ly * 0.5 + 0.5, lz * 0.5 + 0.5
    inside = ~((u < 0) | (u > 1) | (v < 0) | (v > 1))
    sh, gap = np.ones_like(u), np.full_like(u, np.inf)
    if inside.any():
        sh[inside], gap[inside] = _pcf(shadow, u[inside], v[inside], wz[inside])
    sh = np.maximum(sh, 0.5)
    tt = np.clip((lx * lx + ly * ly - 1.0) / (0.5 - 1.0), 0.0, 1.0)
    att = np.maximum(tt * tt * (3.0 - 2.0 * tt), 0.05)
    ndl = -(n @ fr.light_dir.astype(np.float64))
    diff = np.maximum(0.0, ndl * sh) * att
    mixv = ndl * 0.5 + 0.5
    light, dark = np.array([0.03, 0.025, 0.025]) * 1.5, np.array([0.025, 0.025, 0.03])
    amb = 4.0 * color * (dark * (1.0 - mixv[:, None]) + light * mixv[:, None]) * att[:, None]
    lit = color * diff[:, None] + amb
    ez = p @ V[2, :3] + V[2, 3]
    fogged = lit * np.exp(ez * float(FOG))[:, None]
    return np.power(np.maximum(fogged, 0.0), 1.0 / 2.2), gap


# ------------------------------------------------------------------------------------------------ one frame
def render(fr, pos, tris, sph_verts=None, sph_nrms=None, sph_tris=None, want_color=True):
    """Everything the rasteriser produces for one frame, from the rules above.

    pos float32 [n, 4], tris int [T, 3]; sph_*: the picker meshes (float32 [v, 4], int [t, 3]).  Returns a dict:
    zkeys (triangles only) / keys (ground joined in) uint64 [H, W], margin [H, W], shadow uint32 [2048, 2048],
    shadow_margin, depth float32 [H, W], rgba uint8 [H, W, 4] (rows bottom-up), normals float64 [n, 3], pcf_gap [H, W] (how
    close, in shadow depth24 steps, the nearest PCF compare of the pixel came to its threshold)."""
    W, H = fr.W, fr.H
    pos = np.asarray(pos, F32).reshape(-1, 4)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    n_s = 0 if sph_tris is None else len(sph_tris)
    sv = np.zeros((0, 4), F32) if n_s == 0 else np.asarray(sph_verts, F32).reshape(-1, 4)
    sn = np.zeros((0, 4), F32) if n_s == 0 else np.asarray(sph_nrms, F32).reshape(-1, 4)
    st = np.zeros((0, 3), np.int64) if n_s == 0 else np.asarray(sph_tris, np.int64).reshape(-1, 3)
    # one vertex array, one triangle list in draw order: spheres, then cloth
    verts = np.concatenate([sv[:, :3], pos[:, :3]])
    all_tris = np.concatenate([st, tris + sv.shape[0]])
    is_sphere = np.arange(len(all_tris)) < n_s
    out = {}
    vs_l = vertex_stage(fr.light, SHADOW_RES, SHADOW_RES, verts)
    out["shadow"], out["shadow_margin"] = raster_exact(vs_l, all_tris, SHADOW_RES, SHADOW_RES, shadow=True)
    vs = vertex_stage(fr.vp, W, H, verts)
    out["zkeys"], out["margin"] = raster_exact(vs, all_tris, W, H, first_id=1, cull_back=is_sphere)
    gk, _ = ground_keys(fr)
    keys = np.minimum(out["zkeys"], gk)
    out["keys"] = keys
    cleared = keys == CLEARED_KEY
    out["depth"] = linear_depth((keys >> np.uint64(32)).astype(np.int64), cleared)
    nrm64, _ = vertex_normals64(pos, tris)
    out["normals"] = nrm64
    if not want_color:
        return out
    rgb, pcf_gap = np.zeros((H, W, 3)), np.full((H, W), np.inf)
    ids = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    # ground: the camera ray through the pixel centre meets y = 0 (float64, from the matrices alone)
    g = (~cleared) & (ids == 0)
    if g.any():
        ys, xs = np.nonzero(g)
        V = fr.view.astype(np.float64)
        tan = 1.0 / float(fr.proj[1, 1])
        ex = ((xs + 0.5) / W * 2 - 1) * tan * (W / H)
        ey = ((ys + 0.5) / H * 2 - 1) * tan
        dirs = np.stack([ex, ey, -np.ones_like(ex)], 1) @ V[:3, :3]  # rows of V^T applied: eye -> world
        cam = fr.cam_pos.astype(np.float64)
        tpar = -cam[1] / dirs[:, 1]
        p = cam + dirs * tpar[:, None]
        nn = np.broadcast_to(np.array([0.0, 1.0, 0.0]), p.shape)
        rgb[ys, xs], pcf_gap[ys, xs] = shade(fr, out["shadow"], p, nn, COL_PLANE, np.zeros(len(p)))
    tpx = (~cleared) & (ids > 0)
    if tpx.any():
        ys, xs = np.nonzero(tpx)
        tid = ids[ys, xs] - 1
        tv = all_tris[tid]
        X, Y = vs["X"], vs["Y"]
        cx, cy = xs * 256 + 128, ys * 256 + 128
        lam = np.zeros((len(tid), 3))
        for k in range(3):
            i, j = tv[:, (k + 1) % 3], tv[:, (k + 2) % 3]
            lam[:, k] = ((X[j] - X[i]) * (cy - Y[i]) - (Y[j] - Y[i]) * (cx - X[i])).astype(np.float64)
        area2 = lam.sum(1)
        lam /= area2[:, None]  # affine weights in window space
        qw = lam / vs["w"][tv].astype(np.float64)  # perspective-correct: weights of 1 / w
        bw = qw / qw.sum(1, keepdims=True)
        vn = np.concatenate([sn[:, :3].astype(np.float64), nrm64])
        p = (bw[:, :, None] * verts[tv].astype(np.float64)).sum(1)
        nn = (bw[:, :, None] * vn[tv]).sum(1)
        nn = np.where((area2 < 0)[:, None], -nn, nn)  # seen from behind: flipped normal
        sph = tid < n_s
        col = np.where(sph[:, None], COL_SHAPE, COL_CLOTH)
        rgb[ys, xs], pcf_gap[ys, xs] = shade(fr, out["shadow"], p, nn, col, np.where(sph, BIAS_SHAPE, 0.0))
    rgba = np.zeros((H, W, 4), np.uint8)
    rgba[..., :3] = np.floor(np.clip(rgb, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    rgba[..., 3] = np.where(cleared, 0, 255)
    out["rgba"], out["pcf_gap"] = rgba, pcf_gap
    return out
