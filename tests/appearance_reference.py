"""The appearance rules (include/flingsim.h fs_appearance, csrc/fs_raster_kernels.h "ground texture") restated in numpy
float64 -- the reference tests/test_appearance_gpu.py compares the shading kernels with.  Not a test module.

Written from the rule in the header, not from the kernel: whole arrays at a time, Python integers masked to 32 bits for
the hash, np.floor on float64 coordinates.  render() takes keys, depth, shadow map and normals from
raster_reference.render(..., want_color=False) (through raster_scenes.reference) and shades every pixel with
raster_reference.shade, the colour given per pixel."""
import numpy as np

import raster_reference as rr
import raster_scenes as rs

M32 = 0xFFFFFFFF


def hash32(i, j, o, seed):
    """h = i 0x9E3779B1 + j 0x85EBCA77 + o 0xC2B2AE3D + seed; h ^= h >> 16; h *= 0x7FEB352D; h ^= h >> 15; h *= 0x846CA68B;
    h ^= h >> 16 -- wrapping 32-bit unsigned; i, j integer arrays (two's complement for negatives)."""
    shape = np.broadcast(i, j).shape
    # (& on a negative int64: its two's complement; uint64 arrays wrap modulo 2^64, which the mask reduces to modulo 2^32)
    i, j = ((np.atleast_1d(np.asarray(v, np.int64)) & M32).astype(np.uint64) for v in (i, j))
    m32 = np.uint64(M32)
    h = (i * np.uint64(0x9E3779B1) + j * np.uint64(0x85EBCA77) + np.uint64((int(o) * 0xC2B2AE3D + int(seed)) & M32)) & m32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x7FEB352D)) & m32
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x846CA68B)) & m32
    h ^= h >> np.uint64(16)
    return h.astype(np.int64).reshape(shape)


def lattice(i, j, o, seed):
    return (hash32(i, j, o, seed) >> 8).astype(np.float64) * 2.0 ** -24


def noise(hx, hz, seed, cells_per_m, octaves):
    """t of the rule at the ground points (hx, hz), float64 arrays."""
    hx, hz = np.asarray(hx, np.float64), np.asarray(hz, np.float64)
    total = np.zeros(np.broadcast(hx, hz).shape)
    smooth = lambda x: x * x * (3.0 - 2.0 * x)   # noqa: E731
    for o in range(int(octaves)):
        f = float(cells_per_m) * 2.0 ** o
        u, v = np.clip(hx * f, -2.0 ** 30, 2.0 ** 30), np.clip(hz * f, -2.0 ** 30, 2.0 ** 30)
        i, j = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
        sa, sb = smooth(u - i), smooth(v - j)
        low = lattice(i, j, o, seed) * (1.0 - sa) + lattice(i + 1, j, o, seed) * sa
        high = lattice(i, j + 1, o, seed) * (1.0 - sa) + lattice(i + 1, j + 1, o, seed) * sa
        total = total + (low * (1.0 - sb) + high * sb) * 2.0 ** -(o + 1)
    return total / (1.0 - 2.0 ** -int(octaves)) if octaves > 0 else total


def ground_albedo(ap, hx, hz):
    """[n, 3] linear albedo of the ground at (hx, hz) under appearance dictionary `ap`."""
    g = np.asarray(ap["ground_rgb"], np.float32).astype(np.float64).reshape(2, 3)
    t = noise(hx, hz, ap["ground_seed"], np.float32(ap["ground_cells_per_m"]), ap["ground_octaves"])
    return g[0] + (g[1] - g[0]) * np.asarray(t)[..., None]


def render(sc, ap):
    """Scene `sc` of raster_scenes under appearance `ap`: dict(rgba uint8 [H, W, 4] rows bottom-up, depth, keys, ground
    (bool [H, W]: the pixel shows the ground), sphere (bool [H, W]), pcf_gap)."""
    ref = rs.reference(sc, False)
    fr, W, H = ref["frame"], sc.W, sc.H
    keys, shadow = ref["keys"], ref["shadow"]
    sv, sn, st = ref["mesh"]
    n_s = 0 if st is None else len(st)
    sv = np.zeros((0, 4), np.float32) if n_s == 0 else np.asarray(sv, np.float32).reshape(-1, 4)
    sn = np.zeros((0, 4), np.float32) if n_s == 0 else np.asarray(sn, np.float32).reshape(-1, 4)
    st = np.zeros((0, 3), np.int64) if n_s == 0 else np.asarray(st, np.int64).reshape(-1, 3)
    verts = np.concatenate([sv[:, :3], sc.pos[:, :3]])
    all_tris = np.concatenate([st, np.asarray(ref["faces"], np.int64) + sv.shape[0]])
    cleared = keys == rr.CLEARED_KEY
    ids = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    rgb, gap = np.zeros((H, W, 3)), np.full((H, W), np.inf)
    ground = (~cleared) & (ids == 0)
    if ground.any():   # the camera ray through the pixel centre meets y = 0 (float64, from the matrices alone)
        ys, xs = np.nonzero(ground)
        V = fr.view.astype(np.float64)
        tan = 1.0 / float(fr.proj[1, 1])
        ex, ey = ((xs + 0.5) / W * 2 - 1) * tan * (W / H), ((ys + 0.5) / H * 2 - 1) * tan
        dirs = np.stack([ex, ey, -np.ones_like(ex)], 1) @ V[:3, :3]
        cam = fr.cam_pos.astype(np.float64)
        p = cam + dirs * (-cam[1] / dirs[:, 1])[:, None]
        up = np.broadcast_to(np.array([0.0, 1.0, 0.0]), p.shape)
        rgb[ys, xs], gap[ys, xs] = rr.shade(fr, shadow, p, up, ground_albedo(ap, p[:, 0], p[:, 2]), np.zeros(len(p)))
    tri = (~cleared) & (ids > 0)
    sphere = np.zeros((H, W), bool)
    if tri.any():
        ys, xs = np.nonzero(tri)
        tid = ids[ys, xs] - 1
        tv = all_tris[tid]
        vs = rr.vertex_stage(fr.vp, W, H, verts)
        X, Y = vs["X"], vs["Y"]
        cx, cy = xs * 256 + 128, ys * 256 + 128
        lam = np.zeros((len(tid), 3))
        for k in range(3):
            i, j = tv[:, (k + 1) % 3], tv[:, (k + 2) % 3]
            lam[:, k] = ((X[j] - X[i]) * (cy - Y[i]) - (Y[j] - Y[i]) * (cx - X[i])).astype(np.float64)
        area2 = lam.sum(1)
        lam /= area2[:, None]
        qw = lam / vs["w"][tv].astype(np.float64)
        bw = qw / qw.sum(1, keepdims=True)
        vn = np.concatenate([sn[:, :3].astype(np.float64), ref["normals"]])
        p = (bw[:, :, None] * verts[tv].astype(np.float64)).sum(1)
        nn = (bw[:, :, None] * vn[tv]).sum(1)
        nn = np.where((area2 < 0)[:, None], -nn, nn)
        sph = tid < n_s
        sphere[ys, xs] = sph
        cloth = np.asarray(ap["cloth_rgb"], np.float32).astype(np.float64)
        col = np.where(sph[:, None], rr.COL_SHAPE, cloth)
        rgb[ys, xs], gap[ys, xs] = rr.shade(fr, shadow, p, nn, col, np.where(sph, rr.BIAS_SHAPE, 0.0))
    rgba = np.zeros((H, W, 4), np.uint8)
    rgba[..., :3] = np.floor(np.clip(rgb, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    rgba[..., 3] = np.where(cleared, 0, 255)
    return dict(rgba=rgba, depth=ref["depth"], keys=keys, ground=ground, sphere=sphere, pcf_gap=gap)
