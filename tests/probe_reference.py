"""The rules of the probe (flingbot_amd/probe.py, include/flingsim.h fs_lattice_actions and fs_probe_panels) restated in numpy
and plain Python, independently of the code under test: the on-cloth rule, the lattice's codes through the CPU oracle
(oracle/action.py), rank statistics by counting, and the probe strip on top of tests/report_reference.py."""
import numpy as np

import report_reference as ref
from oracle import action as oracle_action


# ---- fs_lattice_actions ---------------------------------------------------------------------------------------------------
def on_cloth(depth, row, col, r):
    """BatchedFlingEnv._on_cloth: no pixel of the plane inside the disc of radius r around (row, col) is background (2.0)."""
    if r <= 0:
        return True
    S = depth.shape[0]
    for y in range(max(0, row - r), min(S - 1, row + r) + 1):
        for x in range(max(0, col - r), min(S - 1, col + r) + 1):
            if (y - row) ** 2 + (x - col) ** 2 <= r * r and depth[y, x] == np.float32(2.0):
                return False
    return True


def oracle_cfg(depth, scales, rotations, D, g, drag, place, reach, left=(0.765, 0, 0), right=(-0.765, 0, 0)):
    return dict(pix_grasp_dist=g, pix_drag_dist=drag, pix_place_dist=place, obs_dim=D, scales=list(scales),
                rotations=list(rotations), depth=depth, reach_distance_limit=reach, left_arm_base=np.array(left, np.float64),
                right_arm_base=np.array(right, np.float64), grasp_height=0.02, stretchdrag_dist=0.3)


def oracle_cell(action, t, y, z, cfg):
    """oracle.action.evaluate_candidate; a zero depth under a grasp pixel ('Invalid pick point') is an invalid cell."""
    try:
        return oracle_action.evaluate_candidate(action, t, y, z, cfg)
    except Exception as err:
        if "Invalid pick point" not in str(err):
            raise
        return None


def lattice_oracle(actions, cfgs, requests):
    """Every cell of the requests through the oracle, once: per request (valid bool [gy, gz], pretransform pixels int
    [gy, gz, 2, 2]), and how close any cell comes to a rounding boundary of the validity test, computed with the oracle's own
    functions: reach_margin = the smallest |distance - limit| over the distances between either arm base and either grasp
    point, pixel_margin = the smallest distance of a transformed coordinate to an integer, reach_cut = the cells that pass
    every pixel test and fail on reach."""
    reach_margin, pixel_margin, cut, cells = np.inf, np.inf, 0, []
    pose = oracle_action.compute_pose(pos=[0, 2, 0], lookat=[0, 0, 0], up=[0, 0, 1])
    for e, p, t, y0, z0, stride, gy, gz in requests:
        cfg = cfgs[e]
        depth, S = cfg["depth"], cfg["depth"].shape[0]
        n_scales = len(cfg["scales"])
        mat = oracle_action.get_transform_matrix(original_dim=S, resized_dim=cfg["obs_dim"], rotation=-cfg["rotations"][t // n_scales],
                                                 scale=cfg["scales"][t % n_scales])
        valid, pixels = np.zeros((gy, gz), bool), np.zeros((gy, gz, 2, 2), np.int64)
        for i in range(gy):
            for j in range(gz):
                y, z = y0 + i * stride, z0 + j * stride
                got = oracle_cell(actions[p], t, y, z, cfg)
                if got is not None:
                    valid[i, j], pixels[i, j] = True, got["pretransform_pixels"]
                pts = np.array(oracle_action.get_action_params(actions[p], (t, y, z), cfg["pix_grasp_dist"], cfg["pix_drag_dist"],
                                                               cfg["pix_place_dist"]))
                if (pts < 0).any() or (pts >= cfg["obs_dim"]).any():
                    continue
                moved = np.matmul(np.concatenate((pts, np.ones((2, 1), pts.dtype)), axis=1), mat)[:, :2]
                pixel_margin = min(pixel_margin, float(np.abs(moved - np.round(moved)).min()))
                pix = moved.astype(int)
                if (pix < 0).any() or (pix >= S).any() or any(depth[b, a] == 0 for a, b in pix):
                    continue
                world = [oracle_action.pixel_to_3d(depth.copy(), x=a, y=b, pose_matrix=pose) for a, b in pix]
                dist = [np.linalg.norm(base - w) for base in (cfg["left_arm_base"], cfg["right_arm_base"]) for w in world]
                reach_margin = min(reach_margin, float(np.abs(np.array(dist) - cfg["reach_distance_limit"]).min()))
                cut += got is None
        cells.append((valid, pixels))
    return dict(cells=cells, reach_margin=reach_margin, pixel_margin=pixel_margin, reach_cut=int(cut))


def lattice_codes(oracle, cfgs, requests, radius):
    """code uint8 per request [gy, gz]: bit 0 valid (the oracle), bits 1 / 2 the grasp points on cloth, 0 where invalid."""
    out = []
    for (valid, pixels), req in zip(oracle["cells"], requests):
        depth = cfgs[req[0]]["depth"]
        code = np.zeros(valid.shape, np.uint8)
        for i, j in np.argwhere(valid):
            (a0, a1), (b0, b1) = pixels[i, j]
            code[i, j] = 1 | (2 if on_cloth(depth, int(a1), int(a0), radius) else 0) | (4 if on_cloth(depth, int(b1), int(b0), radius) else 0)
        out.append(code)
    return out


# ---- statistics -----------------------------------------------------------------------------------------------------------
def ranks_by_counting(v):
    """Average ranks without sorting: 1 + (how many are smaller) + (how many others are equal) / 2."""
    v = [float(x) for x in v]
    return [1.0 + sum(w < x for w in v) + (sum(w == x for w in v) - 1) / 2.0 for x in v]


def spearman(predicted, measured):
    """Rank correlation over the cells finite on both sides; None below 2 cells or at zero variance on either side."""
    p, m = np.ravel(np.asarray(predicted, np.float64)), np.ravel(np.asarray(measured, np.float64))
    cells = [k for k in range(len(p)) if np.isfinite(p[k]) and np.isfinite(m[k])]
    if len(cells) < 2:
        return None
    a, b = ranks_by_counting(p[cells]), ranks_by_counting(m[cells])
    n = float(len(cells))
    ma, mb = sum(a) / n, sum(b) / n
    saa = sum((x - ma) ** 2 for x in a)
    sbb = sum((y - mb) ** 2 for y in b)
    if saa == 0 or sbb == 0:
        return None
    return sum((x - ma) * (y - mb) for x, y in zip(a, b)) / (saa ** 0.5 * sbb ** 0.5)


def pair_counts(predicted, measured):
    """lookahead.pair_agreement's rule with min_gap 0, over the cells finite on both sides: (pairs, concordant)."""
    p, m = np.ravel(np.asarray(predicted, np.float64)), np.ravel(np.asarray(measured, np.float64))
    cells = [k for k in range(len(p)) if np.isfinite(p[k]) and np.isfinite(m[k])]
    pairs = concordant = 0
    for a in cells:
        for b in cells:
            if m[a] > m[b]:
                pairs += 1
                concordant += int(p[a] > p[b])
    return pairs, concordant


# ---- fs_probe_panels ------------------------------------------------------------------------------------------------------
def measured_image(table, D, measured, valid, vrange, origin, stride, chosen_cell):
    """uint8 [D, D, 3]: every map pixel in the colour of the lattice cell it is nearest to -- jet for a finite measured value,
    (128, 128, 128) valid and not executed, (64, 64, 64) invalid, black outside the lattice, the chosen cell's outermost pixels
    white.  A whole image at a time: cell index vectors per axis, colours per cell, one gather."""
    measured = np.asarray(measured, np.float32)
    gy, gz = measured.shape
    cell = np.where(np.asarray(valid).astype(bool)[..., None], np.uint8(128), np.uint8(64)) * np.ones(3, np.uint8)
    finite = np.isfinite(measured)
    cell[finite] = ref.jet(table, measured, vrange[0], vrange[1])[finite]
    out = np.zeros((D, D, 3), np.uint8)
    axes = []
    for o, count in ((origin[0], gy), (origin[1], gz)):
        n = np.arange(D, dtype=np.int64) - int(o) + int(stride) // 2
        idx = np.where(n >= 0, n, 0) // int(stride)
        axes.append((idx, (n >= 0) & (idx < count), np.where(n >= 0, n, 0) % int(stride)))
    (iy, oky, ry), (iz, okz, rz) = axes
    inside = oky[:, None] & okz[None, :]
    out[inside] = cell[np.minimum(iy, gy - 1)[:, None], np.minimum(iz, gz - 1)[None, :]][inside]
    if chosen_cell is not None:
        edge = lambda r: (r == 0) | (r == int(stride) - 1)   # noqa: E731
        mine = (inside & (iy == chosen_cell[0])[:, None] & (iz == chosen_cell[1])[None, :]) & (edge(ry)[:, None] | edge(rz)[None, :])
        out[mine] = 255
    return out


def strip(table, stack, value_map, vrange, measured, valid, origin, stride, chosen_cell, after, small, panel, S):
    """uint8 [panel, 4 * panel, 3]: transformed RGB + action | predicted map | measured map | after"""
    D = np.asarray(value_map).shape[0]
    last = np.zeros((S, S, 3), np.uint8) if after is None else ref.image_of(after)
    parts = [ref.draw(ref.image_of(stack), small), ref.jet(table, value_map, vrange[0], vrange[1]),
             measured_image(table, D, measured, valid, vrange, origin, stride, chosen_cell), last]
    return np.concatenate([ref.sample(p, panel) for p in parts], axis=1)
