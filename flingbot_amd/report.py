"""Action reports: what the policy picked, drawn on what it saw (the reference's visualize.py and visualize_action).

    env = BatchedFlingEnv(sim, action_report=True, report_root="report")        # or evaluate's --report DIR
    stats = evaluate.run_tasks(policy, env, tasks)
    write_report("report")                                                      # report/index.html

The reference builds a matplotlib figure on the host for every chosen action (environment/utils.py visualize_action,
:369-432, called from simEnv.py:653-654) and visualize.py turns the replay buffer into index.html.  Here the inputs stay
on the device: `value_range` (fs_value_range) takes the colour range over the chosen primitive's value maps and `compose`
(fs_action_panels) draws, for all actions of a list in one launch, the strip
    before | value map (jet) | transformed RGB + action | before + action | after
as uint8 [panel, 5 panel, 3].  include/flingsim.h states every rule; tests/report_reference.py restates them in numpy and
the kernels are compared with it byte for byte.  The colour bar and the titles of the reference's figure are not drawn.
`compose_lanes` (fs_lane_panels) draws a look-ahead step (flingbot_amd/lookahead.py) the same way:
    before + the action of every executed lane in its rank colour | after lane 0 | ... | after lane K-1
as uint8 [panel, (1 + K) panel, 3], each after panel framed in its rank colour, the followed one with a white inner frame
(tests/lane_report_reference.py restates its rules on top of report_reference).
`compose_probe` (fs_probe_panels) draws a probed map (flingbot_amd/probe.py):
    what the net saw + the chosen action | predicted map (jet) | measured map on its lattice, the same range | after the best cell
as uint8 [panel, 4 panel, 3] (tests/probe_reference.py restates its rules).

`action_overlays` restates draw_action and its helpers (environment/utils.py:283-366) as a list of integer primitives --
rings and segments, pixels as (row, column) -- which is all the kernel ever sees.  The coverage rules of a ring and of a
segment are this project's own: cv2 is absent here, so its line / circle rasterisation and the shape of cv2.arrowedLine's
tip (taken as two segments of 0.1 |shaft| at +-45 degrees to the shaft) are NOT pinned to OpenCV (PARITY.md section 3).
PNG and HTML are written with zlib / struct and plain strings: neither PIL nor matplotlib is needed.
"""
import json
import os

import numpy as np

RING, SEGMENT = 0, 1             # include/flingsim.h FS_PANEL_RING / FS_PANEL_SEGMENT
MAX_PRIMS = 8
ACTIONS_FILE = "actions.jsonl"
# include/flingsim.h fs_panel_record / fs_range_item
PANEL_RECORD = np.dtype([("stack", np.uint64), ("value_map", np.uint64), ("range", np.uint64), ("before", np.uint64),
                         ("after", np.uint64), ("n_small", np.int32), ("n_large", np.int32),
                         ("small", np.int32, (MAX_PRIMS, 9)), ("large", np.int32, (MAX_PRIMS, 9))])
RANGE_ITEM = np.dtype([("values", np.uint64), ("count", np.int64)])
assert PANEL_RECORD.itemsize == 624 and RANGE_ITEM.itemsize == 16
LANE_MAX = 8                     # include/flingsim.h FS_LANE_MAX / fs_lane_record
LANE_RECORD = np.dtype([("before", np.uint64), ("after", np.uint64, (LANE_MAX,)), ("n_lanes", np.int32), ("followed", np.int32),
                        ("n_prims", np.int32, (LANE_MAX,)), ("prims", np.int32, (LANE_MAX, MAX_PRIMS, 9))])
assert LANE_RECORD.itemsize == 2416
# include/flingsim.h fs_probe_record
PROBE_RECORD = np.dtype([("stack", np.uint64), ("value_map", np.uint64), ("range", np.uint64), ("measured", np.uint64),
                         ("code", np.uint64), ("after", np.uint64), ("y0", np.int32), ("z0", np.int32), ("stride", np.int32),
                         ("gy", np.int32), ("gz", np.int32), ("cy", np.int32), ("cz", np.int32), ("n_small", np.int32),
                         ("small", np.int32, (MAX_PRIMS, 9))])
assert PROBE_RECORD.itemsize == 368

GREEN, YELLOW, RED, MAGENTA, CYAN = (0, 255, 0), (255, 255, 0), (255, 0, 0), (255, 0, 255), (0, 255, 255)
JET_BREAKPOINTS = (((0, 0), (0.35, 0), (0.66, 1), (0.89, 1), (1, 0.5)),                    # red
                   ((0, 0), (0.125, 0), (0.375, 1), (0.64, 1), (0.91, 0), (1, 0)),         # green
                   ((0, 0.5), (0.11, 1), (0.34, 1), (0.65, 0), (1, 0)))                    # blue


# ---- the overlay of an action as integer primitives ---------------------------------------------------------------------------
def _ring(centre, thickness, colour):
    """cv2.circle(center, radius=2 * thickness, thickness=thickness)"""
    return (RING, int(centre[0]), int(centre[1]), 2 * int(thickness), 0, int(thickness)) + tuple(colour)


def _segment(a, b, thickness, colour):
    return (SEGMENT, int(a[0]), int(a[1]), int(b[0]), int(b[1]), int(thickness)) + tuple(colour)


def _arrow(start, end, thickness, colour):
    """cv2.arrowedLine with its default tipLength = 0.1 as three segments: the shaft, and from the end point two tips of
    length 0.1 |shaft| at +-45 degrees to the direction back along the shaft; the tips' end points in float64, rounded half
    to even.  A zero-length arrow is three degenerate segments (one dot)."""
    sy, sx, ey, ex = int(start[0]), int(start[1]), int(end[0]), int(end[1])
    back = np.arctan2(float(sy - ey), float(sx - ex))      # the angle of end -> start, rows as y
    tip = 0.1 * np.hypot(float(sy - ey), float(sx - ex))
    out = [_segment((sy, sx), (ey, ex), thickness, colour)]
    for turn in (np.pi / 4, -np.pi / 4):
        ty = int(np.rint(ey + tip * np.sin(back + turn)))
        tx = int(np.rint(ex + tip * np.cos(back + turn)))
        out.append(_segment((ey, ex), (ty, tx), thickness, colour))
    return out


def action_overlays(action_primitive, pixels, thickness=1):
    """draw_action (environment/utils.py:350-366) as a primitive list [(kind, y0, x0, y1, x1, t, r, g, b), ...] in drawing
    order.  pixels: the action's two points as (row, column) -- the reference hands cv2 center=(int(p[1]), int(p[0])).
      fling        ring (green) at the first point, segment (yellow), ring (red) at the second        (:283-301)
      stretchdrag  ring (magenta), segment (yellow), ring (cyan), and a red arrow from the integer midpoint along
                   cross((left - right, 0), (0, 0, 1))[:2]                                            (:304-332)
      drag         one magenta arrow from the first point to the second                               (:335-347, 357-360)
      place        one cyan arrow                                                                     (:361-364)"""
    pts = np.asarray(pixels)
    if pts.shape != (2, 2):
        raise ValueError(f"action_overlays: two (row, column) pixels, got shape {pts.shape}")
    left, right = pts[0], pts[1]
    t = int(thickness)
    if action_primitive == "fling":
        return [_ring(left, t, GREEN), _segment(left, right, t, YELLOW), _ring(right, t, RED)]
    if action_primitive == "stretchdrag":
        d = left - right
        direction = np.array([d[1], -d[0]])                       # cross((d0, d1, 0), (0, 0, 1))[:2]
        start = ((left + right) / 2).astype(int)
        end = start + direction
        return [_ring(left, t, MAGENTA), _segment(left, right, t, YELLOW), _ring(right, t, CYAN)] + \
            _arrow((int(start[0]), int(start[1])), (int(end[0]), int(end[1])), t, RED)
    if action_primitive == "drag":
        return _arrow(left, right, t, MAGENTA)
    if action_primitive == "place":
        return _arrow(left, right, t, CYAN)
    raise NotImplementedError(f"action_overlays: unknown primitive {action_primitive!r}")


def transformed_pixels(action_primitive, max_indices, selector):
    """The action's two points in the network image, (row, column): simEnv.get_action_params (simEnv.py:517-537)."""
    from .action import get_action_params
    return np.array(get_action_params(action_primitive, max_indices, selector.pix_grasp_dist, selector.pix_drag_dist,
                                      selector.pix_place_dist))


# ---- the colour table ---------------------------------------------------------------------------------------------------------
def jet_closed_form():
    """matplotlib's jet from its breakpoints: piecewise linear per channel, sampled at linspace(0, 1, 256), trunc(c * 255);
    uint8 [256, 3]."""
    x = np.linspace(0.0, 1.0, 256)
    return np.stack([np.trunc(np.interp(x, [p[0] for p in ch], [p[1] for p in ch]) * 255.0).astype(np.uint8)
                     for ch in JET_BREAKPOINTS], axis=1)


def jet_table():
    """The table compiled into libflingsim (csrc/fs_jet_table.h), uint8 [256, 3]."""
    import ctypes as C

    from .sim import load_library
    lib = load_library()
    out = np.zeros((256, 3), np.uint8)
    if lib.fs_jet_table(out.ctypes.data_as(C.POINTER(C.c_ubyte)), out.size) != 0:
        raise RuntimeError("fs_jet_table: " + lib.fs_last_error().decode())
    return out


# ---- the device side ----------------------------------------------------------------------------------------------------------
def _plane(t, name):
    import torch
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError(f"report: {name} must be a contiguous float32 CUDA tensor")
    return t


def value_range(maps):
    """(vmin, vmax) over the finite values of every tensor in `maps` (contiguous float32 CUDA tensors of any shape, on one
    device): a float32 CUDA tensor [len(maps), 2], (0, 0) for a tensor without a finite value.  One launch per 128 tensors
    and no host synchronisation: the result stays on the device."""
    import torch

    from .sim import stream_call
    maps = [_plane(m, "a value map") for m in maps]
    dev = maps[0].device if maps else torch.device("cuda")
    out = torch.empty((len(maps), 2), dtype=torch.float32, device=dev)
    if not maps:
        return out
    items = np.zeros(len(maps), RANGE_ITEM)
    for k, m in enumerate(maps):
        if m.device != dev:
            raise ValueError("value_range: the maps live on different devices")
        if m.numel() < 1:
            raise ValueError("value_range: an empty tensor has no range")
        items[k] = (m.data_ptr(), m.numel())
    stream_call("fs_value_range", dev, items.ctypes.data, len(maps), out)
    return out


def compose(items, panel=200):
    """The strips of a list of actions: ONE table upload, ONE launch, ONE download.  An item is a dictionary of
      stack [4, D, D], value_map [D, D], range [2], before [>= 3, S, S], after [>= 3, S, S] or None  (float32 CUDA tensors)
      small, large: primitive lists (action_overlays) for the D x D and the S x S panel, at most 8 each.
    Returns uint8 [len(items), panel, 5 * panel, 3] (numpy)."""
    import torch

    from .sim import stream_call, work_buffer
    panel = int(panel)
    if not items:
        return np.zeros((0, panel, 5 * panel, 3), np.uint8)
    first = items[0]
    D, S = int(first["stack"].shape[-1]), int(first["before"].shape[-1])
    dev = first["stack"].device
    table = np.zeros(len(items), PANEL_RECORD)
    for k, it in enumerate(items):
        stack, vmap, rng, before = (_plane(it[n], n) for n in ("stack", "value_map", "range", "before"))
        after = None if it.get("after") is None else _plane(it["after"], "after")
        if tuple(stack.shape) != (4, D, D) or tuple(vmap.shape) != (D, D) or rng.numel() != 2:
            raise ValueError(f"compose: item {k}: stack {tuple(stack.shape)}, value map {tuple(vmap.shape)}, range {tuple(rng.shape)}")
        for name, t in (("before", before), ("after", after)):
            if t is not None and (t.dim() != 3 or t.shape[0] < 3 or tuple(t.shape[1:]) != (S, S)):
                raise ValueError(f"compose: item {k}: {name} has shape {tuple(t.shape)}, expected [>= 3, {S}, {S}]")
        if any(t is not None and t.device != dev for t in (stack, vmap, rng, before, after)):
            raise ValueError(f"compose: item {k} lives on another device")
        row = table[k]
        row["stack"], row["value_map"], row["range"], row["before"] = (t.data_ptr() for t in (stack, vmap, rng, before))
        row["after"] = 0 if after is None else after.data_ptr()
        for name in ("small", "large"):
            prims = np.asarray(it.get(name, ()), np.int64).reshape(-1, 9)
            if len(prims) > MAX_PRIMS:
                raise ValueError(f"compose: item {k}: {len(prims)} primitives on a panel (at most {MAX_PRIMS})")
            if prims.size and np.abs(prims).max() > 2 ** 31 - 1:
                raise ValueError(f"compose: item {k}: a primitive does not fit an int")
            row["n_" + name] = len(prims)
            row[name][:len(prims)] = prims
    out = torch.empty((len(items), panel, 5 * panel, 3), dtype=torch.uint8, device=dev)
    work = work_buffer("fs_action_panels_work_bytes", dev, len(items))
    stream_call("fs_action_panels", dev, table.ctypes.data, len(items), D, S, panel, out, work)
    return out.cpu().numpy()


def lane_colours():
    """The rank colours compiled into libflingsim (csrc/fs_panels.hip), uint8 [8, 3]."""
    import ctypes as C

    from .sim import load_library
    lib = load_library()
    out = np.zeros((LANE_MAX, 3), np.uint8)
    if lib.fs_lane_colours(out.ctypes.data_as(C.POINTER(C.c_ubyte)), out.size) != 0:
        raise RuntimeError("fs_lane_colours: " + lib.fs_last_error().decode())
    return out


def compose_lanes(items, lanes, panel=200):
    """The strips of a list of look-ahead steps (fs_lane_panels): ONE table upload, ONE launch, ONE download.  An item is a
    dictionary of
      before [>= 3, S, S] (float32 CUDA tensor): the observation all lanes started from
      lanes: one dictionary per EXECUTED lane in rank order, at most `lanes`: after [>= 3, S, S] or None, prims: a primitive
             list (action_overlays) for the S x S panel, at most 8
      followed: the rank the episode continued from, or -1 / None.
    Returns uint8 [len(items), panel, (1 + lanes) * panel, 3] (numpy): before + every lane's action | after lane 0 | ..."""
    import torch

    from .sim import stream_call, work_buffer
    panel, lanes = int(panel), int(lanes)
    if not 1 <= lanes <= LANE_MAX:
        raise ValueError(f"compose_lanes: 1 .. {LANE_MAX} lanes, got {lanes}")
    if not items:
        return np.zeros((0, panel, (1 + lanes) * panel, 3), np.uint8)
    dev = items[0]["before"].device
    S = int(items[0]["before"].shape[-1])
    table = np.zeros(len(items), LANE_RECORD)
    for k, it in enumerate(items):
        before = _plane(it["before"], "before")
        if len(it["lanes"]) > lanes:
            raise ValueError(f"compose_lanes: item {k}: {len(it['lanes'])} lanes on a strip of {lanes}")
        row = table[k]
        afters = [None if lane.get("after") is None else _plane(lane["after"], "after") for lane in it["lanes"]]
        for name, t in [("before", before)] + [("after", t) for t in afters]:
            if t is not None and (t.dim() != 3 or t.shape[0] < 3 or tuple(t.shape[1:]) != (S, S)):
                raise ValueError(f"compose_lanes: item {k}: {name} has shape {tuple(t.shape)}, expected [>= 3, {S}, {S}]")
            if t is not None and t.device != dev:
                raise ValueError(f"compose_lanes: item {k} lives on another device")
        row["before"], row["n_lanes"] = before.data_ptr(), len(it["lanes"])
        row["followed"] = -1 if it.get("followed") is None else int(it["followed"])
        for j, (lane, after) in enumerate(zip(it["lanes"], afters)):
            row["after"][j] = 0 if after is None else after.data_ptr()
            prims = np.asarray(lane.get("prims", ()), np.int64).reshape(-1, 9)
            if len(prims) > MAX_PRIMS:
                raise ValueError(f"compose_lanes: item {k}: {len(prims)} primitives on lane {j} (at most {MAX_PRIMS})")
            if prims.size and np.abs(prims).max() > 2 ** 31 - 1:
                raise ValueError(f"compose_lanes: item {k}: a primitive does not fit an int")
            row["n_prims"][j] = len(prims)
            row["prims"][j, :len(prims)] = prims
    out = torch.empty((len(items), panel, (1 + lanes) * panel, 3), dtype=torch.uint8, device=dev)
    work = work_buffer("fs_lane_panels_work_bytes", dev, len(items))
    stream_call("fs_lane_panels", dev, table.ctypes.data, len(items), lanes, S, panel, out, work)
    return out.cpu().numpy()


def probe_range(predicted, measured):
    """The default colour range of a probe strip: float32 (min, max) over the predicted values at the executed cells (finite
    `measured`) and the measured values themselves, finite ones only; (0, 0) when there is none."""
    p, m = np.asarray(predicted, np.float32), np.asarray(measured, np.float32)
    done = np.isfinite(m)
    v = np.concatenate([p[done & np.isfinite(p)], m[done]])
    return np.array([v.min(), v.max()], np.float32) if v.size else np.zeros(2, np.float32)


def compose_probe(items, panel=200):
    """The strips of a list of probed maps (fs_probe_panels): ONE table upload, ONE launch, ONE download.  An item is a
    dictionary of
      stack [4, D, D], value_map [D, D], after [>= 3, S, S] or None (float32 CUDA tensors): the chosen stack entry, the chosen
          primitive's map of the chosen transform, the observation after the best-measured cell's lane
      measured float32 [gy, gz] (NaN: not executed), valid bool or uint8 [gy, gz]: numpy arrays or CUDA tensors, in whatever
          unit the value map is in
      predicted float32 [gy, gz] (numpy): the value map at the cells -- only read for the default range
      range: (vmin, vmax) or None: `probe_range(predicted, measured)`
      origin (y0, z0), stride, chosen_cell (i, j) or None, small: a primitive list (action_overlays) for the D x D panel.
    Returns uint8 [len(items), panel, 4 * panel, 3] (numpy)."""
    import torch

    from .sim import stream_call, work_buffer
    panel = int(panel)
    if not items:
        return np.zeros((0, panel, 4 * panel, 3), np.uint8)
    first = items[0]
    D = int(first["stack"].shape[-1])
    dev = first["stack"].device
    S = next((int(it["after"].shape[-1]) for it in items if it.get("after") is not None), 1)
    table = np.zeros(len(items), PROBE_RECORD)
    keep = []   # the planes made here live until the download
    for k, it in enumerate(items):
        stack, vmap = _plane(it["stack"], "stack"), _plane(it["value_map"], "value_map")
        after = None if it.get("after") is None else _plane(it["after"], "after")
        if tuple(stack.shape) != (4, D, D) or tuple(vmap.shape) != (D, D):
            raise ValueError(f"compose_probe: item {k}: stack {tuple(stack.shape)}, value map {tuple(vmap.shape)}")
        if after is not None and (after.dim() != 3 or after.shape[0] < 3 or tuple(after.shape[1:]) != (S, S)):
            raise ValueError(f"compose_probe: item {k}: after has shape {tuple(after.shape)}, expected [>= 3, {S}, {S}]")
        measured, valid = it["measured"], it["valid"]
        if not torch.is_tensor(measured):
            measured = torch.from_numpy(np.ascontiguousarray(measured, np.float32)).to(dev)
        if not torch.is_tensor(valid):
            valid = torch.from_numpy(np.ascontiguousarray(valid).astype(np.uint8)).to(dev)
        measured, valid = _plane(measured, "measured"), valid.to(torch.uint8).contiguous()
        if measured.dim() != 2 or valid.shape != measured.shape:
            raise ValueError(f"compose_probe: item {k}: measured {tuple(measured.shape)}, valid {tuple(valid.shape)}")
        vrange = it.get("range")
        if vrange is None:
            vrange = probe_range(it["predicted"], measured.cpu().numpy())
        if not torch.is_tensor(vrange):
            vrange = torch.from_numpy(np.ascontiguousarray(vrange, np.float32)).to(dev)
        vrange = _plane(vrange, "range")
        if vrange.numel() != 2:
            raise ValueError(f"compose_probe: item {k}: range {tuple(vrange.shape)}")
        if any(t is not None and t.device != dev for t in (stack, vmap, after, measured, valid, vrange)):
            raise ValueError(f"compose_probe: item {k} lives on another device")
        keep += [measured, valid, vrange]
        row = table[k]
        row["stack"], row["value_map"], row["range"], row["measured"], row["code"] = (
            t.data_ptr() for t in (stack, vmap, vrange, measured, valid))
        row["after"] = 0 if after is None else after.data_ptr()
        row["y0"], row["z0"] = (int(v) for v in it["origin"])
        row["stride"], (row["gy"], row["gz"]) = int(it["stride"]), measured.shape
        row["cy"], row["cz"] = (-1, -1) if it.get("chosen_cell") is None else (int(v) for v in it["chosen_cell"])
        prims = np.asarray(it.get("small", ()), np.int64).reshape(-1, 9)
        if len(prims) > MAX_PRIMS:
            raise ValueError(f"compose_probe: item {k}: {len(prims)} primitives on a panel (at most {MAX_PRIMS})")
        if prims.size and np.abs(prims).max() > 2 ** 31 - 1:
            raise ValueError(f"compose_probe: item {k}: a primitive does not fit an int")
        row["n_small"] = len(prims)
        row["small"][:len(prims)] = prims
    out = torch.empty((len(items), panel, 4 * panel, 3), dtype=torch.uint8, device=dev)
    work = work_buffer("fs_probe_panels_work_bytes", dev, len(items))
    stream_call("fs_probe_panels", dev, table.ctypes.data, len(items), D, S, panel, out, work)
    return out.cpu().numpy()


# ---- files --------------------------------------------------------------------------------------------------------------------
def write_png(path, array):
    """One 8-bit RGB (uint8 [H, W, 3]) or grey (uint8 [H, W]) image as a PNG, with zlib and struct alone (the chunk layout
    taskio.FrameDump writes for its films)."""
    import struct
    import zlib

    a = np.ascontiguousarray(array)
    if a.dtype != np.uint8 or not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)) or a.size == 0:
        raise ValueError(f"write_png: uint8 [H, W, 3] or [H, W], got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    channels = 1 if a.ndim == 2 else 3

    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xffffffff)

    rows = np.zeros((h, 1 + channels * w), np.uint8)          # filter type 0 per scanline
    rows[:, 1:] = a.reshape(h, channels * w)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0 if channels == 1 else 2, 0, 0, 0)))
        f.write(chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)))
        f.write(chunk(b"IEND", b""))
    return path


def read_actions(directory):
    """The lines of <directory>/actions.jsonl as dictionaries, in key order."""
    path = os.path.join(str(directory), ACTIONS_FILE)
    rows = []
    if os.path.exists(path):
        with open(path) as f:
            rows = [json.loads(line) for line in f if line.strip()]
    return sorted(rows, key=lambda r: str(r["key"]))


def write_report(directory):
    """<directory>/index.html from <directory>/actions.jsonl: one table row per action in key order -- key, primitive, coverage
    before and after over max_coverage, the strip, and a link to the episode's film where one was recorded.  The strips are
    named relative to the directory, so it can be moved as a whole; a film lies outside it and its link is the way from the
    directory to the film (actions.jsonl holds the film directory as an absolute path; one found relative there is taken
    from the working directory, as the run that wrote it took it).  Returns the file's path."""
    from html import escape

    directory = str(directory)
    rows = read_actions(directory)

    def rel(p):      # a strip: listed relative to the directory
        p = str(p)
        return os.path.relpath(p, directory) if os.path.isabs(p) else p

    def way_to(p):   # a film: somewhere else
        return os.path.relpath(os.path.abspath(str(p)), os.path.abspath(directory))

    def share(r, name):
        mx = float(r.get("max_coverage") or 0.0)
        v = r.get(name)
        return "" if v is None or mx <= 0.0 else f"{100.0 * float(v) / mx:.1f} %"

    lines = ["<!DOCTYPE html>", '<html lang="en">', "<head>", '<meta charset="utf-8">', "<title>Action report</title>",
             "</head>", "<body>", f"<h1>Action report: {len(rows)} actions</h1>",
             "<p>Each strip, left to right: observation before, value map, the action on what the net saw, "
             "the action on the observation, observation after.</p>",
             '<table border="1" cellpadding="4">',
             "<tr><th>key</th><th>primitive</th><th>coverage before</th><th>coverage after</th><th>strip</th><th>film</th></tr>"]
    if any("lanes" in r for r in rows):
        lines.insert(-2, "<p>A look-ahead step's strip: the observation before with every executed lane's action in its rank colour, "
                         "then the observation after each lane, framed in its rank colour; the followed lane has a white inner "
                         "frame.  Regret: (best reward - rank-0 reward) / max_coverage.</p>")
    if any("probe" in r for r in rows):
        lines.insert(-2, "<p>A probed map's strip: what the net saw with the chosen action, the predicted map, the measured map "
                         "(reward / max_coverage per lattice cell, the same colour range; light grey: valid and not executed, dark "
                         "grey: invalid, white frame: the chosen cell), the observation after the best-measured cell.  Lattice "
                         "regret: (best reward - chosen reward) / max_coverage.</p>")
    for r in rows:
        if "probe" in r:   # a probed map (probe.run_episodes): one row per (task, step)
            png, st, pr = escape(rel(r["png"]), quote=True), r.get("stats") or {}, r["probe"]
            show = lambda v, digits=4: "-" if v is None else format(float(v), f".{digits}f")   # noqa: E731
            detail = (f'{escape(str(r["primitive"]))}, map {int(pr["transform_index"])}, {pr["shape"][0]} x {pr["shape"][1]} cells, '
                      f'{int(pr["n_executed"])} executed<br>lattice regret {show(st.get("lattice_regret"))}<br>Spearman '
                      f'{show(st.get("spearman"), 3)}<br>chosen rank {"-" if st.get("chosen_rank") is None else int(st["chosen_rank"])}'
                      f'<br>pairs {int(st.get("concordant", 0))} / {int(st.get("pairs", 0))} concordant')
            lines.append(f'<tr><td>{escape(str(r["key"]))}</td><td>{detail}</td><td></td><td></td>'
                         f'<td><img src="{png}" alt="{escape(str(r["key"]), quote=True)}"></td><td></td></tr>')
            continue
        if "lanes" in r:   # a look-ahead step (lookahead.run_episodes): one row per step, all lanes on one strip
            png = escape(rel(r["png"]), quote=True)
            mx = float(r.get("max_coverage") or 0.0)
            rewards = [float(c["reward"]) for c in r["lanes"]]
            regret = "" if not rewards or mx <= 0.0 else f"regret {(max(rewards) - rewards[0]) / mx:.4f}"
            per_lane = "<br>".join(escape(f'rank {int(c["rank"])}: {c["primitive"]}, value {float(c["value"]):.4f}, reward '
                                          + (f'{100.0 * float(c["reward"]) / mx:.1f} %' if mx > 0.0 else f'{float(c["reward"]):.4f}'))
                                   for c in r["lanes"])
            lines.append(f'<tr><td>{escape(str(r["key"]))}</td><td>look-ahead, {len(r["lanes"])} lanes, followed rank '
                         f'{int(r.get("followed_rank", 0))}<br>{regret}<br>{per_lane}</td>'
                         f'<td>{share(r, "preaction_coverage")}</td><td>{share(r, "postaction_coverage")}</td>'
                         f'<td><img src="{png}" alt="{escape(str(r["key"]), quote=True)}"></td><td></td></tr>')
            continue
        film = ""
        if r.get("film_dir"):
            from .taskio import VIDEO_NAME
            film = f'<a href="{escape(way_to(os.path.join(str(r["film_dir"]), VIDEO_NAME)), quote=True)}">film</a>'
        png = escape(rel(r["png"]), quote=True)
        detail = f'rotation {float(r.get("rotation", 0.0)):.1f}, scale {float(r.get("scale", 0.0)):.3f}'
        lines.append(f'<tr><td>{escape(str(r["key"]))}</td><td>{escape(str(r["primitive"]))}<br>{escape(detail)}</td>'
                     f'<td>{share(r, "preaction_coverage")}</td><td>{share(r, "postaction_coverage")}</td>'
                     f'<td><img src="{png}" alt="{escape(str(r["key"]), quote=True)}"></td><td>{film}</td></tr>')
    lines += ["</table>", "</body>", "</html>", ""]
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, "index.html")
    with open(path, "w") as f:
        f.write("\n".join(lines))
    return path


SUMMARY_SKIPS = ("distribution", "img", "min", "max", "_steps")   # statistics that are not one number to read (visualize.py:18-19)
LENGTH_ROWS = (("mean", np.mean), ("25-quantile", lambda v: np.quantile(v, 0.25)), ("median", np.median),
               ("75-quantile", lambda v: np.quantile(v, 0.75)))


def summary_lines(stats):
    """The text visualize.summarize prints before its plots (visualize.py:15-43) for one collect_stats dictionary, as lines:
    one row per statistic whose key holds none of SUMMARY_SKIPS -- the key left-justified to 36 characters in brackets, the
    value with four decimals --, then the episode lengths per difficulty: mean, lower quartile, median, upper quartile.  As
    there, the easy header is printed whether or not the run had easy tasks, the hard block only when it had hard ones, and
    the hard figures carry two decimals where the easy ones carry four."""
    lines = []
    for key, value in stats.items():
        if not any(word in key for word in SUMMARY_SKIPS):
            lines.append("\t[" + key.ljust(36) + "]:\t" + format(float(value), ".4f"))
    for level, digits, always in (("easy", 4, True), ("hard", 2, False)):
        lengths = stats.get(f"episode_length/{level}/distribution")
        if always or lengths is not None:
            lines.append(f"{level.capitalize()} Episode Lengths:")
        if lengths is not None:
            lines += [f"\t{name}: " + format(float(fn(lengths)), f".{digits}f") for name, fn in LENGTH_ROWS]
    return lines


def summarize(replay_paths, file=None):
    """visualize.summarize's printed summary for every file written by taskio.save_replay: the file's name, then
    summary_lines of taskio.collect_stats over ALL entries of the file.  The seaborn plots are not made (pandas and seaborn
    are absent here)."""
    from .taskio import collect_stats
    if isinstance(replay_paths, (str, bytes)) or hasattr(replay_paths, "__fspath__"):
        replay_paths = [replay_paths]
    for path in replay_paths:
        print(f"{path}:", file=file)
        for line in summary_lines(collect_stats(path, num_points=int(1e7))):
            print(line, file=file)


# ---- what BatchedFlingEnv keeps of an action, and where the strips go ----------------------------------------------------------
class ActionLog:
    """Where the strips of a run go: <root>/<episode name>/step{k:02d}.png plus one line per action in <root>/actions.jsonl,
    or -- without a root -- nowhere (the caller keeps the arrays)."""

    def __init__(self, root):
        self.root = None if root is None else str(root)
        if self.root is not None:
            os.makedirs(self.root, exist_ok=True)
            open(os.path.join(self.root, ACTIONS_FILE), "w").close()     # a run starts its own list

    def write(self, name, meta, strip, suffix=""):
        """One action: the png and the line.  meta: the held item's 'meta' dictionary, completed by the caller.  suffix: what
        the file's name carries after the step number ("_lanes" for a look-ahead step's lane strip)."""
        folder = os.path.join(self.root, str(name))
        os.makedirs(folder, exist_ok=True)
        png = os.path.join(folder, f"step{int(meta['step']):02d}{suffix}.png")
        write_png(png, strip)
        line = dict(meta, png=os.path.relpath(png, self.root))
        if line.get("film_dir"):     # (given relative to the run's working directory; the page is read from elsewhere)
            line["film_dir"] = os.path.abspath(str(line["film_dir"]))
        with open(os.path.join(self.root, ACTIONS_FILE), "a") as f:
            f.write(json.dumps(line) + "\n")
        return png
