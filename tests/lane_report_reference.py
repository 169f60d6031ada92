"""The rules of fs_lane_panels (include/flingsim.h) restated in numpy on top of tests/report_reference.py -- the reference
the kernel is compared with byte for byte (tests/test_lane_panels_gpu.py).  Not a test module.

A whole image at a time: the lanes' primitives are drawn lane after lane with report_reference.draw's own rule (the last
primitive that covers a pixel gives its colour, blended once), the frames are boolean masks over the destination panel."""
import numpy as np

import report_reference as ref

# include/flingsim.h, "rank colours"
RANK_COLOURS = np.array([(230, 25, 75), (60, 180, 75), (0, 130, 200), (245, 130, 48), (145, 30, 180), (70, 240, 240),
                         (240, 50, 230), (255, 225, 25)], np.uint8)
WHITE = np.array([255, 255, 255], np.uint8)


def frame_width(panel):
    """t = max(1, panel / 50) in integer division"""
    return max(1, int(panel) // 50)


def edge_distance(panel):
    """int64 [panel, panel]: min(y, x, panel - 1 - y, panel - 1 - x)"""
    y, x = np.meshgrid(np.arange(panel, dtype=np.int64), np.arange(panel, dtype=np.int64), indexing="ij")
    return np.minimum(np.minimum(y, x), np.minimum(panel - 1 - y, panel - 1 - x))


def frame(image, rank, followed):
    """uint8 [panel, panel, 3] with the frame of lane `rank` written over it: the rank colour where the edge distance is
    below t, white where it lies in [t, 2 t) on the followed lane's panel.  Overwrites, no blend."""
    panel = image.shape[0]
    m, t = edge_distance(panel), frame_width(panel)
    out = image.copy()
    if followed:
        out[(m >= t) & (m < 2 * t)] = WHITE
    out[m < t] = RANK_COLOURS[rank]
    return out


def recolour(prims, rank):
    """A lane's primitives with the lane's rank colour in place of their own."""
    return [tuple(int(c) for c in p[:6]) + tuple(int(c) for c in RANK_COLOURS[rank]) for p in prims]


def before_panel(before, lanes_prims):
    """uint8 [S, S, 3]: the observation with every lane's primitives on it, in rank order."""
    prims = [p for rank, lane in enumerate(lanes_prims) for p in recolour(lane, rank)]
    return ref.draw(ref.image_of(before), prims)


def strip(before, afters, lanes_prims, followed, lanes, panel):
    """uint8 [panel, (1 + lanes) * panel, 3].  afters / lanes_prims: one entry per EXECUTED lane (an after may be None);
    followed: a rank or -1; lanes: the strip's lane count."""
    assert len(afters) == len(lanes_prims) <= lanes
    parts = [ref.sample(before_panel(before, lanes_prims), panel)]
    for rank in range(lanes):
        if rank >= len(afters) or afters[rank] is None:
            parts.append(np.zeros((panel, panel, 3), np.uint8))
        else:
            parts.append(frame(ref.sample(ref.image_of(afters[rank]), panel), rank, rank == followed))
    return np.concatenate(parts, axis=1)
