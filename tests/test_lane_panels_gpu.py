"""fs_lane_panels (csrc/fs_panels.hip) through report.compose_lanes against tests/lane_report_reference.py, byte for byte, and
its refusals with a real output buffer behind them."""
import numpy as np
import pytest
import torch

import lane_report_reference as lref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FS_ERR_ARG = -1


def _records(S, lanes, n, seed):
    """n records that between them hold the cases of the list: fewer lanes than the strip has, a null after, followed = -1 and
    every rank, primitives partly and wholly outside the image and at +-8191, two lanes on one pixel.  Host arrays."""
    from flingbot_amd.report import RING, SEGMENT, action_overlays
    rng = np.random.default_rng(seed)
    at = lambda fy, fx: (int(fy * (S - 1)), int(fx * (S - 1)))   # noqa: E731
    out = []
    for r in range(n):
        n_lanes = lanes if r % 2 == 0 else max(1, lanes - 1 - r // 2)          # record 1, 3: fewer lanes than panels
        before = rng.uniform(-0.2, 1.2, (4, S, S)).astype(np.float32)          # four planes: three are shown
        before[0, 0, :3] = [np.nan, 1.0, 0.0]
        afters, prims = [], []
        for j in range(n_lanes):
            after = rng.uniform(-0.2, 1.2, (3 + j % 2, S, S)).astype(np.float32)
            afters.append(None if (r, j) in ((0, lanes - 1), (3, 0)) and n_lanes > 1 else after)
            a, b = at(rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.9)), at(rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.9))
            lane = action_overlays(("fling", "stretchdrag", "drag", "place")[(r + j) % 4], np.array([a, b]), 1 + (r + j) % 3)
            if j == 0:   # every lane-0 list crosses the image's middle row, every lane-1 list its middle column: one shared pixel
                lane = lane[:6] + [(SEGMENT, S // 2, -3, S // 2, S + 2, 1, 1, 2, 3), (RING, S + 40, S + 40, 6, 0, 3, 9, 9, 9)]
            elif j == 1:
                lane = lane[:5] + [(SEGMENT, -8191, S // 2, 8191, S // 2, 1 + r % 2, 4, 5, 6), (RING, 0, 0, 8191, 0, 64, 0, 0, 0),
                                   (SEGMENT, -8191, -8191, -20, -20, 64, 255, 255, 255)]
            elif j == 2:
                lane = lane + [(RING, S - 1, S - 1, 4, 0, 2, 7, 7, 7)]           # a ring on the corner: partly outside
            assert len(lane) <= 8
            prims.append(lane)
        followed = (-1, 0, n_lanes - 1, min(1, n_lanes - 1), n_lanes // 2)[r % 5]
        out.append(dict(before=before, afters=afters, prims=prims, followed=followed))
    return out


def _item(rec):
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    return dict(before=up(rec["before"]), followed=rec["followed"],
                lanes=[dict(after=up(a), prims=p) for a, p in zip(rec["afters"], rec["prims"])])


def _want(rec, lanes, panel):
    return lref.strip(rec["before"], rec["afters"], rec["prims"], rec["followed"], lanes, panel)


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("S,panel,lanes", [(16, 8, 1), (33, 37, 3), (128, 200, 8)])
def test_lane_panels_match_reference(gpu_required, S, panel, lanes, n):
    from flingbot_amd import report

    host = _records(S, lanes, n, seed=100 * S + n)
    dev = [_item(r) for r in host]
    got = report.compose_lanes(dev, lanes, panel=panel)
    assert got.dtype == np.uint8 and got.shape == (n, panel, (1 + lanes) * panel, 3)
    for k, rec in enumerate(host):
        want = _want(rec, lanes, panel)
        diff = np.argwhere(got[k] != want)
        assert diff.size == 0, (k, len(diff), diff[:4], got[k][tuple(diff[0][:2])], want[tuple(diff[0][:2])])
        for j in range(lanes):   # a lane that was not executed, or a null after: black, and no frame
            if j >= len(rec["afters"]) or rec["afters"][j] is None:
                assert not got[k][:, (1 + j) * panel:(2 + j) * panel].any(), (k, j)
    if n > 1:   # a record alone equals the same record inside the batch (odd strips start off the dword grid)
        for k in (1, n - 1):
            assert (report.compose_lanes([dev[k]], lanes, panel=panel)[0] == got[k]).all(), k


def test_lane_panels_show_what_they_should(gpu_required):
    """The kernel and the reference could agree on drawing nothing: the overlays, the shared pixel and the frames, looked at
    directly."""
    from flingbot_amd import report

    S, panel, lanes = 128, 128, 3                                            # panel == S: destination pixel = source pixel
    rec = _records(S, lanes, 1, seed=9)[0]
    rec["afters"] = [np.full((3, S, S), 0.5, np.float32) for _ in range(lanes)]
    got = report.compose_lanes([_item(dict(rec, followed=f)) for f in (-1, 0, 1, 2)], lanes, panel=panel)
    colours = report.lane_colours().astype(int)
    assert (colours == lref.RANK_COLOURS).all()
    base = lref.ref.image_of(rec["before"]).astype(int)
    mid = S // 2
    blend = lambda c, at: tuple((9 * c + base[at] + 5) // 10)   # noqa: E731
    covering = [j for j, lane in enumerate(rec["prims"]) if any(lref.ref.mask_of(p, S)[mid, mid] for p in lane)]
    assert covering[:2] == [0, 1]                                            # lane 0's row and lane 1's column cross there
    assert tuple(got[0][mid, mid]) == blend(colours[covering[-1]], (mid, mid))   # the LAST lane that covers it, blended once
    bare = report.compose_lanes([_item(dict(rec, prims=[[], [], []]))], lanes, panel=panel)[0]
    assert (bare[:, :panel] == base).all()
    assert ((got[0][:, :panel] != bare[:, :panel]).any(axis=2)).sum() > S    # the overlays are there, on panel 0 only
    assert (got[0][:, panel:] == bare[:, panel:]).all()
    t = lref.frame_width(panel)
    assert t == 2
    for f, strip in zip((-1, 0, 1, 2), got):
        assert (strip == lref.strip(rec["before"], rec["afters"], rec["prims"], f, lanes, panel)).all(), f
        assert (strip[:, :panel] == got[0][:, :panel]).all()                 # `followed` does not touch panel 0
        for j in range(lanes):
            p = strip[:, (1 + j) * panel:(2 + j) * panel]
            assert (p[0] == colours[j]).all() and (p[:, t - 1] == colours[j]).all() and (p[panel - 1] == colours[j]).all()
            inner = (255, 255, 255) if j == f else (127, 127, 127)
            assert tuple(p[t, t]) == inner and tuple(p[2 * t - 1, 2 * t - 1]) == inner and tuple(p[panel - 2 * t, mid]) == inner
            assert tuple(p[2 * t, 2 * t]) == (127, 127, 127) and tuple(p[mid, mid]) == (127, 127, 127)


def test_lane_panels_refusals_leave_the_output_untouched(gpu_required):
    from flingbot_amd import report, sim as fsim

    lib = fsim.load_library()
    S, panel, lanes = 16, 8, 2
    rec = _records(S, lanes, 1, seed=3)[0]
    rec["afters"], rec["followed"] = [np.zeros((3, S, S), np.float32)] * lanes, 1
    item = _item(rec)
    out = torch.full((2, panel, (1 + lanes) * panel, 3), 0xAB, dtype=torch.uint8, device=DEV)
    work = fsim.work_buffer("fs_lane_panels_work_bytes", DEV, 2)

    def table():
        t = np.zeros(1, report.LANE_RECORD)
        t["before"], t["n_lanes"], t["followed"] = item["before"].data_ptr(), lanes, 1
        for j, lane in enumerate(item["lanes"]):
            t["after"][0, j] = lane["after"].data_ptr()
            t["n_prims"][0, j] = len(lane["prims"])
            t["prims"][0, j, :len(lane["prims"])] = lane["prims"]
        return t

    def call(t, n=1, lanes_=lanes, S_=S, panel_=panel, out_=None, work_=None):
        out_ = out.data_ptr() if out_ is None else out_
        work_ = work.data_ptr() if work_ is None else work_
        with torch.cuda.device(0):
            return lib.fs_lane_panels(None if t is None else t.ctypes.data, n, lanes_, S_, panel_, out_ or None, work_ or None,
                                      torch.cuda.current_stream().cuda_stream)

    def edited(field, value, *index):
        t = table()
        if index:
            t[field][(0,) + index] = value
        else:
            t[field] = value
        return t

    big = np.concatenate([table()] * 2)
    refused = [call(None), call(table(), out_=0), call(table(), work_=0), call(table(), n=0), call(big, n=65536),
               call(table(), lanes_=0), call(table(), lanes_=9), call(edited("n_lanes", 0)), call(edited("n_lanes", lanes + 1)),
               call(edited("followed", -2)), call(edited("followed", lanes)), call(edited("n_prims", 9, 0)),
               call(edited("prims", 2, 0, 0, 0)), call(edited("prims", 8192, 0, 0, 1)), call(edited("prims", -8192, 1, 0, 4)),
               call(edited("prims", 0, 0, 0, 5)), call(edited("prims", 65, 0, 0, 5)), call(edited("prims", 256, 0, 0, 6)),
               call(edited("prims", -1, 0, 0, 8)), call(table(), S_=0), call(table(), S_=4097), call(table(), panel_=0),
               call(table(), panel_=4097), call(table(), work_=work.data_ptr() + 4), call(table(), out_=out.data_ptr() + 1),
               call(edited("before", 0)), call(edited("after", item["before"].data_ptr() + 2, 1))]
    assert refused == [FS_ERR_ARG] * len(refused)
    assert lib.fs_last_error()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xAB).all()                                 # nothing was launched
    # the same table, unedited, is served -- into the first strip only
    assert call(table()) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[0] == _want(rec, lanes, panel)).all() and (got[1] == 0xAB).all()
