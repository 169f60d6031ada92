"""The exact-arithmetic rasteriser reference (tests/raster_reference.py) against the C restatement of the kernel
(oracle/raster_oracle.c) on the synthetic scenes of tests/raster_scenes.py.  No GPU: this pins the two checkers of
tests/test_raster_synthetic_gpu.py and tests/test_render_gpu.py to each other, and the reference's two restated float32
stages to float64."""
import numpy as np
import pytest

import raster_reference as rr
import raster_scenes as rs

SCENES = rs.all_scenes()


def _oracle_render(sc, want_color=True):
    from oracle.render import render as orc_render

    ref = rs.reference(sc, want_color)
    orc = rs._oracle_side(sc)[0]
    m = ref["mats"]
    mats = np.concatenate([m["view"].ravel(), m["proj"].ravel(), m["light"].ravel(), m["lightpos"], m["lightdir"]])
    rgba, depth = orc_render(mats, np.array(sc.cam_pos, np.float32), sc.W, sc.H, orc.get_positions(), orc.get_normals(),
                             orc.get_faces(), orc.get_shape_states(), [s[0] for s in sc.spheres])
    return rgba.reshape(sc.H, sc.W, 4), depth.reshape(sc.H, sc.W)


def check_against(ref, rgba, depth, colour=True):
    """depth bit for bit (pixels under the margin aside), alpha exact, colour within 1 LSB and differing on < 2 % of the
    channels (the figures of test_render_matches_raster_oracle)."""
    sure = ~(ref["margin"] < rr.MARGIN_LSB)
    bad = (depth.view(np.uint32) != ref["depth"].view(np.uint32)) & sure
    assert not bad.any(), f"{bad.sum()} depth pixels differ, first at {np.argwhere(bad)[0]}"
    assert np.array_equal(rgba[..., 3][sure], ref["rgba"][..., 3][sure])
    if colour:
        diff = np.abs(rgba[..., :3].astype(int) - ref["rgba"][..., :3].astype(int))[sure]
        assert diff.max(initial=0) <= 1, f"max colour difference {diff.max()} on {(diff > 1).sum()} channels"
        assert (diff > 0).mean() < 0.02 if diff.size else True, (diff > 0).mean()


@pytest.mark.parametrize("sc", SCENES, ids=repr)
def test_margin_excludes_no_pixel(sc):
    """On the committed seeds no exact depth lies within MARGIN_LSB of a rounding or discard boundary: the bit comparisons
    leave nothing out (the condition would allow 0.1 % of the covered pixels)."""
    ref = rs.reference(sc)
    assert not (ref["margin"] < rr.MARGIN_LSB).any(), ref["margin"].min()
    assert not (ref["shadow_margin"] < rr.MARGIN_LSB).any(), ref["shadow_margin"].min()


@pytest.mark.parametrize("sc", SCENES, ids=repr)
def test_reference_equals_raster_oracle(sc):
    rgba, depth = _oracle_render(sc)
    check_against(rs.reference(sc), rgba, depth)


def test_reference_equals_raster_oracle_720():
    """The folded mesh once at the product's frame size (depth and alpha only: the float64 shading of half a million pixels
    is checked on the small frames)."""
    sc = rs.fold_720()
    ref = rs.reference(sc, False)
    rgba, depth = _oracle_render(sc, False)
    sure = ~(ref["margin"] < rr.MARGIN_LSB)
    assert (~sure).sum() <= 1e-3 * (ref["keys"] != rr.CLEARED_KEY).sum()
    assert np.array_equal(depth.view(np.uint32)[sure], ref["depth"].view(np.uint32)[sure])
    assert np.array_equal(rgba[..., 3] == 255, ref["keys"] != rr.CLEARED_KEY)


@pytest.mark.parametrize("sc", SCENES, ids=repr)
def test_vertex_stage_within_float32_bound(sc):
    """The restated float32 vertex stage against float64, camera and light pass: window x / y and window depth within the
    bound derived in raster_reference.vertex_stage64: a few ulp of the frame's size for points in front of a camera near the
    origin, more where 1 / w or a distant origin amplifies (the sphere around the camera, the tent 20 m out)."""
    ref = rs.reference(sc)
    fr = ref["frame"]
    verts = sc.pos[:, :3] if ref["mesh"][0] is None else np.concatenate([ref["mesh"][0][:, :3], sc.pos[:, :3]])
    for m, W, H in ((fr.vp, fr.W, fr.H), (fr.light, rr.SHADOW_RES, rr.SHADOW_RES)):
        v32, v64 = rr.vertex_stage(m, W, H, verts), rr.vertex_stage64(m, W, H, verts)
        ok = v32["ok"]
        assert np.array_equal(ok, (v64["w"] > 1e-6) & (np.abs(v64["fx"]) < 1e6) & (np.abs(v64["fy"]) < 1e6))
        for name in ("fx", "fy", "d"):
            err = np.abs(v32[name].astype(np.float64) - v64[name])[ok]
            assert (err <= v64[name + "_bound"][ok]).all(), (name, (err / v64[name + "_bound"][ok]).max())


@pytest.mark.parametrize("sc", [s for s in SCENES if s.cam_pos[1] < 3.0 and s.W > 1], ids=repr)
def test_ground_plane_within_float32_bound(sc):
    """The restated float32 ground ray against the analytic depth: the plane y = 0 seen from straight above at height c has
    window depth (f + n) / (2 (f - n)) - f n / ((f - n) c) + 1 / 2 at every pixel; a dozen float32 roundings on values <= 2
    may move it by 12 2^-24 (about 12 depth24 steps), no more."""
    ref = rs.reference(sc)
    keys, _ = rr.ground_keys(ref["frame"])
    assert (keys != rr.CLEARED_KEY).all()
    n, f, c = 0.01, 3.0, float(sc.cam_pos[1])
    d = (f + n) / (2 * (f - n)) - f * n / ((f - n) * c) + 0.5
    q = (keys >> np.uint64(32)).astype(np.float64)
    assert np.abs(q - d * rr.DEPTH_MAX).max() <= 12.5, np.abs(q - d * rr.DEPTH_MAX).max()


def test_tan_half_fov_is_consistent_with_the_projection():
    fr = rs.reference(SCENES[0])["frame"]
    assert np.float32(1.0) / fr.tan_half_fov == fr.proj[1, 1]


def test_lattice_covers_exactly_its_cells():
    """Every shared edge and vertex of the aligned lattice passes through pixel centres.  From the fill rule alone: a centre
    on a left edge or on a top edge (rows run bottom-up: the edge of largest y) is inside, one on a right or bottom edge is
    not, so the lattice spanning centres 28 .. 68 x 12 .. 52 covers columns 28 .. 67 and rows 13 .. 52, each pixel exactly
    once, by the triangle of its own cell: no hole, nothing outside.  Shifted by half a pixel no centre lies on an edge and
    the same 40 x 40 block (columns 28 .. 67, rows 12 .. 51) is covered."""
    for sc, rows in ((SCENES[0], slice(13, 53)), (SCENES[1], slice(12, 52))):
        ref = rs.reference(sc)
        vs = rr.vertex_stage(ref["frame"].vp, sc.W, sc.H, sc.pos[:, :3])
        off = 128 if sc is SCENES[0] else 0
        assert ((vs["X"] - off) % (5 * 256) == 28 * 256 % (5 * 256)).all() and ((vs["Y"] - off) % (5 * 256) == 12 * 256 % (5 * 256)).all()
        covered = ref["zkeys"] != rr.CLEARED_KEY
        expect = np.zeros((sc.H, sc.W), bool)
        expect[rows, 28:68] = True
        assert np.array_equal(covered, expect)
        # the id at (row, column): the cell it falls into, and which side of the cell's diagonal
        ids = (ref["zkeys"] & np.uint64(0xFFFFFFFF)).astype(np.int64)[rows, 28:68] - 1
        faces = ref["faces"]
        cell = ids // 2
        # local row / column of the covered block -> cell: five pixels per cell either way, because a centre on a cell's
        # upper edge goes to that cell and one on its left edge too.  Window x runs against iz, window y against ix.
        py, px = np.meshgrid(np.arange(40), np.arange(40), indexing="ij")
        cell_ix, cell_iz = 7 - py // 5, 7 - px // 5
        assert np.array_equal(cell, cell_iz * 8 + cell_ix), "a pixel went to a triangle of another cell"
        assert set(np.unique(ids)) == set(range(len(faces))), "every triangle of the lattice owns pixels"


def test_scene_properties():
    """The scenes contain what they are there for."""
    by = {s.name: s for s in SCENES}
    # fold: front and back faces both show
    ref = rs.reference(by["tilted_fold"])
    vs = rr.vertex_stage(ref["frame"].vp, 96, 64, by["tilted_fold"].pos[:, :3])
    ids = (ref["keys"] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    seen = np.unique(ids[ids > 0]) - 1
    f = ref["faces"][seen]
    area = (vs["X"][f[:, 1]] - vs["X"][f[:, 0]]) * (vs["Y"][f[:, 2]] - vs["Y"][f[:, 0]]) - \
        (vs["Y"][f[:, 1]] - vs["Y"][f[:, 0]]) * (vs["X"][f[:, 2]] - vs["X"][f[:, 0]])
    assert (area > 0).sum() > 20 and (area < 0).sum() > 20
    # borders: cleared pixels (alpha 0, depth = zfar), triangles dropped for the vertex behind the camera, some wholly outside
    sc = by["borders_and_planes"]
    ref = rs.reference(sc)
    cleared = ref["keys"] == rr.CLEARED_KEY
    assert 200 < cleared.sum() < sc.W * sc.H - 2000
    far = rr.linear_depth(np.zeros(1, np.int64), np.ones(1, bool))[0]  # the formula at window depth 1: zfar up to float32 rounding
    assert abs(float(far) - 3.0) < 1e-5
    assert (ref["rgba"][..., 3][cleared] == 0).all() and (ref["depth"][cleared] == far).all()
    assert (ref["keys"] & np.uint64(0xFFFFFFFF) != 0).all(), "the ground is beyond the far plane"
    vs = rr.vertex_stage(ref["frame"].vp, sc.W, sc.H, sc.pos[:, :3])
    assert (~vs["ok"]).sum() == 1
    ids = (ref["keys"][~cleared] & np.uint64(0xFFFFFFFF)).astype(np.int64) - 1
    dropped = np.nonzero((ref["faces"] == 2 * 12 + 2).any(1))[0]
    assert len(dropped) == 6 and not np.isin(dropped, ids).any()
    assert ((vs["d"] > 1.0) & vs["ok"]).sum() > 10  # vertices beyond the far plane
    f = ref["faces"]
    outside = (vs["X"][f].max(1) < 0) | (vs["X"][f].min(1) > sc.W * 256) | (vs["Y"][f].max(1) < 0) | (vs["Y"][f].min(1) > sc.H * 256)
    assert outside.sum() > 20
    okv = vs["ok"]
    assert vs["X"][okv].min() < 0 and vs["X"][okv].max() > sc.W * 256 and vs["Y"][okv].min() < 0 and vs["Y"][okv].max() > sc.H * 256
    for border in (ref["keys"][0], ref["keys"][-1], ref["keys"][:, -1]):
        assert (border != rr.CLEARED_KEY).any(), "the mesh is drawn up to the border"
    assert (ref["keys"][:, 0] == rr.CLEARED_KEY).all(), "the left border (z > 1.2) lies beyond the far plane"
    # ties: rows 0-4 and their copies; the copy (higher ids) never wins, the sliver and the zero-area strips own nothing
    sc = by["ties_and_degenerates"]
    ref = rs.reference(sc)
    ids = (ref["keys"] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert (ids > 0).sum() > 200
    vs = rr.vertex_stage(ref["frame"].vp, sc.W, sc.H, sc.pos[:, :3])
    first, _ = rr.raster_exact(vs, ref["faces"][:72], sc.W, sc.H, first_id=1)
    copy, _ = rr.raster_exact(vs, ref["faces"][90:162], sc.W, sc.H, first_id=91)
    assert np.array_equal(first != rr.CLEARED_KEY, ids > 0) and np.array_equal(copy != rr.CLEARED_KEY, ids > 0)
    tie = ((first >> np.uint64(32)) == (copy >> np.uint64(32))) & (ids > 0)
    assert tie.sum() > 0.5 * (ids > 0).sum(), tie.mean()  # same surface, other diagonal: most depths tie to the bit ...
    assert (ids[tie] <= 72).all()                         # ... and there the layer drawn first keeps the pixel
    assert (ids[(ids > 0) & ~tie] > 0).all() and ((ids > 72) & (ids <= 90)).sum() == 0  # the strip of zero area owns nothing,
    assert (ids > 162).sum() == 0                                                      # nor do the sliver and the strip behind it
    assert np.abs(vs["X"][100:110] - vs["X"][0:10]).max() < 256 * 0.1 and (vs["X"][100:110] != vs["X"][0:10]).all()  # a real sliver
    # sphere tie: the eight cloth triangles (ids 801 ..) coincide with sphere triangles and never win; alone they cover pixels
    sc = by["sphere_tie"]
    ref = rs.reference(sc)
    ids = (ref["keys"] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert (ids > 800).sum() == 0
    vs = rr.vertex_stage(ref["frame"].vp, sc.W, sc.H, sc.pos[:, :3])
    alone, _ = rr.raster_exact(vs, ref["faces"], sc.W, sc.H, first_id=801)
    hit = alone != rr.CLEARED_KEY
    assert hit.sum() > 20 and np.array_equal(alone[hit] >> np.uint64(32), ref["keys"][hit] >> np.uint64(32))
    # tent: perspective matters (w differs 2 : 1 inside a triangle) and no pixel takes a PCF sample
    ref = rs.reference(by["tent"])
    vs = rr.vertex_stage(ref["frame"].vp, 96, 64, by["tent"].pos[:, :3])
    assert vs["w"].max() / vs["w"].min() > 2.0 and np.isinf(ref["pcf_gap"]).all()
    assert ((ref["keys"] & np.uint64(0xFFFFFFFF)) > 0).sum() > 500
    # ground plane: which of cloth and ground wins where both lie in y = 0 -- recorded, see PARITY.md
    ref = rs.reference(by["ground_coplanar"])
    ids = (ref["keys"] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    inside = ref["zkeys"] != rr.CLEARED_KEY
    assert inside.sum() > 300
    gq = (rr.ground_keys(ref["frame"])[0] >> np.uint64(32)).astype(np.int64)[inside]
    cq = (ref["zkeys"] >> np.uint64(32)).astype(np.int64)[inside]
    print("ground_coplanar: cloth wins", (ids[inside] > 0).sum(), "of", inside.sum(), "pixels; ground depth24 - cloth depth24:",
          (gq - cq).min(), "..", (gq - cq).max())
    assert (ids[inside] > 0).all() and (gq - cq).min() >= 1  # recorded: the cloth's own depth is a step or more nearer everywhere
    # pickers: three spheres show, back faces are culled in the camera pass and drawn in the shadow pass
    sc = by["pickers"]
    ref = rs.reference(sc)
    ids = (ref["keys"] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    for q in range(3):
        assert ((ids > 800 * q) & (ids <= 800 * (q + 1))).sum() > 10, q
    sv, _, st = ref["mesh"]
    vs = rr.vertex_stage(ref["frame"].vp, sc.W, sc.H, sv[:, :3])
    unculled, _ = rr.raster_exact(vs, st[:2400], sc.W, sc.H)
    culled, _ = rr.raster_exact(vs, st[:2400], sc.W, sc.H, cull_back=np.ones(2400, bool))
    assert np.array_equal(unculled, culled)  # closed meshes seen from outside: culling cannot change the nearest surface ...
    assert (ids > 2400).sum() == (ids > 3200).sum()  # ... but the sphere around the camera shows only its inside: culled away
    inside_out, _ = rr.raster_exact(vs, st[2400:], sc.W, sc.H, first_id=2401)
    assert (inside_out != rr.CLEARED_KEY).all(), "without culling it would fill the frame"
    vl = rr.vertex_stage(ref["frame"].light, 2048, 2048, sv[:, :3])
    assert not np.array_equal(rr.raster_exact(vl, st, 2048, 2048, shadow=True)[0],
                              rr.raster_exact(vl, st, 2048, 2048, shadow=True, cull_back=np.ones(len(st), bool))[0])


@pytest.mark.parametrize("name", ["tilted_fold", "coincident", "grid17x16"])
def test_oracle_normals_within_float32_bound(name):
    """OracleSim.get_normals (the float32 formula the kernel shares) against float64 on the three inputs of the GPU test."""
    from oracle import OracleSim
    from scenarios import cloth_params

    dimx, dimz, pos = rs.normals_input(name)
    orc = OracleSim()
    orc.set_scene(cloth_params(dimx, dimz, pos=rs.SCENE_POS))
    p = pos.copy()
    p[:, 3] = orc.get_positions().reshape(-1, 4)[:, 3]
    orc.set_positions(p.ravel())
    rs.check_normals(np.array(orc.get_normals()).reshape(-1, 4), p, np.array(orc.get_faces()).reshape(-1, 3))
