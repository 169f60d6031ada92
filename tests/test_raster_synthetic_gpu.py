"""The HIP rasteriser against the exact-arithmetic reference (tests/raster_reference.py) on the synthetic scenes of
tests/raster_scenes.py: z-buffer keys (depth24 and primitive id) and the shadow map through the white-box read-back
FlingSim.render_buffers, the depth plane, alpha and colour through render().  tests/test_raster_reference_cpu.py holds the
CPU half (reference == oracle/raster_oracle.c on the same scenes)."""
import numpy as np
import pytest

import raster_reference as rr
import raster_scenes as rs

pytestmark = pytest.mark.gpu
SCENES = rs.all_scenes()
_ctx, _device = [], {}


def _env():
    from flingbot_amd import sim as fsim

    if not _ctx:
        _ctx.append(fsim.FlingSim(n_envs=1))
    return _ctx[0].env(0)


def device(sc):
    """What the device makes of the scene, rendered once per scene: render(), render_buffers() twice, render() again."""
    if sc not in _device:
        env = _env()
        rs.install(env, sc)
        before = env.render()
        first = env.render_buffers()
        second = env.render_buffers()
        after = env.render()
        _device[sc] = dict(before=before, first=first, second=second, after=after, faces=np.array(env.get_faces()).reshape(-1, 3),
                           bounds=env.get_scene_bounds(), mesh=env.sphere_mesh() if sc.spheres else None)
    return _device[sc]


def check_buffers(sc, ref, dev):
    W, H = sc.W, sc.H
    zkeys, shadow = dev["first"][0].reshape(H, W), dev["first"][1].reshape(2048, 2048)
    # the reference was given the same scene: faces, light bounds, picker meshes
    assert np.array_equal(dev["faces"], ref["faces"])
    assert np.array_equal(dev["bounds"][0], ref["lower"]) and np.array_equal(dev["bounds"][1], ref["upper"])
    if sc.spheres:
        assert all(np.array_equal(a, b) for a, b in zip(dev["mesh"], ref["mesh"]))
    # pixels whose exact depth sits within 1e-6 step of a boundary may be left out: none is on these seeds (CPU test), 0.1 % is the cap
    sure, sure_s = ~(ref["margin"] < rr.MARGIN_LSB), ~(ref["shadow_margin"] < rr.MARGIN_LSB)
    assert (~sure).sum() <= 1e-3 * max(1, (ref["zkeys"] != rr.CLEARED_KEY).sum())
    assert (~sure_s).sum() <= 1e-3 * max(1, (ref["shadow"] != rr.CLEARED_TEXEL).sum())
    bad = (zkeys != ref["zkeys"]) & sure
    assert not bad.any(), f"{bad.sum()} z keys differ; first (row, column) {np.argwhere(bad)[0]}: " \
                          f"{int(zkeys[bad][0]):#x} for {int(ref['zkeys'][bad][0]):#x}"
    bad = (shadow != ref["shadow"]) & sure_s
    assert not bad.any(), f"{bad.sum()} shadow texels differ; first {np.argwhere(bad)[0]}: {shadow[bad][0]} for {ref['shadow'][bad][0]}"
    # the depth plane: the formula on the device's own keys, the ground plane joined in
    rgba, depth = dev["before"][0].reshape(H, W, 4), dev["before"][1].reshape(H, W)
    keys = np.minimum(zkeys, rr.ground_keys(ref["frame"])[0])
    cleared = keys == rr.CLEARED_KEY
    assert np.array_equal(depth.view(np.uint32), rr.linear_depth((keys >> np.uint64(32)).astype(np.int64), cleared).view(np.uint32))
    assert np.array_equal(depth.view(np.uint32)[sure], ref["depth"].view(np.uint32)[sure])
    assert np.array_equal(rgba[..., 3], np.where(cleared, 0, 255))
    # the read-back is repeatable and leaves the renderer as it was
    assert np.array_equal(dev["first"][0], dev["second"][0]) and np.array_equal(dev["first"][1], dev["second"][1])
    assert np.array_equal(dev["before"][0], dev["after"][0]) and np.array_equal(dev["before"][1], dev["after"][1])
    return rgba


@pytest.mark.parametrize("sc", SCENES, ids=repr)
def test_scene_matches_exact_reference(gpu_required, sc):
    """Keys (depth24 and id) at every pixel, the shadow map at all 2048^2 texels, depth plane, alpha; colour within 1 LSB of the
    float64 shading on at most 2 % of the channels -- on the scenes that allow it (raster_scenes: Scene.colour / .why)."""
    ref = rs.reference(sc)
    rgba = check_buffers(sc, ref, device(sc))
    if sc.colour:
        diff = np.abs(rgba[..., :3].astype(int) - ref["rgba"][..., :3].astype(int))
        print(f"{sc}: colour max difference {diff.max()}, share of differing channels {(diff > 0).mean():.5f}; "
              f"nearest PCF compare {ref['pcf_gap'].min():.2f} steps from its threshold ({sc.why})")
        assert diff.max() <= 1, f"max colour difference {diff.max()} on {(diff > 1).sum()} channels"
        assert (diff > 0).mean() < 0.02, (diff > 0).mean()


def test_folded_mesh_at_720(gpu_required):
    """The folded mesh at the product's own frame size: 2025 shading tiles, triangles some 30 pixels wide."""
    sc = rs.fold_720()
    check_buffers(sc, rs.reference(sc, False), device(sc))


@pytest.mark.parametrize("name", ["tilted_fold", "coincident", "grid17x16"])
def test_vertex_normals_within_float32_bound(gpu_required, name):
    """get_normals against float64 within the bound derived in raster_reference.vertex_normals64 (a quarter of the worst
    case; measured maximum 0.20 of it, 1.3e-7 absolute), and exactly (0, 1, 0) where all incident normals cancel."""
    from scenarios import cloth_params

    dimx, dimz, pos = rs.normals_input(name)
    env = _env()
    env.set_scene(cloth_params(dimx, dimz, pos=rs.SCENE_POS))
    p = pos.copy()
    p[:, 3] = env.get_positions().reshape(-1, 4)[:, 3]
    env.set_positions(p.ravel())
    rs.check_normals(np.array(env.get_normals()).reshape(-1, 4), p, np.array(env.get_faces()).reshape(-1, 3))
