"""Domain-randomised appearance, everything that needs no GPU: the draw (flingbot_amd/appearance.py), the palette against
the reference's cloth mask, the argument checks of the C-ABI (include/flingsim.h fs_appearance) and the texture rule --
restated in tests/appearance_reference.py and compiled for the host in the library (fs_host_ground_texture)."""
import colorsys
import ctypes as C
import os
import re

import numpy as np
import pytest

import appearance_reference as ar
import raster_reference as rr
import raster_scenes as rs
from flingbot_amd import appearance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the draw -----------------------------------------------------------------------------------------------------------
def test_draw_is_a_pure_function_of_its_key_with_the_reference_colour_draw():
    key = (3, 5, 2)
    a, b = appearance.draw(key), appearance.draw(list(key))
    assert appearance.equal(a, b) and a["ground_seed"] == b["ground_seed"]
    rng = np.random.default_rng([*key, appearance.TAG])
    h, s, v = rng.uniform(0.0, 1.0), rng.uniform(0.0, 1.0), rng.uniform(0.5, 1.0)   # hsv = (U(0,1), U(0,1), U(0.5,1)), in that order
    assert np.array_equal(a["cloth_rgb"], np.array(colorsys.hsv_to_rgb(h, s, v), np.float32))
    assert a["cloth_rgb"].dtype == np.float32 and a["ground_rgb"].shape == (2, 3) and a["ground_octaves"] == 4
    assert 2.0 <= a["ground_cells_per_m"] <= 16.0 and 0 <= a["ground_seed"] < 1 << 24
    appearance.check(a)
    row = appearance.as_row(a)
    assert row.dtype == np.float32 and row.shape == (appearance.ROW,) and int(row[9]) == a["ground_seed"]
    # 64 different keys: 64 different appearances
    rows = {appearance.as_row(appearance.draw((3, t, k))).tobytes() for t in range(8) for k in range(8)}
    assert len(rows) == 64
    # the key words all count, and the modes key as documented
    assert not appearance.equal(appearance.draw((3, 5, 2)), appearance.draw((4, 5, 2)))
    assert appearance.key_of("observation", 3, 5, 2) == (3, 5, 2) and appearance.key_of("episode", 3, 5, 2) == (3, 5, 0)
    with pytest.raises(ValueError):
        appearance.key_of("frame", 3, 5, 2)


def test_draw_is_independent_of_the_exploration_stream():
    """nets.MaximumValuePolicy._explore draws from default_rng((seed, task, step)): the appearance's uniforms on the same
    triple come from another stream (the key's fourth word), so none of its first draws reappears."""
    for key in ((0, 0, 0), (3, 1, 2), (7, 95, 9)):
        explore = np.random.default_rng([int(k) for k in key]).random(16)
        mine = np.random.default_rng([*key, appearance.TAG]).random(16)
        assert not np.isin(mine, explore).any()
        h = np.random.default_rng([*key, appearance.TAG]).uniform(0.0, 1.0)
        assert abs(colorsys.rgb_to_hsv(*appearance.draw(key)["cloth_rgb"].astype(np.float64))[0] - h) < 1e-5
        assert np.abs(explore - h).min() > 0


# ---- 2. the ground stays background ----------------------------------------------------------------------------------------
def test_every_drawn_ground_is_background_for_the_reference_mask():
    """256 keys x (both albedos + 16 mixes) shaded by raster_reference.shade under the default camera -- fully lit, at the shadow
    floor (0.5) and at the spot floor (0.05) -- are background for oracle.observe.cloth_mask_raw (8-bit H, S, V all <= 100):
    the condition the draw's ranges exist for."""
    from oracle.observe import cloth_mask_raw

    sc = rs.tilted_fold()
    fr = rs.reference(sc, False)["frame"]          # top-down camera at (0, 2, 0), the light of the scene's bounds
    lit = np.full((rr.SHADOW_RES, rr.SHADOW_RES), rr.CLEARED_TEXEL, np.uint32)
    dark = np.zeros((rr.SHADOW_RES, rr.SHADOW_RES), np.uint32)
    albedos = []
    for k in range(256):
        g = appearance.draw((11, k // 16, k % 16))["ground_rgb"].astype(np.float64)
        albedos += [g[0] + (g[1] - g[0]) * t for t in np.linspace(0.0, 1.0, 18)]   # both ends and 16 mixes between them
    col = np.array(albedos)
    n = len(col)
    up, zero = np.tile([0.0, 1.0, 0.0], (n, 1)), np.zeros(n)
    L = fr.light.astype(np.float64)
    ndc_r2 = lambda z: sum((L[r, 2] * z + L[r, 3]) ** 2 for r in (0, 1)) / (L[3, 2] * z + L[3, 3]) ** 2   # noqa: E731
    z_out = next(z for z in np.arange(1.0, 200.0, 1.0) if ndc_r2(z) >= 1.0)   # the first metre mark outside the light's cone
    centre, far = np.tile([0.0, 0.0, 0.0], (n, 1)), np.tile([0.0, 0.0, z_out], (n, 1))
    probe = lambda shadow, p: rr.shade(fr, shadow, p[:1], up[:1], np.ones((1, 3)), zero[:1])[0][0]   # noqa: E731
    # the three conditions are what they claim to be: white shades 2:1 between lit and shadowed (plus the ambient term), and
    # the far point sits at the spot's floor
    w_lit, w_dark, w_far = (probe(lit, centre) ** 2.2, probe(dark, centre) ** 2.2, probe(lit, far) ** 2.2)
    assert 0.5 < w_dark[1] / w_lit[1] < 0.62 and 0.035 < w_far[1] / w_lit[1] < 0.05    # (0.05, and some more fog on the way)
    assert abs(w_lit.max() - 1.021) < 0.01         # "a fully lit ground of albedo c shades to (1.021 c)^(1 / 2.2)"
    for name, shadow, p in (("lit", lit, centre), ("shadow floor", dark, centre), ("spot floor", lit, far)):
        rgb = rr.shade(fr, shadow, p, up, col, zero)[0]
        u8 = np.floor(np.clip(rgb, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
        mask = cloth_mask_raw(u8.reshape(1, n, 3))
        assert not mask.any(), f"{name}: {int(mask.sum())} of {n} ground colours read as cloth, first {u8[np.nonzero(mask.ravel())[0][0]]}"


# ---- 3. setter, default, layout --------------------------------------------------------------------------------------------
def test_default_equals_the_literals_of_the_camera_header():
    from flingbot_amd import sim as fsim

    text = open(os.path.join(ROOT, "flingbot_amd", "csrc", "fs_camera.h")).read()
    cloth = [np.float32(a) * np.float32(b) for a, b in re.findall(r"fr\.col_cloth\[\d\] = ([0-9.]+)f \* ([0-9.]+)f;", text)]
    plane = np.float32(re.search(r"fr\.col_plane\[k\] = ([0-9.]+)f;", text).group(1))
    assert len(cloth) == 3
    d = appearance.default()
    assert np.array_equal(d["cloth_rgb"], np.array(cloth, np.float32)) and np.array_equal(d["ground_rgb"], np.full((2, 3), plane))
    assert d["ground_octaves"] == 0
    lib = fsim.load_library()
    out = fsim.Appearance()
    assert lib.fs_appearance_default(C.byref(out)) == C.sizeof(fsim.Appearance) == 48     # sizeof(fs_appearance)
    assert lib.fs_appearance_default(None) == 48
    assert appearance.equal(appearance.from_struct(out), d)
    assert np.array_equal(appearance.as_row(appearance.from_struct(appearance.to_struct(d))), appearance.as_row(d))


def test_header_declares_and_library_exports_the_entry_points():
    from flingbot_amd import sim as fsim

    header = open(os.path.join(ROOT, "include", "flingsim.h")).read()
    assert "typedef struct fs_appearance {" in header
    assert re.search(r"^int fs_set_appearance\(fs_ctx \*ctx, int n, const int \*envs, const fs_appearance \*table\);", header, re.M)
    assert re.search(r"^int fs_get_appearance\(fs_ctx \*ctx, int env, fs_appearance \*out\);", header, re.M)
    lib = fsim.load_library()
    for name in ("fs_set_appearance", "fs_get_appearance", "fs_appearance_default", "fs_appearance_check", "fs_host_ground_texture"):
        assert hasattr(lib, name) and name in lib._fs_symbols
    # host-side refusals need no device
    ok = appearance.to_struct(appearance.draw((1, 2, 3)))
    env0 = (C.c_int * 1)(0)
    assert lib.fs_set_appearance(None, 1, env0, C.byref(ok)) == -1 and b"fs_set_appearance" in lib.fs_last_error()
    assert lib.fs_get_appearance(None, 0, C.byref(ok)) == -1


def _bad_appearances():
    good = appearance.draw((1, 2, 3))
    def mod(**kw):   # noqa: E306
        a = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        for k, v in kw.items():
            if isinstance(v, tuple):
                a[k][v[0]] = v[1]
            else:
                a[k] = v
        return a
    return good, {
        "negative cloth": mod(cloth_rgb=(1, -0.01)), "nan cloth": mod(cloth_rgb=(0, np.nan)), "inf cloth": mod(cloth_rgb=(2, np.inf)),
        "negative ground": mod(ground_rgb=((0, 2), -1e-6)), "nan ground": mod(ground_rgb=((1, 0), np.nan)),
        "inf ground": mod(ground_rgb=((1, 1), -np.inf)),
        "octaves -1": mod(ground_octaves=-1), "octaves 7": mod(ground_octaves=7),
        "finest octave 257": mod(ground_cells_per_m=257.0, ground_octaves=1),
        "finest octave 32.01 * 8": mod(ground_cells_per_m=32.01, ground_octaves=4),
        "finest octave 8.1 * 32": mod(ground_cells_per_m=8.1, ground_octaves=6),
        "cells 0": mod(ground_cells_per_m=0.0), "cells negative": mod(ground_cells_per_m=-2.0),
        "cells nan": mod(ground_cells_per_m=float("nan")), "cells inf": mod(ground_cells_per_m=float("inf")),
    }


def test_check_refuses_every_bad_argument():
    good, bad = _bad_appearances()
    appearance.check(good)
    appearance.check(appearance.default())
    for edge in (dict(ground_cells_per_m=256.0, ground_octaves=1), dict(ground_cells_per_m=8.0, ground_octaves=6),
                 dict(ground_cells_per_m=0.0, ground_octaves=0), dict(ground_cells_per_m=-1.0, ground_octaves=0)):
        appearance.check({**good, **edge})     # the bounds themselves pass; cells_per_m is not read with 0 octaves
    for name, a in bad.items():
        with pytest.raises(ValueError, match="fs_appearance"):
            appearance.check(a)
            pytest.fail(name)


# ---- 4. the texture rule ---------------------------------------------------------------------------------------------------
def test_texture_rule_in_the_reference():
    rng = np.random.default_rng(5)
    hx, hz = rng.uniform(-3.0, 3.0, 20000), rng.uniform(-3.0, 3.0, 20000)
    for seed, cells, octaves in ((1, 2.0, 1), (7, 16.0, 4), (123456789, 8.0, 6), (0xFFFFFFFF, 3.3, 3)):
        t = ar.noise(hx, hz, seed, cells, octaves)
        assert t.min() >= 0.0 and t.max() <= 1.0
        assert t.std() > 0.1 and 0.3 < t.mean() < 0.7                       # it is a texture, not a constant
    # continuous across 1000 lattice lines of every octave (p on the line of octave 0 is on a line of the finer ones too)
    lines = np.arange(-500, 500) / 16.0
    other = rng.uniform(-3.0, 3.0, 1000)
    for a, b in ((lines, other), (other, lines)):
        assert np.abs(ar.noise(a, b, 7, 16.0, 4) - ar.noise(a + 1e-6, b + 1e-6, 7, 16.0, 4)).max() < 1e-4
        assert np.abs(ar.noise(a, b, 7, 16.0, 4) - ar.noise(a - 1e-6, b - 1e-6, 7, 16.0, 4)).max() < 1e-4
    # one octave at integer lattice points: the hash value itself
    i, j = np.meshgrid(np.arange(-40, 40), np.arange(-40, 40))
    got = ar.noise(i / 2.0, j / 2.0, 99, 2.0, 1)
    assert np.array_equal(got, (ar.hash32(i, j, 0, 99) >> 8) * 2.0 ** -24)
    assert len(np.unique(got)) > 6300                                        # 6400 lattice points, (almost) no collisions
    # the hash, worked by hand for one point: h = 1 * 0x9E3779B1 + 2 * 0x85EBCA77 + 3 * 0xC2B2AE3D + 4
    h = (0x9E3779B1 + 2 * 0x85EBCA77 + 3 * 0xC2B2AE3D + 4) & 0xFFFFFFFF
    h ^= h >> 16; h = (h * 0x7FEB352D) & 0xFFFFFFFF; h ^= h >> 15; h = (h * 0x846CA68B) & 0xFFFFFFFF; h ^= h >> 16   # noqa: E702
    assert int(ar.hash32(1, 2, 3, 4)) == h
    assert int(ar.hash32(-1, -2, 0, 0)) == int(ar.hash32(0xFFFFFFFF, 0xFFFFFFFE, 0, 0))   # two's complement


def test_library_texture_function_matches_the_reference():
    """fs_host_ground_texture -- the function the shading kernels inline, compiled for the host -- against the float64 rule.
    Bound: u = hx f is rounded once (2^-24 |u|), a = u - floor(u) inherits it, n_o moves by at most 1.5 per unit of a and
    of b (s' <= 1.5, lattice values differ by < 1): 3 * 2^-24 max|u| per octave, the octaves' weights sum to 1; 32 ulp of 1
    for the mixes, the sum and the division."""
    rng = np.random.default_rng(9)
    hx, hz = rng.uniform(-2.0, 2.0, 50000).astype(np.float32), rng.uniform(-2.0, 2.0, 50000).astype(np.float32)
    for seed, cells, octaves in ((1, 2.0, 1), (7, 16.0, 4), (123456789, 8.0, 6), (0xFFFFFFFF, 3.3, 3)):
        ap = dict(appearance.default(), ground_seed=seed, ground_cells_per_m=cells, ground_octaves=octaves)
        got = appearance.host_ground_texture(ap, hx, hz)
        want = ar.noise(hx.astype(np.float64), hz.astype(np.float64), seed, np.float32(cells), octaves)
        bound = 3 * 2.0 ** -24 * 2.0 * float(np.float32(cells)) * 2 ** (octaves - 1) + 32 * 2.0 ** -24
        print(f"seed {seed} cells {cells} octaves {octaves}: max |dt| {np.abs(got - want).max():.3e}, bound {bound:.3e}")
        assert np.abs(got - want).max() <= bound
    # negative cells and far points: floor, not truncation; the clamp keeps a far hit defined
    ap = dict(appearance.default(), ground_seed=5, ground_cells_per_m=4.0, ground_octaves=2)
    far = appearance.host_ground_texture(ap, [-0.3, 1e30, -1e30], [-0.3, 0.0, 1e30])
    assert np.isfinite(far).all() and abs(far[0] - ar.noise(np.float64(np.float32(-0.3)), np.float64(np.float32(-0.3)), 5, 4.0, 2)) < 1e-5
    assert np.array_equal(appearance.host_ground_texture(appearance.default(), [0.1], [0.2]), np.zeros(1, np.float32))


def test_reference_render_with_the_default_appearance_is_the_raster_reference():
    """appearance_reference.render(scene, default()) reproduces raster_reference.render's colours exactly: the helper adds the
    appearance and nothing else."""
    sc = rs.tilted_fold()
    mine, theirs = ar.render(sc, appearance.default()), rs.reference(sc)
    assert np.array_equal(mine["rgba"], theirs["rgba"]) and mine["ground"].any()


# ---- command line ----------------------------------------------------------------------------------------------------------
def test_command_lines_take_the_flag():
    from flingbot_amd import evaluate, train

    a = evaluate.build_parser().parse_args(["--tasks", "set.npz", "--randomize-appearance", "observation", "--seed", "3"])
    assert a.randomize_appearance == "observation" and evaluate.appearance_env_kwargs(a) == dict(randomize_appearance="observation")
    a = evaluate.build_parser().parse_args(["--tasks", "set.npz"])
    assert a.randomize_appearance is None and evaluate.appearance_env_kwargs(a) == {}      # off: nothing is passed on
    a = train.build_parser().parse_args(["--log", "d", "--tasks", "set.npz", "--randomize-appearance", "episode"])
    assert a.randomize_appearance == "episode"
    with pytest.raises(SystemExit):
        evaluate.build_parser().parse_args(["--tasks", "set.npz", "--randomize-appearance", "frame"])


def test_replay_file_carries_the_rows_only_when_randomised(tmp_path):
    from flingbot_amd import taskio

    task = dict(cloth_mass=0.5, flatten_area=1.0, task_difficulty="easy", initial_coverage=0.4)
    rec = dict(coverage=[0.4, 0.5, 0.6], actions=["fling", None], rewards=[0.1, 0.1], preaction_coverage=[0.4, 0.5])
    rows = [appearance.as_row(appearance.draw((3, 0, k))) for k in range(2)]
    taskio.save_replay(str(tmp_path / "off.npz"), [rec], [task])
    taskio.save_replay(str(tmp_path / "on.npz"), [dict(rec, appearance=rows)], [task])
    off, on = np.load(tmp_path / "off.npz"), np.load(tmp_path / "on.npz")
    extra = sorted(set(on.files) - set(off.files))
    assert extra == ["000000000_step00/appearance", "000000000_step01_last/appearance"] and set(off.files) <= set(on.files)
    assert np.array_equal(on[extra[1]], rows[1]) and on[extra[0]].dtype == np.float32
    assert all(np.array_equal(off[f], on[f]) for f in off.files)


def test_drop_in_module_has_the_additive_names():
    from test_pyflex_module import REFERENCE_NAMES, _import_pyflex

    pyflex = _import_pyflex()
    for name in ("set_appearance", "get_appearance"):
        assert callable(getattr(pyflex, name, None)) and name not in REFERENCE_NAMES     # additive: shadows none of the 40
    with pytest.raises((RuntimeError, TypeError)):
        pyflex.set_appearance(list(range(11)))                                           # 12 numbers, checked before the library
