"""Fixtures recorded OUTSIDE this repository -- real PyFleX trajectories and real cv2 / skimage outputs -- and the path that
ingests them.

The two pins this repository cannot close itself are the solver arithmetic (closed-source NVIDIA FleX: needs an NVIDIA GPU)
and the cv2 / skimage calls of the observation stage (neither package is in the build image).  tests/golden/capture_pyflex.py
and tests/golden/capture_cv2.py are standalone kits that record them on a machine that has those libraries; this module
consumes the resulting files when they are present (tests/golden/external/*.npz, or FLINGBOT_PYFLEX_FIXTURE /
FLINGBOT_CV2_FIXTURE) and skips cleanly when they are not.  So that the ingest path itself is tested here and now, every
check first runs on a fixture of the same format written by the repository's own restatements (the capture functions take
the backend as an argument): there the divergence must be exactly zero, and a deliberately different backend must be
caught.

What a PyFleX fixture is compared with: the same scenario (tests/scenarios.py, the fixture stores its arguments) replayed
(a) free-running and (b) re-synchronised -- after every recorded frame the replay's particle state is overwritten with the
fixture's, so the next recorded frame measures the error of the steps in between alone (one step when the fixture keeps
every frame).  PARITY.md explains why (b) is the number north_star's 1e-4 can be held against: a crumpling cloth is chaotic,
even last-bit arithmetic differences reach 1e-1 within a few hundred frames when free-running.
"""
import importlib.util
import json
import os

import numpy as np
import pytest

import scenarios as sc

HERE = os.path.dirname(os.path.abspath(__file__))
EXT = os.path.join(HERE, "golden", "external")
PYFLEX_FIXTURE = os.environ.get("FLINGBOT_PYFLEX_FIXTURE", os.path.join(EXT, "pyflex_fixture.npz"))
CV2_FIXTURE = os.environ.get("FLINGBOT_CV2_FIXTURE", os.path.join(EXT, "cv2_fixture.npz"))
REL_TOL = 1e-4  # north_star: positions within 1e-4 relative fp32


def _kit(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Follower:
    """record= callback of a replay: at every frame the fixture holds, the divergence of the replay from it (relative to the
    scene extent, at least 1 m) and whether the two are bit-identical; with resync, the replay's particle state is then
    overwritten with the fixture's."""

    def __init__(self, frames, pos, vel, resync):
        self.at = {int(f): i for i, f in enumerate(frames)}
        self.pos, self.vel, self.resync, self.count = pos, vel, resync, 0
        self.frames, self.div, self.exact = [], [], []

    def __call__(self, sim):
        self.count += 1
        i = self.at.get(self.count)
        if i is None:
            return
        mine, ref = np.asarray(sim.get_positions(), np.float32), self.pos[i]
        a, b = mine.reshape(-1, 4)[:, :3], ref.reshape(-1, 4)[:, :3]
        self.frames.append(self.count)
        self.div.append(float(np.abs(a - b).max() / max(1.0, float(np.abs(b).max()))))
        self.exact.append(bool(np.array_equal(mine.view(np.uint32), ref.view(np.uint32))))
        if self.resync:
            sim.set_positions(ref)
            sim.set_velocities(self.vel[i])


def replay_pyflex_fixture(path, make_sim):
    """{scenario: {"frames", "free", "resync", "exact", "every"}} for every scenario in the fixture."""
    z = np.load(path)
    meta = json.loads(str(z["meta"]))
    assert meta["format"] == "flingbot_amd pyflex fixture v1", meta
    out = {}
    for name in meta["scenarios"]:
        args = json.loads(str(z[name + "/args"]))
        frames, pos, vel = z[name + "/frames"], z[name + "/positions"], z[name + "/velocities"]
        runs = {}
        for mode in ("free", "resync"):
            fol = _Follower(frames, pos, vel, resync=(mode == "resync"))
            sc.CANONICAL[name](make_sim(), record=fol, **args)
            assert fol.frames == [int(f) for f in frames], (name, "the replay took a different number of steps than the fixture")
            runs[mode] = fol
        out[name] = {"frames": runs["free"].frames, "free": runs["free"].div, "resync": runs["resync"].div,
                     "exact": all(runs["free"].exact), "every": meta["every"], "backend": meta["backend"]}
    return out


def _report(res, who):
    lines = []
    for name, r in res.items():
        pick = sorted(set([0, len(r["frames"]) // 4, len(r["frames"]) // 2, len(r["frames"]) - 1]))
        lines.append(f"  {who} vs {r['backend']} fixture, {name}: " + ", ".join(
            f"frame {r['frames'][i]}: free {r['free'][i]:.1e} / resync {r['resync'][i]:.1e}" for i in pick) +
            f"; worst resync {max(r['resync']):.1e}" + ("  [bit-identical]" if r["exact"] else ""))
    return "\n".join(lines)


@pytest.fixture(scope="module")
def self_made_fixture(tmp_path_factory):
    """A fixture of the real format, written by the capture kit with the CPU oracle in PyFleX's place (16 x 16, short)."""
    from oracle import OracleSim

    path = str(tmp_path_factory.mktemp("fixture") / "oracle_fixture.npz")
    _kit("capture_pyflex").capture(OracleSim, path, names=("c1", "c2", "fling"), every=1, dim=16, quick=True, backend="oracle")
    return path


def test_pyflex_fixture_ingest_path_on_a_self_made_fixture(self_made_fixture, capsys):
    """Capture kit -> file -> replay: the oracle replays its own recording bit for bit in both modes, and an oracle with ONE
    model choice changed (oracle/flex_oracle.c MODEL switches) is caught by both."""
    from oracle import OracleSim

    z = np.load(self_made_fixture)
    for name in ("c1", "c2", "fling"):
        for key in ("frames", "positions", "velocities", "shape_states", "params", "args"):
            assert f"{name}/{key}" in z.files
        assert z[name + "/positions"].dtype == np.float32 and z[name + "/positions"].shape[0] == z[name + "/frames"].size
    assert z["fling/shape_states"].shape[1] == 28          # two pickers x 14 floats (pyflex.cpp:789-822)
    same = replay_pyflex_fixture(self_made_fixture, OracleSim)
    for name, r in same.items():
        assert r["exact"] and max(r["free"]) == 0.0 and max(r["resync"]) == 0.0, name
    other = replay_pyflex_fixture(self_made_fixture, lambda: OracleSim("alt_damping_mult"))
    for name, r in other.items():
        assert not r["exact"] and max(r["free"]) > 0.0 and max(r["resync"]) > 0.0, name
        # one step of the damping alternative moves a particle by ~1.5e-6; a particle whose speed sits on sleepThreshold
        # flips between "kept" and "moved" (<= 0.02 m/s x 10 ms), which is where the few 1e-5 entries come from
        assert np.median(r["resync"]) <= 3e-6 and max(r["resync"]) <= 2.5e-4, name
    with capsys.disabled():
        print("\n" + _report(other, "oracle[alt_damping_mult]"))


def test_a_fixture_identifies_the_reading_that_made_it(tmp_path):
    """tests/parity_table.py --fixture: the tool that tells, the day a PyFleX fixture exists, WHICH reading of the closed solver it
    agrees with.  Proved on fixtures whose answer is known: one recorded from the default oracle ranks the default first with
    zero error, one recorded from an oracle with two model choices changed (friction after the solve + applyDeltas per
    constraint type) ranks exactly that pair first with zero error, above either single change, and so does one recorded with
    two readings of the finalize clamp changed (clamp per frame + position following the clamped velocity)."""
    import parity_table as pt
    from oracle import OracleSim

    kit = _kit("capture_pyflex")
    model = ("alt_friction_post", "alt_apply_per_type", "alt_stiffness_iter", "alt_damping_mult", "alt_shape_end_pose",
             "alt_neighbors_by_distance")
    # the finalize clamp's readings (NvFlex.h:112-113; PARITY.md): period per frame + position following the clamped velocity
    clamp = ("alt_maxaccel_per_frame", "alt_maxaccel_position", "alt_no_maxaccel", "alt_friction_post", "alt_damping_mult")
    for maker, only in ((None, model), ("alt_friction_post+apply_per_type", model), ("alt_maxaccel_per_frame+maxaccel_position", clamp)):
        expect = maker
        path = str(tmp_path / f"fix_{expect}.npz")
        kit.capture(lambda: OracleSim(maker), path, names=("fling",), every=1, dim=12, quick=True, backend="oracle")
        ranked = pt.fit_fixture(path, jobs=8, pairs=True, only=only)
        best, per = ranked[0]
        assert best == expect and max(mx for _, mx, _ in per.values()) == 0.0, (best, per)
        worst = {v: max(mx for _, mx, _ in p.values()) for v, p in ranked}
        # every reading that really differs from the maker is off; the list-truncation alternative is a no-op here and ties
        for v in only:
            if v != "alt_neighbors_by_distance":
                assert worst[v] > 0.0, v
        assert worst[None] == (0.0 if expect is None else worst[None]) and (expect is None or worst[None] > 0.0)
        if "alt_neighbors_by_distance" in only:
            assert worst["alt_neighbors_by_distance"] == worst[None]
        if only is clamp:   # (the search never builds "no clamp" together with a rule about the clamp)
            assert not any(v and "no_maxaccel" in v and ("maxaccel_per_frame" in v or "maxaccel_position" in v) for v in worst)


@pytest.mark.gpu
def test_hip_path_replays_the_self_made_fixture_bit_for_bit(gpu_required, self_made_fixture):
    from flingbot_amd import sim as fsim

    ctxs = []

    def make():
        ctxs.append(fsim.FlingSim(n_envs=1))
        return ctxs[-1].env(0)

    res = replay_pyflex_fixture(self_made_fixture, make)
    for name, r in res.items():
        assert r["exact"] and max(r["free"]) == 0.0 and max(r["resync"]) == 0.0, name
    for c in ctxs:
        c.close()


def _check_external(res, who, capsys):
    with capsys.disabled():
        print("\n" + _report(res, who))
    for name, r in res.items():
        # the bar north_star states, on the steps between two recorded frames from PyFleX's own state
        assert max(r["resync"]) <= REL_TOL, (name, f"{who}: {max(r['resync']):.2e} relative after {r['every']} step(s) from "
                                                   f"PyFleX's state (PARITY.md lists which model choice to suspect)")


@pytest.mark.skipif(not os.path.exists(PYFLEX_FIXTURE), reason="no PyFleX fixture (tests/golden/capture_pyflex.py records one "
                                                               "on a machine with the reference's pyflex)")
def test_oracle_against_pyflex_fixture(capsys):
    from oracle import OracleSim

    _check_external(replay_pyflex_fixture(PYFLEX_FIXTURE, OracleSim), "oracle", capsys)


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(PYFLEX_FIXTURE), reason="no PyFleX fixture")
def test_hip_against_pyflex_fixture(gpu_required, capsys):
    from flingbot_amd import sim as fsim

    _check_external(replay_pyflex_fixture(PYFLEX_FIXTURE, lambda: fsim.FlingSim(n_envs=1).env(0)), "HIP", capsys)


# ---------------------------------------------------------------- cv2 / skimage
class _RestatementBackend:
    """capture_cv2's backend made of this repository's restatements: oracle/observe.py (resize, HSV, labelling) and the
    product's host crop / pad / nearest resize (flingbot_amd/nets.py)."""

    versions = {"cv2": "restated (oracle/observe.py)", "skimage": "restated (scipy.ndimage.label)"}

    def resize(self, img, dim):
        from oracle import observe as oo
        return oo.resize_linear_u8(img, dim) if img.dtype == np.uint8 else oo.resize_linear_f32(img, dim)

    def rgb2hsv(self, rgb):
        from oracle import observe as oo
        return oo.rgb2hsv_u8(rgb)

    def inrange(self, hsv):
        return ((hsv <= 100).all(-1) * 255).astype(np.uint8)

    def label(self, mask):
        from scipy import ndimage
        return ndimage.label(mask, structure=np.ones((3, 3), int))

    def crop_center(self, img, crop):
        from flingbot_amd import nets
        return nets.crop_center(img, crop)

    def pad(self, img, size):
        from flingbot_amd import nets
        return nets.pad(img, size)

    def resize_nearest(self, img, dim):
        from flingbot_amd import nets
        return nets.resize_nearest(img, dim)


def check_cv2_fixture(path):
    """List of (key, description) for every recorded output the repository's restatements do not reproduce exactly."""
    kit = _kit("capture_cv2")
    z = np.load(path)
    meta = json.loads(str(z["meta"]))
    assert meta["format"] == "flingbot_amd cv2 fixture v1", meta
    want = kit.inputs(meta["seed"])
    for k, v in want.items():
        assert np.array_equal(z[k], v), f"{k}: the fixture's inputs are not the kit's seeded inputs"
    be, bad = _RestatementBackend(), []

    def cmp(key, mine):
        ref = z[key]
        if mine.shape != ref.shape or not np.array_equal(mine, ref):
            worst = float(np.abs(mine.astype(np.float64) - ref.astype(np.float64)).max()) if mine.shape == ref.shape else float("nan")
            bad.append((key, f"max |diff| {worst:g}, {int((mine != ref).sum()) if mine.shape == ref.shape else -1} of {ref.size} differ"))

    for k in range(4):
        dst = int(z[f"case{k}/dst"])
        cmp(f"case{k}/resize_u8", be.resize(z[f"case{k}/rgb"], dst))
        cmp(f"case{k}/resize_f32", be.resize(z[f"case{k}/depth"], dst))
        r8 = z[f"case{k}/resize_u8"]                      # downstream stages are checked on the fixture's own upstream output
        cmp(f"case{k}/hsv", be.rgb2hsv(r8))
        cmp(f"case{k}/inrange", be.inrange(z[f"case{k}/hsv"]))
        lab, num = be.label((z[f"case{k}/inrange"] == 0).astype(np.uint8))
        if int(num) != int(z[f"case{k}/num"]):
            bad.append((f"case{k}/num", f"{int(num)} components, fixture {int(z[f'case{k}/num'])}"))
        else:  # label VALUES may be numbered differently; the partition and the raster order of first pixels must agree
            ref = z[f"case{k}/label"]
            first_mine = [np.flatnonzero(lab.ravel() == i + 1)[0] for i in range(int(num))]
            first_ref = [np.flatnonzero(ref.ravel() == i + 1)[0] for i in range(int(num))]
            if not (np.array_equal((lab > 0), (ref > 0)) and first_mine == first_ref and
                    all(np.array_equal(lab == i + 1, ref == i + 1) for i in range(int(num)))):
                bad.append((f"case{k}/label", "components are numbered / partitioned differently"))
    cmp("colours_hsv", be.rgb2hsv(z["colours"]))
    cmp("allcolours_hsv", be.rgb2hsv(z["allcolours"]))
    img = z["nearest/img"]
    for scale in kit.SCALES + kit.NEAREST_EXTRA_SCALES:
        if scale in kit.NEAREST_EXTRA_SCALES and f"nearest/scale{scale}/out" not in z.files:
            continue   # a fixture recorded before the kit knew these extents
        new_dim = int(scale * img.shape[0])
        t = be.crop_center(img, new_dim) if scale < 1 else be.pad(img, new_dim) if scale > 1 else img
        if tuple(t.shape) != tuple(z[f"nearest/scale{scale}/shape"]):
            bad.append((f"nearest/scale{scale}/shape", f"{t.shape} vs {tuple(z[f'nearest/scale{scale}/shape'])}"))
        cmp(f"nearest/scale{scale}/out", be.resize_nearest(t, 64))
    return bad, meta


def test_cv2_fixture_ingest_path_on_a_self_made_fixture(tmp_path):
    """Kit -> file -> check with the restatements standing in for cv2 / skimage: nothing differs; a fixture whose HSV plane
    was tampered with is caught."""
    kit = _kit("capture_cv2")
    path = str(tmp_path / "restated.npz")
    kit.capture(path, seed=0, backend=_RestatementBackend())
    bad, meta = check_cv2_fixture(path)
    assert bad == [] and meta["cv2"].startswith("restated")
    z = dict(np.load(path))
    z["case1/hsv"] = z["case1/hsv"].copy()
    z["case1/hsv"][5, 7, 0] ^= 1
    np.savez_compressed(str(tmp_path / "tampered.npz"), **z)
    bad, _ = check_cv2_fixture(str(tmp_path / "tampered.npz"))
    assert [k for k, _ in bad] == ["case1/hsv"]


def _nearest_index(dst, src, inverse_of_forward_scale):
    """source index of cv2.resize INTER_NEAREST under the two readings of its scale (PARITY.md)"""
    x = np.arange(dst)
    ratio = 1.0 / (dst / src) if inverse_of_forward_scale else src / dst
    return np.minimum(np.floor(x * ratio).astype(np.int64), src - 1)


def test_nearest_extra_extents_tell_the_two_index_formulas_apart():
    """The extents the kit records in addition really discriminate: floor(x * (src / dst)) and floor(x * (1 / (dst / src)))
    pick different source pixels for some x < 64 there, and the same pixels at the extents recorded all along."""
    kit = _kit("capture_cv2")
    extents = [int(s * 400) for s in kit.NEAREST_EXTRA_SCALES]
    assert extents == [186, 372, 396, 420]
    for e in extents:
        e = e if e <= 400 else 400 + 2 * ((e - 400) // 2)     # what crop_center / pad make of it
        a, b = _nearest_index(64, e, False), _nearest_index(64, e, True)
        assert 1 <= int((a != b).sum()) <= 15, (e, int((a != b).sum()))
        assert np.array_equal(a, (np.arange(64) * e) // 64)   # the repository's reading is the exact floor(x * src / dst)
    for s in kit.SCALES:
        e = int(s * 400)
        assert np.array_equal(_nearest_index(64, e, False), _nearest_index(64, e, True)), e


def test_cv2_fixture_old_format_and_other_nearest_reading(tmp_path):
    """A fixture without the added nearest/ keys (recorded by the kit before them) is accepted as before; one recorded from a
    backend that forms the nearest index the other way is reported at exactly the added extents."""
    kit = _kit("capture_cv2")
    path = str(tmp_path / "restated.npz")
    kit.capture(path, seed=0, backend=_RestatementBackend())
    z = dict(np.load(path))
    added = [k for k in z if any(k.startswith(f"nearest/scale{s}/") for s in kit.NEAREST_EXTRA_SCALES)]
    assert len(added) == 2 * len(kit.NEAREST_EXTRA_SCALES)
    old = {k: v for k, v in z.items() if k not in added}
    np.savez_compressed(str(tmp_path / "old_format.npz"), **old)
    bad, meta = check_cv2_fixture(str(tmp_path / "old_format.npz"))
    assert bad == []

    class Other(_RestatementBackend):
        def resize_nearest(self, img, dim):
            ys, xs = (_nearest_index(dim, e, True) for e in img.shape[:2])
            return img[ys][:, xs]

    kit.capture(str(tmp_path / "other.npz"), seed=0, backend=Other())
    bad, _ = check_cv2_fixture(str(tmp_path / "other.npz"))
    assert [k for k, _ in bad] == [f"nearest/scale{s}/out" for s in kit.NEAREST_EXTRA_SCALES]


@pytest.mark.skipif(not os.path.exists(CV2_FIXTURE), reason="no cv2 fixture (tests/golden/capture_cv2.py records one on a machine "
                                                            "with opencv-python and scikit-image)")
def test_restatements_against_cv2_fixture():
    bad, meta = check_cv2_fixture(CV2_FIXTURE)
    assert bad == [], (meta, bad)


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(CV2_FIXTURE) or "render/rgba" not in (np.load(CV2_FIXTURE).files if os.path.exists(CV2_FIXTURE) else ()),
                    reason="no pyflex.render() frame in the cv2 fixture (capture_cv2.py --render)")
def test_rasteriser_against_pyflex_render_frame(gpu_required, capsys):
    """One real pyflex.render() readback (pyflex.cpp:1032-1054) against fs_render on the recorded particle state: depth within
    the 24-bit depth buffer's resolution away from silhouettes, colour within 2 grey levels on >= 99 % of the pixels."""
    from flingbot_amd import sim as fsim

    z = np.load(CV2_FIXTURE)
    ctx = fsim.FlingSim(n_envs=1)
    env = ctx.env(0)
    sc.canonical_flat(env, 64)
    for p in ((0.5, 0.5, -0.5), (-0.5, 0.5, -0.5)):
        env.add_sphere(0.02, p, [1, 0, 0, 0])
    env.set_positions(z["render/positions"])
    env.set_shape_states(z["render/shape_states"])
    rgba, depth = ctx.render(0)
    ref_rgba, ref_depth = z["render/rgba"].reshape(-1, 4), z["render/depth"]
    dd = np.abs(depth.ravel() - ref_depth.ravel())
    dc = np.abs(np.asarray(rgba).reshape(-1, 4)[:, :3].astype(int) - ref_rgba[:, :3].astype(int)).max(1)
    with capsys.disabled():
        print(f"\n  fs_render vs pyflex.render: depth median |diff| {np.median(dd):.2e}, 99th pct {np.percentile(dd, 99):.2e}; "
              f"colour within 2 levels on {(dc <= 2).mean() * 100:.2f} % of the pixels")
    assert np.percentile(dd, 95) <= 2e-4 and (dc <= 2).mean() >= 0.99
    ctx.close()
