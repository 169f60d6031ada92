"""Per-episode appearance on the GPU: the shading kernels (csrc/fs_raster_kernels.h: fs_k_shade / fs_k_shade_capture and their
textured forms) against tests/appearance_reference.py on the 96 x 64 scenes of tests/raster_scenes.py, fs_fork / fs_set_scene,
the observation stage on drawn grounds, and the loops (evaluate.run_tasks, lookahead.run_episodes) with
BatchedFlingEnv(randomize_appearance=...).

Colour gate: test_raster_synthetic_gpu.py's -- at most 1 level, on fewer than 2 % of the channels -- and on the scenes that
module compares colours on (raster_scenes: Scene.colour; on `pickers` a sphere sunk into the ground brings PCF compares to their
thresholds, so there the frame is checked through what must not move: depth, alpha, z-keys, shadow map, and every sphere
pixel's bytes)."""
import random

import numpy as np
import pytest
import torch

import appearance_reference as ar
import raster_scenes as rs
from flingbot_amd import appearance

pytestmark = pytest.mark.gpu

SCENE_NAMES = ("tilted_fold", "pickers", "borders_and_planes")
CLOTH_COLOURS = {"default": None, "blue": (0.05, 0.6, 0.9), "darkest": "hsv(0.3, 1, 0.5)"}
TEXTURES = ((1, 2.0, 1), (7, 16.0, 4), (123456789, 8.0, 6))      # (seed, cells_per_m, octaves)
GROUND = np.array([[0.02, 0.05, 0.03], [0.1, 0.09, 0.05]], np.float32)
_ctx, _base = [], {}


def _scene(name):
    return getattr(rs, name)()


def _sim():
    from flingbot_amd import sim as fsim

    if not _ctx:
        _ctx.append(fsim.FlingSim(n_envs=2))
    return _ctx[0]


def _cloth(which):
    import colorsys

    if CLOTH_COLOURS[which] is None:
        return appearance.default()["cloth_rgb"]
    if which == "darkest":      # the darkest cloth the draw allows: v = 0.5 at full saturation
        return np.array(colorsys.hsv_to_rgb(0.3, 1.0, 0.5), np.float32)
    return np.array(CLOTH_COLOURS[which], np.float32)


def _textured(seed, cells, octaves, cloth=None):
    return dict(cloth_rgb=appearance.default()["cloth_rgb"] if cloth is None else cloth, ground_rgb=GROUND, ground_seed=seed,
                ground_cells_per_m=cells, ground_octaves=octaves)


def _frame(env, sc):
    rgba, depth = env.render()
    zkeys, shadow = env.render_buffers()
    return dict(rgba=rgba.reshape(sc.H, sc.W, 4).copy(), depth=depth.copy(), zkeys=zkeys, shadow=shadow)


def _capture(sim, sc):
    """Captured frames of episode 0 at the scene's size with nothing simulated in between: two pickers far outside the frame
    and the light's map are "moved" to where they are (float32 targets = their positions: iterations that take no step, filmed
    after iterations 0 and 4 all the same).  Returns (frames uint8 [F, H, W, 3], render()'s RGBA of the same state)."""
    for c in ((5.0, 0.5, 5.0), (5.2, 0.5, 5.0)):
        sim.add_sphere(0, 0.02, list(c), [1, 0, 0, 0])
    sim.picker_reset(0, picker_radius=0.02)
    plain = sim.render(0)[0].reshape(sc.H, sc.W, 4).copy()
    hold = sim.get_shape_states(0).reshape(-1, 14)[:, :3].astype(np.float32)
    sim.capture_enable(0, sc.W, sc.H)
    try:
        sim.movep(0, hold, [[0] * len(hold)], speed=1e-2, min_steps=5)
        frames = sim.capture_take(0)
    finally:
        sim.capture_disable(0)
    sim.clear_shapes(0)
    return frames, plain


def base(name):
    """The scene under the default appearance, on a context that never called the setter for it: rendered once per scene."""
    if name not in _base:
        sc = _scene(name)
        env = _sim().env(0)
        rs.install(env, sc)
        _base[name] = _frame(env, sc)
    return _base[name]


def _install(name, ap):
    sc = _scene(name)
    env = _sim().env(0)
    rs.install(env, sc)       # (set_scene: the default appearance is back)
    if ap is not None:
        env.set_appearance(ap)
    return sc, env


def _gate(rgba, ref, what):
    diff = np.abs(rgba[..., :3].astype(int) - ref["rgba"][..., :3].astype(int))
    print(f"{what}: colour max difference {diff.max()}, share of differing channels {(diff > 0).mean():.5f}")
    assert diff.max() <= 1, f"{what}: max colour difference {diff.max()} on {(diff > 1).sum()} channels"
    assert (diff > 0).mean() < 0.02, (what, (diff > 0).mean())


def _same_geometry(got, want):
    assert np.array_equal(got["depth"].view(np.uint32), want["depth"].view(np.uint32))
    assert np.array_equal(got["rgba"][..., 3], want["rgba"][..., 3])
    assert np.array_equal(got["zkeys"], want["zkeys"]) and np.array_equal(got["shadow"], want["shadow"])


# ---- 5. the off path -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_default_appearance_renders_the_bytes_of_a_context_that_never_set_one(gpu_required, name):
    """Never set / default() set explicitly / the float64 reference the renderer was pinned to before the setter existed:
    render() RGBA and depth and render_buffers() are identical bytes, and so is a captured frame (flipped rows, no alpha)."""
    want = base(name)
    sc, env = _install(name, appearance.default())
    assert appearance.equal(env.get_appearance(), appearance.default())
    got = _frame(env, sc)
    _same_geometry(got, want)
    assert np.array_equal(got["rgba"], want["rgba"])
    if sc.colour:
        _gate(got["rgba"], rs.reference(sc), f"{name} default")     # the parent's behaviour: test_raster_synthetic_gpu's reference
    if name == "tilted_fold":
        sim = _sim()
        rs.install(env, sc)                                         # (never set since this set_scene)
        never, plain = _capture(sim, sc)
        sim.set_appearance(0, appearance.default())
        explicit, _ = _capture(sim, sc)
        assert len(never) >= 2 and np.array_equal(never, explicit)
        assert all(np.array_equal(f, plain[::-1, :, :3]) for f in never)
        assert np.array_equal(plain, want["rgba"])                  # (the pickers are out of sight and cast no shadow into it)


# ---- 6. cloth colour -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(CLOTH_COLOURS))
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_cloth_colour(gpu_required, name, which):
    ap = dict(appearance.default(), cloth_rgb=_cloth(which))
    sc, env = _install(name, ap)
    got = _frame(env, sc)
    _same_geometry(got, base(name))
    ref = ar.render(sc, ap)
    assert np.array_equal(got["rgba"][~ref["sphere"] & ~_cloth_pixels(ref)], base(name)["rgba"][~ref["sphere"] & ~_cloth_pixels(ref)])
    assert np.array_equal(got["rgba"][ref["sphere"]], base(name)["rgba"][ref["sphere"]])     # only the cloth changes
    if which != "default" and _cloth_pixels(ref).any():
        assert not np.array_equal(got["rgba"], base(name)["rgba"])
    if sc.colour:
        _gate(got["rgba"], ref, f"{name} cloth {which}")


def _cloth_pixels(ref):
    ids = (ref["keys"] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return (ref["keys"] != np.uint64(0xFFFFFFFFFFFFFFFF)) & (ids > 0) & ~ref["sphere"]


# ---- 7. textured ground ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tex", TEXTURES, ids=lambda t: f"seed{t[0]}-cells{t[1]:g}-oct{t[2]}")
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_textured_ground(gpu_required, name, tex):
    ap = _textured(*tex, cloth=_cloth("blue"))
    sc, env = _install(name, ap)
    assert appearance.equal(env.get_appearance(), ap)
    got = _frame(env, sc)
    _same_geometry(got, base(name))
    ref = ar.render(sc, ap)
    assert np.array_equal(got["rgba"][ref["sphere"]], base(name)["rgba"][ref["sphere"]])
    if sc.colour:
        _gate(got["rgba"], ref, f"{name} texture {tex}")
    if ref["ground"].any():
        levels = len(np.unique(got["rgba"][ref["ground"]][:, :3], axis=0))
        print(f"{name} texture {tex}: {levels} distinct ground colours on {int(ref['ground'].sum())} pixels")
        assert levels >= 8, "the ground ignores the texture"
        env.set_appearance(dict(ap, ground_seed=tex[0] + 1))
        other = env.render()[0].reshape(sc.H, sc.W, 4)
        assert not np.array_equal(other[ref["ground"]], got["rgba"][ref["ground"]])
        assert np.array_equal(other[~ref["ground"]], got["rgba"][~ref["ground"]])
        env.set_appearance(ap)
    else:
        assert name == "borders_and_planes"        # the ground is beyond the far plane: nothing of the texture shows
        assert np.array_equal(got["rgba"], _frame_with(env, sc, dict(ap, ground_octaves=0))["rgba"])
    if name == "tilted_fold":                      # the capture form: flipped rows of render()'s RGB, byte for byte
        frames, plain = _capture(_sim(), sc)
        assert len(frames) >= 2 and all(np.array_equal(f, plain[::-1, :, :3]) for f in frames)
        assert np.array_equal(plain, got["rgba"])                   # (the pickers are out of sight and cast no shadow into it)


def _frame_with(env, sc, ap):
    env.set_appearance(ap)
    return _frame(env, sc)


def test_texture_is_fixed_in_the_world_when_the_camera_moves(gpu_required):
    """The same ground point shows the same albedo from two camera positions: the frame from a camera moved by (dx, dz)
    matches the float64 reference of ITS frame (the rule is evaluated at world coordinates)."""
    sc = rs.Scene("moved_camera", 12, 12, rs.tilted_fold().pos, 96, 64, cam_pos=(0.31, 2.0, -0.17), why="tilted_fold seen from aside")
    ap = _textured(7, 16.0, 4)
    env = _sim().env(0)
    rs.install(env, sc)
    env.set_appearance(ap)
    _gate(_frame(env, sc)["rgba"], ar.render(sc, ap), "moved camera")


# ---- 3 (device half) / 8. setter refusals, fork, set_scene -------------------------------------------------------------------
def test_setter_refuses_bad_arguments_and_keeps_the_stored_value(gpu_required):
    from flingbot_amd import sim as fsim
    from test_appearance_cpu import _bad_appearances

    sim = _sim()
    sc, env = _install("tilted_fold", None)
    good, bad = _bad_appearances()
    env.set_appearance(good)
    for name, a in bad.items():
        with pytest.raises(fsim.FlingSimError, match="fs_appearance"):
            env.set_appearance(a)
        assert appearance.equal(env.get_appearance(), good), name
    # all or nothing over a list; an episode without a scene; an index outside the context
    fresh = fsim.FlingSim(n_envs=2)
    try:
        rs.install(fresh.env(0), sc)
        with pytest.raises(fsim.FlingSimError, match="no scene"):
            fresh.set_appearance([0, 1], [good, good])
        assert appearance.equal(fresh.get_appearance(0), appearance.default())
        assert appearance.equal(fresh.get_appearance(1), appearance.default())
        with pytest.raises(fsim.FlingSimError, match="out of range"):
            fresh.set_appearance([0, 2], [good, good])
        rs.install(fresh.env(1), sc)
        with pytest.raises(fsim.FlingSimError, match="fs_appearance"):
            fresh.set_appearance([0, 1], [good, bad["octaves 7"]])
        assert appearance.equal(fresh.get_appearance(0), appearance.default())
        fresh.set_appearance([1, 0], [good, _textured(1, 2.0, 1)])
        assert appearance.equal(fresh.get_appearance(1), good) and fresh.get_appearance(0)["ground_octaves"] == 1
    finally:
        fresh.close()
    assert sim.get_appearance(0)["ground_seed"] == good["ground_seed"]


def test_fork_copies_the_appearance_and_set_scene_restores_the_default(gpu_required):
    sim = _sim()
    ap = _textured(7, 16.0, 4, cloth=_cloth("blue"))
    sc, env = _install("tilted_fold", ap)
    want = _frame(env, sc)
    rs.install(sim.env(1), rs.lattice(False))      # slot 1 holds another scene with the default appearance ...
    sim.fork([0], [1])                             # ... and is overwritten by the fork
    assert appearance.equal(sim.get_appearance(1), ap)
    got = _frame(sim.env(1), sc)
    assert np.array_equal(got["rgba"], want["rgba"]) and np.array_equal(got["depth"], want["depth"])
    sim.set_appearance(1, dict(ap, ground_seed=8))                   # the copies are independent
    assert appearance.equal(sim.get_appearance(0), ap)
    rs.install(sim.env(1), sc)
    assert appearance.equal(sim.get_appearance(1), appearance.default())
    assert np.array_equal(_frame(sim.env(1), sc)["rgba"], base("tilted_fold")["rgba"])
    assert appearance.equal(sim.get_appearance(0), ap)


# ---- 9. the observation stage on drawn grounds -------------------------------------------------------------------------------
def test_observation_on_drawn_grounds(gpu_required):
    """One 16 x 16 cloth, camera 180 x 180, observe(env, 100, want_mask=True), the default cloth colour on 32 drawn grounds:
    the depth plane is the default appearance's bit for bit; the mask differs from the default's only next to its border (the
    bilinear resize blends cloth with a ground that is no longer black); the bounding box moves by at most one pixel a side."""
    from scenarios import cloth_params

    sim = _sim()
    env = sim.env(0)
    env.set_scene(cloth_params(16, 16, pos=(0.0, 0.02, 0.0)))
    env.step(5)                                   # (the scene's particles start under the ground plane: contacts lift them out)
    cp = sim.get_camera_params(0)
    sim.set_camera_params(0, [*cp[2:8], 180, 180])
    obs0, bbox0, mask0 = sim.observe(0, 100, want_mask=True)
    obs0, mask0 = obs0.cpu().numpy(), mask0.cpu().numpy().astype(bool)
    assert bbox0[4] > 20
    pad = np.pad(mask0, 1)
    windows = np.stack([pad[dy:dy + 100, dx:dx + 100] for dy in range(3) for dx in range(3)])
    border = windows.any(0) & ~windows.all(0)      # pixels with both mask and background in their 3 x 3 neighbourhood
    worst = 0
    for k in range(32):
        drawn = appearance.draw((5, k, 0))
        sim.set_appearance(0, dict(drawn, cloth_rgb=appearance.default()["cloth_rgb"]))
        obs, bbox, mask = sim.observe(0, 100, want_mask=True)
        obs, mask = obs.cpu().numpy(), mask.cpu().numpy().astype(bool)
        assert np.array_equal(obs[3].view(np.uint32), obs0[3].view(np.uint32)), k
        assert not np.array_equal(obs[:3], obs0[:3])
        changed = mask != mask0
        worst = max(worst, int(changed.sum()))
        assert not (changed & ~border).any(), f"ground {k}: {int((changed & ~border).sum())} mask pixels away from the border changed"
        assert np.abs(bbox[:4].astype(int) - bbox0[:4].astype(int)).max() <= 1, (k, bbox, bbox0)
    print(f"observation: at most {worst} mask pixels changed (all on the border), of {int(mask0.sum())}")


# ---- 10. the loops -----------------------------------------------------------------------------------------------------------
ROTATIONS, SCALES, SEED = 3, (1.0, 1.5), 3


def _env_policy(slots, **env_kwargs):
    from flingbot_amd import nets, sim as fsim
    from flingbot_amd.env import BatchedFlingEnv

    ctx = fsim.FlingSim(n_envs=slots, solver=0)
    env = BatchedFlingEnv(ctx, image_dim=128, num_rotations=ROTATIONS, scale_factors=SCALES, episode_length=2, **env_kwargs)
    torch.manual_seed(SEED)
    policy = nets.MaximumValuePolicy(action_primitives=["fling"], num_rotations=ROTATIONS, scale_factors=list(env.scale_factors),
                                     obs_dim=64, pix_grasp_dist=8, pix_drag_dist=8, pix_place_dist=5, rgb_only=True,
                                     depth_only=False, action_expl_prob=0.0, action_expl_decay=1.0, value_expl_prob=0.0,
                                     value_expl_decay=1.0, device="cuda:0")
    return ctx, env, policy


@pytest.fixture(scope="module")
def tasks(gpu_required):
    from flingbot_amd import sim as fsim, tasks as ftasks

    random.seed(SEED); np.random.seed(SEED)   # noqa: E702
    gen = fsim.FlingSim(n_envs=4, solver=0)
    made = ftasks.generate_tasks(gen, [ftasks.draw_task_parameters(min_cloth_size=24, strict_min_edge_length=24, max_cloth_size=32)
                                       for _ in range(4)])
    gen.close()
    assert all(t is not None for t in made)
    return made


def _run_tasks(tasks, slots, mode):
    from flingbot_amd import evaluate

    ctx, env, policy = _env_policy(slots, randomize_appearance=mode, record_experience=True)
    try:
        return evaluate.run_tasks(policy, env, tasks, seed=SEED)["records"]
    finally:
        ctx.close()


def _records_equal(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert ra["actions"] == rb["actions"] and ra["coverage"] == rb["coverage"] and ra["rewards"] == rb["rewards"]
        assert len(ra["appearance"]) == len(rb["appearance"]) == len(ra["actions"])
        assert all(np.array_equal(x, y) for x, y in zip(ra["appearance"], rb["appearance"]))
        for ea, eb in zip(ra["experience"], rb["experience"]):
            assert (ea is None) == (eb is None)
            if ea is not None:
                assert all(np.array_equal(ea[f], eb[f]) for f in ea)


def test_run_tasks_draws_from_seed_task_and_step_whatever_the_slots(gpu_required, tasks):
    two, four = _run_tasks(tasks, 2, "observation"), _run_tasks(tasks, 4, "observation")
    _records_equal(two, four)
    assert sum(len(r["actions"]) for r in two) >= 5, "episodes of one action show nothing about the timestep"
    for ti, rec in enumerate(two):
        for step, row in enumerate(rec["appearance"]):
            assert row.dtype == np.float32 and np.array_equal(row, appearance.as_row(appearance.draw((SEED, ti, step)))), (ti, step)


def test_run_tasks_episode_mode_and_flag_off(gpu_required, tasks):
    from flingbot_amd import evaluate

    for ti, rec in enumerate(_run_tasks(tasks, 4, "episode")):
        for row in rec["appearance"]:
            assert np.array_equal(row, appearance.as_row(appearance.draw((SEED, ti, 0))))
    ctx, env, policy = _env_policy(4, record_experience=True)
    try:
        calls = []
        ctx.set_appearance = lambda *a: calls.append(a)
        off = evaluate.run_tasks(policy, env, tasks, seed=SEED)["records"]
    finally:
        ctx.close()
    assert not calls and all("appearance" not in r for r in off)     # off: no call is added, the records are what they were


def test_lookahead_lanes_share_their_trunks_appearance(gpu_required, tasks):
    from flingbot_amd import evaluate, lookahead

    ctx, env, policy = _env_policy(2, randomize_appearance="observation", record_experience=True)
    try:
        got = lookahead.run_episodes(policy, env, tasks[:1], 2, follow="best", seed=SEED)
    finally:
        ctx.close()
    lanes = got["lane_records"]
    assert max(r["rank"] for r in lanes) == 1, "a run that never executed a second lane shows nothing"
    for r in lanes:
        assert np.array_equal(r["appearance"][0], appearance.as_row(appearance.draw((SEED, 0, r["step"])))), (r["step"], r["rank"])
    rec = got["records"][0]
    assert len(rec["appearance"]) == len(rec["actions"])
    assert all(np.array_equal(row, appearance.as_row(appearance.draw((SEED, 0, k)))) for k, row in enumerate(rec["appearance"]))
    # the lock-step loop keys the same way
    ctx, env, policy = _env_policy(1, randomize_appearance="observation")
    try:
        lock = evaluate.run_episodes(policy, env, tasks[:1], seed=SEED)["records"][0]
    finally:
        ctx.close()
    assert all(np.array_equal(row, appearance.as_row(appearance.draw((SEED, 0, k)))) for k, row in enumerate(lock["appearance"]))
