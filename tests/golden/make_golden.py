"""Generates the golden fixtures under tests/golden/ by running the importable parts of the REFERENCE in this
container (/root/reference is read-only and never travels to the GPU box; only the vectors written here do).

    python tests/golden/make_golden.py

Sources:  environment/flex_utils.py get_current_covered_area (stubs for pyflex, cv2),
          oracle/_ref/camera_ref  (compiled from the reference's PyFlex/core/maths.h by oracle/Makefile),
          oracle/_ref/sphere_ref  (compiled from the reference's PyFlex/core/mesh.cpp, same Makefile),
          learning/nets.py (stubs for cv2, ray), environment/utils.py (stubs for cv2, trimesh, ...),
          utils.py collect_stats run over an in-memory stand-in of the replay buffer's HDF5 groups (`replay`: replay_golden.npz).
"""
import json
import os
import subprocess
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"


def stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def coverage_vectors():
    stub("pyflex")
    stub("cv2")
    sys.path.insert(0, os.path.join(REF, "environment"))
    import flex_utils  # the reference module

    rng = np.random.RandomState(0)
    cases = {}

    def grid(dx, dz, sp=0.00625):
        xs, zs = np.meshgrid(np.arange(dx) * sp, np.arange(dz) * sp)
        p = np.zeros((dx * dz, 4), np.float32)
        p[:, 0], p[:, 2], p[:, 1], p[:, 3] = xs.ravel(), zs.ravel(), 0.005, 1.0
        return p

    cases["flat64"] = grid(64, 64)
    cases["flat32"] = grid(32, 32)
    cases["rect40x20"] = grid(40, 20)
    f = grid(64, 64); f[:, 0] = np.abs(f[:, 0] - 0.2); cases["folded64"] = f
    cases["random500"] = np.concatenate([rng.rand(500, 3) * [0.5, 0.2, 0.3], np.ones((500, 1))], 1).astype(np.float32)
    c = grid(32, 32); c[:, [0, 2]] *= 0.35; c[:, 0] += 0.01 * rng.randn(1024).astype(np.float32); cases["crumpled32"] = c
    cases["shifted"] = grid(48, 30) + np.array([-0.31, 0, 0.77, 0], np.float32)
    out = {}
    for k, p in cases.items():
        out["pos_" + k] = p
        out["area_" + k] = np.float64(flex_utils.get_current_covered_area(pos=p.ravel().copy()))
    np.savez_compressed(os.path.join(HERE, "coverage_golden.npz"), **out)
    print("coverage:", {k[5:]: float(v) for k, v in out.items() if k.startswith("area_")})


def coverage_edge_vectors():
    """The constructed particle sets of tests/coverage_cases.py (rounding ties, the flat-index quirk, range ends, sample
    counts, zero extent, particle counts around the wave and the block, NaN) through the reference's own
    get_current_covered_area(pos=...).  Records per case the float64 area, n and the SHA-256 of the position bytes -- no
    positions: the table regenerates them and the hash proves they are the same.  The archive's members carry a fixed date, so the
    same table gives the same bytes.  coverage_golden.npz is not touched."""
    stub("pyflex")
    stub("cv2")
    sys.path.insert(0, os.path.join(REF, "environment"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import flex_utils  # the reference module
    import coverage_cases as cc

    areas = []
    with np.errstate(divide="ignore", invalid="ignore"):  # zero extent and NaN are cases of the table
        for case in cc.CASES:
            areas.append(np.float64(flex_utils.get_current_covered_area(pos=case["pos"].ravel().copy())))
    out = {"names": np.array([c["name"] for c in cc.CASES]), "area": np.array(areas, np.float64),
           "n": np.array([c["pos"].shape[0] for c in cc.CASES], np.int64),
           "sha256": np.array([cc.sha256(c["pos"]) for c in cc.CASES])}
    path = os.path.join(HERE, "coverage_edges_golden.npz")
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:  # np.savez stamps the members with the current time
        for key, arr in out.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arr), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    print("coverage edges:", {n: float(a) for n, a in zip(out["names"].tolist(), areas)})
    print("coverage edges:", len(cc.CASES), "cases,", os.path.getsize(path), "bytes")


def camera_vectors():
    exe = os.path.join(ROOT, "oracle", "_ref", "camera_ref")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "_ref/camera_ref"])
    cases = [
        dict(cam=[0, 2, 0], ang=[np.pi / 2, -np.pi / 2, 0], w=720, h=720, lo=[-1.005, -2.005, -1.005], up=[1.005, 1.005, 1.005]),
        dict(cam=[0, 2, 0], ang=[np.pi / 2, -np.pi / 2, 0], w=720, h=720, lo=[-1.005, -0.205, -1.005], up=[1.005, 1.005, 1.005]),
        dict(cam=[0.3, 1.5, 0.7], ang=[0.4, -0.9, 0], w=640, h=480, lo=[-1.2, -0.3, -1.0], up=[1.0, 1.0, 2.5]),
    ]
    out = []
    for c in cases:
        f32 = lambda v: [float(np.float32(x)) for x in v]
        args = [repr(x) for x in (*f32(c["cam"]), *f32(c["ang"]), float(c["w"]), float(c["h"]), *f32(c["lo"]), *f32(c["up"]))]
        txt = subprocess.check_output([exe] + args).decode()
        rec = dict(c)
        rec["cam"], rec["ang"], rec["lo"], rec["up"] = f32(c["cam"]), f32(c["ang"]), f32(c["lo"]), f32(c["up"])
        for line in txt.strip().split("\n"):
            name, *vals = line.split()
            rec[name] = [float(v) for v in vals]
        out.append(rec)
    with open(os.path.join(HERE, "camera_golden.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    print("camera:", len(out), "cases")


def sphere_vectors():
    """The mesh the reference draws for a kinematic sphere: oracle/_ref/sphere_ref = the reference's own core/mesh.cpp
    CreateSphere(20, 20, r) + Mesh::Transform(Translation(prev pos) * Rotation(prev quat)) (main.cpp:1739-1751)."""
    exe = os.path.join(ROOT, "oracle", "_ref", "sphere_ref")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "_ref/sphere_ref"])
    cases = [
        # the pickers as FlingBot adds them (flex_utils.py:82-83: quat [1, 0, 0, 0] = half a turn about x), parked
        # where reset_end_effectors leaves them (simEnv.py:771-772), radius simEnv.py:129-134
        dict(radius=0.02, pos=[0.5, 0.5, -0.5], quat=[1, 0, 0, 0]),
        dict(radius=0.02, pos=[-0.5, 0.5, -0.5], quat=[1, 0, 0, 0]),
        dict(radius=0.02, pos=[0.04, 0.3, 0.0], quat=[0, 0, 0, 1]),
        dict(radius=0.05, pos=[0.123, 0.456, -0.789], quat=[0.18257419, 0.36514837, 0.54772256, 0.73029674]),
        dict(radius=0.031, pos=[-0.3, 0.07, 0.2], quat=[0.5, -0.5, 0.5, 0.5]),
    ]
    out = []
    for c in cases:
        f32 = lambda v: [float(np.float32(x)) for x in v]
        rec = dict(radius=float(np.float32(c["radius"])), pos=f32(c["pos"]), quat=f32(c["quat"]))
        txt = subprocess.check_output([exe] + [repr(x) for x in (rec["radius"], *rec["pos"], *rec["quat"])]).decode()
        for line in txt.strip().split("\n"):
            name, *vals = line.split()
            rec[name] = [int(v) for v in vals] if name in ("counts", "indices") else [float(v) for v in vals]
        assert rec["counts"] == [441, 441, 2400]
        out.append(rec)
    with open(os.path.join(HERE, "sphere_golden.json"), "w") as fh:
        json.dump(out, fh)
    print("sphere:", len(out), "cases")


def nets_vectors():
    """Reference learning/nets.py (stubs: cv2, ray): state_dict layout, a seeded forward, policy rotations."""
    import torch

    stub("cv2")
    ray = stub("ray")
    ray.remote = lambda f: f
    sys.path.insert(0, os.path.join(REF, "learning"))
    import nets as refnets  # the reference module

    torch.manual_seed(0)
    kw = dict(action_primitives=["fling"], num_rotations=12, scale_factors=[1.0, 1.25, 1.5, 1.75, 2.0, 2.25, 2.5, 2.75],
              obs_dim=64, pix_grasp_dist=16, pix_drag_dist=16, pix_place_dist=10, rgb_only=True, depth_only=False,
              action_expl_prob=0.0, action_expl_decay=0.9, value_expl_prob=0.0, value_expl_decay=0.9, device="cpu")
    pol = refnets.MaximumValuePolicy(**kw)
    g = torch.Generator().manual_seed(1)
    for m in pol.modules():  # make BatchNorm statistics non-trivial
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.2)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
            m.weight.data.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
            m.bias.data.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    pol.eval()
    sd = pol.state_dict()
    obs = torch.rand(3, 4, 24, 24, generator=g)
    obs[:, 3] = 1.9 + 0.1 * obs[:, 3]
    with torch.no_grad():
        out = pol.value_nets["fling"](obs)
        acted = pol.act([obs, obs[:2]])
    g64 = torch.Generator().manual_seed(2)  # obs_dim-sized observations (the size the hand-written forward serves)
    obs64 = torch.rand(2, 4, 64, 64, generator=g64)
    obs64[:, 3] = 1.9 + 0.1 * obs64[:, 3]
    with torch.no_grad():
        out64 = pol.value_nets["fling"](obs64)
    arrays = {"sd::" + k: v.numpy() for k, v in sd.items()}
    arrays.update(obs64=obs64.numpy(), out64=out64.numpy())
    arrays.update(obs=obs.numpy(), out=out.numpy(), act0=acted[0]["fling"].numpy(), act1=acted[1]["fling"].numpy(),
                  rotations=np.array(pol.rotations), num_transforms=np.array(pol.num_transforms))
    np.savez_compressed(os.path.join(HERE, "nets_golden.npz"), **arrays)
    with open(os.path.join(HERE, "nets_state_dict_keys.json"), "w") as fh:
        json.dump({k: list(v.shape) for k, v in sd.items()}, fh, indent=0)
    # rotate stage of transform() (scipy only; cv2 is absent so pad/resize cannot be run from the reference)
    from scipy import ndimage as nd

    img = torch.rand(4, 40, 40, generator=g)
    rots = {}
    for ang in (-90.0, -40.909, 0.0, 16.3636, 57.27, 90.0):
        rots[f"rot_{ang}"] = nd.rotate(input=img.permute(2, 1, 0), angle=ang, reshape=False, mode="nearest")
    np.savez_compressed(os.path.join(HERE, "rotate_golden.npz"), img=img.numpy(), **rots)
    print("nets:", len(sd), "state_dict entries; out", tuple(out.shape))


def _import_reference_env_utils():
    """environment/utils.py of the reference with every absent third-party module stubbed (cv2, trimesh, OpenEXR, ...)."""
    class _Any:
        def __init__(self, *a, **k): pass
        def __call__(self, *a, **k): return _Any()
        def __getattr__(self, name): return _Any()

    def anystub(name):
        m = types.ModuleType(name)

        def _ga(attr):
            if attr.startswith("__"):
                raise AttributeError(attr)
            return _Any()
        m.__getattr__ = _ga
        m.__path__ = []
        m.__file__ = "<stub %s>" % name
        sys.modules[name] = m
        return m

    for name in ("h5py", "filelock", "imageio", "trimesh", "OpenEXR", "Imath", "cv2", "PIL", "skimage", "skimage.morphology",
                 "matplotlib", "matplotlib.pyplot", "ray", "pyflex"):
        if name != "pyflex":
            try:
                __import__(name)
                continue
            except Exception:
                pass
        anystub(name)
    sys.modules["ray"].remote = lambda f: f
    for m in [k for k in sys.modules if k == "environment" or k.startswith("environment.") or k in ("flex_utils", "nets")]:
        del sys.modules[m]
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from environment import utils as ref_utils
    return ref_utils


def envutils_vectors():
    """environment/utils.py:161-276, 579-582 -- compute_pose, compute_intrinsics, pixel_to_3d, get_transform_matrix,
    pixels_to_3d_positions, preprocess_obs -- run here on seeded inputs.  The product's host mirror
    (flingbot_amd/action.py) has to reproduce every output bit for bit (float64)."""
    U = _import_reference_env_utils()
    rng = np.random.default_rng(11)
    out = {}
    poses = [([0, 2, 0], [0, 0, 0], [0, 0, 1]), ([0.3, 1.5, -0.2], [0.1, 0.0, 0.05], [0, 0, 1]),
             ([1.0, 1.0, 1.0], [0, 0.2, 0], [0, 1, 0])]
    out["pose_in"] = np.array(poses, np.float64)
    out["pose_out"] = np.stack([U.compute_pose(pos=p, lookat=l, up=u) for p, l, u in poses])
    out["intrinsics_in"] = np.array([[39.5978, 400], [39.5978, 720], [60.0, 97]], np.float64)
    out["intrinsics_out"] = np.stack([U.compute_intrinsics(f, s) for f, s in out["intrinsics_in"]])
    tm = [(400, 64, -30.0, 1.5), (400, 64, 90.0, 0.75), (720, 64, 16.363636363636363, 2.75), (100, 32, 0.0, 1.0),
          (60, 24, -180.0, 2.0), (97, 33, 49.09090909090909, 1.25)]
    out["tm_in"] = np.array(tm, np.float64)
    out["tm_out"] = np.stack([U.get_transform_matrix(original_dim=int(a), resized_dim=int(b), rotation=r, scale=s)
                              for a, b, r, s in tm])
    # pixel_to_3d: float32 depth image like the renderer's, several pixels, two poses (the function scales the depth
    # value it reads IN PLACE -- `click_z *= depth_scale` on a numpy scalar copy -- so the image itself stays untouched)
    depth = (2.0 - rng.random((96, 96)) * 0.4).astype(np.float32)
    pts = np.array([[0, 0], [95, 95], [48, 47], [10, 80], [77, 3], [31, 64]])
    out["p3d_depth"] = depth
    out["p3d_xy"] = pts
    out["p3d_out"] = np.stack([np.stack([U.pixel_to_3d(depth.copy(), int(x), int(y), pose_matrix=out["pose_out"][k])
                                         for x, y in pts]) for k in range(2)])
    out["p3d_scaled"] = U.pixel_to_3d(depth.copy(), 20, 30, pose_matrix=out["pose_out"][0], fov=50.0, depth_scale=0.5)
    # pixels_to_3d_positions: in bounds, out of bounds, pretransform_pix_only
    big = (2.0 - rng.random((120, 120)) * 0.3).astype(np.float32)
    cases = [(np.array([[10, 12], [20, 12]]), 1.5, 30.0, False), (np.array([[16, 16], [16, 24]]), 1.0, -90.0, False),
             (np.array([[2, 2], [29, 29]]), 2.75, 73.63636363636364, False), (np.array([[5, 27], [13, 27]]), 0.75, 0.0, True),
             (np.array([[0, 0], [31, 31]]), 3.5, 45.0, False)]
    out["pp_depth"] = big
    for k, (pix, scale, rot, only) in enumerate(cases):
        r = U.pixels_to_3d_positions(pixels=pix, scale=scale, rotation=rot, pretransform_depth=big.copy(),
                                     transformed_depth=np.zeros((32, 32), np.float32), pose_matrix=out["pose_out"][0],
                                     pretransform_pix_only=only)
        out[f"pp{k}_in"] = np.array([*pix.ravel(), scale, rot, float(only)], np.float64)
        out[f"pp{k}_valid"] = np.array(bool(r["valid_action"]))
        out[f"pp{k}_pixels"] = np.asarray(r["pretransform_pixels"])
        out[f"pp{k}_has_points"] = np.array(r.get("p1") is not None)
        if r.get("p1") is not None:
            out[f"pp{k}_p1"], out[f"pp{k}_p2"] = np.asarray(r["p1"]), np.asarray(r["p2"])
    out["pp_n"] = np.array(len(cases))
    # preprocess_obs
    rgb = rng.integers(0, 256, (40, 40, 3), dtype=np.uint8)
    d = (2.0 - rng.random((40, 40)) * 0.5).astype(np.float32)
    out["obs_rgb"], out["obs_d"] = rgb, d
    out["obs_out"] = U.preprocess_obs(rgb.copy(), d.copy()).numpy()
    np.savez_compressed(os.path.join(HERE, "envutils_golden.npz"), **out)
    print("envutils:", {k: getattr(v, "shape", None) for k, v in out.items() if k.endswith("_out")},
          "pixel_to_3d(d=2, 300, 200) =", U.pixel_to_3d(np.full((400, 400), 2.0, np.float32), 300, 200, out["pose_out"][0]))


def step_vectors():
    """The reference's SimEnv.step (environment/simEnv.py:464-515: preaction, coverage before, action handler, postaction =
    reset_end_effectors + wait_until_stable + the "cloth did not move -> end early" test, coverage after, timestep /
    episode_length termination, reward) executed by the reference's own code on the oracle-backed `pyflex` stub, with the
    action selection scripted (get_max_value_valid_action returns a prepared (primitive, action) per step) and get_obs /
    prepare_image / episode memory / reset stubbed -- what is pinned is the bookkeeping around the primitives, which
    tests/golden/fling_golden.npz pins separately.  Before the first step the episode is brought up exactly like
    SimEnv.reset does after set_scene (simEnv.py:674-681)."""
    sys.path.insert(0, ROOT)
    from oracle import OracleSim

    if not hasattr(np, "alltrue"):
        np.alltrue = np.all
    import torch  # noqa: F401
    import scipy.ndimage  # noqa: F401

    class _Any:
        def __init__(self, *a, **k): pass
        def __call__(self, *a, **k): return _Any()
        def __getattr__(self, name): return _Any()

    def anystub(name):
        m = types.ModuleType(name)

        def _ga(attr):
            if attr.startswith("__"):
                raise AttributeError(attr)
            return _Any()
        m.__getattr__ = _ga
        m.__path__ = []
        m.__file__ = "<stub %s>" % name
        sys.modules[name] = m
        return m

    for name in ("h5py", "filelock", "imageio", "trimesh", "OpenEXR", "Imath", "cv2", "PIL", "skimage", "skimage.morphology",
                 "matplotlib", "matplotlib.pyplot", "ray", "pyflex"):
        if name not in ("pyflex",):
            try:
                __import__(name)
                continue
            except Exception:
                pass
        anystub(name)
    sys.modules["ray"].remote = lambda f: f
    orc_box = {}
    pf = sys.modules["pyflex"]
    for name in ("get_positions", "set_positions", "get_velocities", "set_velocities", "get_shape_states",
                 "set_shape_states", "add_sphere", "get_phases", "set_phases"):
        setattr(pf, name, (lambda nm: lambda *a, **k: getattr(orc_box["o"], nm)(*a, **k))(name))
    counter = {"steps": 0}

    def _step(*a, **k):
        counter["steps"] += 1
        orc_box["o"].step(1)
    pf.step = _step
    for m in [k for k in sys.modules if k == "environment" or k.startswith("environment.") or k in ("flex_utils", "nets")]:
        del sys.modules[m]
    sys.path.insert(0, REF)
    from environment import simEnv as ref_simenv
    from environment import flex_utils as ref_fu
    ref_simenv.prepare_image = lambda *a, **k: "transformed_obs"
    SimEnv = ref_simenv.SimEnv

    sp = np.array([0, 0.2, 0, 32, 32, 0.9, 0.9, 0.9, 2, 0, 2, 0, np.pi / 2, -np.pi / 2, 0, 720, 720, 0.3, 0])
    dim = 32
    xs = (np.arange(dim) - (dim - 1) / 2) * 0.00625
    xx, zz = np.meshgrid(xs, xs)
    corner = dict(p1=[xs[0], 0.0, xs[0]], p2=[xs[-1], 0.0, xs[0]])
    miss = dict(p1=[xs[0] - 0.05, 0.0, xs[0] - 0.05], p2=[xs[-1] + 0.05, 0.0, xs[0] - 0.05])
    # (episode_length, [(primitive or None, p1, p2, p1_grasp_cloth, p2_grasp_cloth), ...])
    cases = [
        (5, [("fling", corner["p1"], corner["p2"], True, True), (None, None, None, None, None)]),  # fling, then nothing moves
        (1, [("fling", [xs[3], 0.0, xs[20]], [xs[-4], 0.0, xs[20]], True, True)]),              # episode_length reached
        (5, [("fling", miss["p1"], miss["p2"], True, True)]),              # grasp misses: terminated inside the handler,
                                                                            # postaction runs with the grasp flags still set
        (5, [("fling", corner["p1"], corner["p2"], False, False), ("drag", [xs[5], 0.0, xs[5]], [xs[5] + 0.1, 0.0, xs[5]], True, True)]),
    ]
    out = {"scene_params": sp, "n_cases": np.array(len(cases))}
    for ci, (episode_length, script) in enumerate(cases):
        orc = OracleSim()
        orc_box["o"] = orc
        orc.set_scene(sp)
        orc.step(1)
        n = orc.n
        w = orc.get_positions().reshape(-1, 4)[0, 3]
        pos = np.zeros((n, 4), np.float32)
        pos[:, 0], pos[:, 1], pos[:, 2], pos[:, 3] = xx.ravel(), 0.0125, zz.ravel(), w
        orc.set_positions(pos.ravel())
        orc.set_velocities(np.zeros(3 * n, np.float32))
        out["init_pos"] = pos
        env = SimEnv.__new__(SimEnv)
        env.gui, env.gui_step, env.dump_visualizations = False, 0, False
        env.default_speed, env.grasp_height, env.fling_speed, env.fixed_fling_height = 1e-2, 0.02, 6e-3, -1
        env.stretchdrag_dist = 0.3
        env.particle_radius = 0.00625
        env.grasp_states = [False, False]
        env.env_video_frames = {}
        env.episode_memory = _Any()
        env.current_task = _Any()
        env.obs_dim, env.parallelize_prepare_image, env.ray_handle = 64, False, {"val": "handle"}
        env.episode_length = episode_length
        env.action_handlers = {"fling": env.pick_and_fling_primitive, "stretchdrag": env.pick_stretch_drag_primitive,
                               "drag": env.pick_and_drag_primitive, "place": env.pick_and_place_primitive}
        env.get_obs = lambda: "obs"
        env.get_transformations = lambda: []
        env.on_episode_end = lambda *a, **k: None
        env.reset = lambda: ("reset", None)
        covs = []

        def cov(_env=env):
            c = SimEnv.compute_coverage(_env)
            covs.append(float(c))
            return c
        env.compute_coverage = cov
        todo = list(script)

        def scripted(value_maps):
            prim, p1, p2, g1, g2 = todo.pop(0)
            if prim is None:
                return None, None
            return prim, dict(p1=np.array(p1, np.float64), p2=np.array(p2, np.float64), p1_grasp_cloth=g1, p2_grasp_cloth=g2)
        env.get_max_value_valid_action = scripted
        env.action_tool = ref_fu.PickerPickPlace(num_picker=2, particle_radius=0.00625, picker_radius=0.02,
                                                 picker_low=(-5, 0, -5), picker_high=(5, 5, 5))
        # SimEnv.reset after set_scene (simEnv.py:674-681)
        env.current_timestep, env.terminate = 0, False
        env.init_coverage = ref_fu.get_current_covered_area(env.particle_radius)
        env.action_tool.reset([0.2, 0.5, 0.0])
        env.reset_end_effectors()
        env.step_simulation()
        env.set_grasp(False)
        out[f"c{ci}_init_coverage"] = np.array(float(env.init_coverage))
        out[f"c{ci}_episode_length"] = np.array(episode_length)
        out[f"c{ci}_prim"] = np.array([str(a[0]) for a in script])
        out[f"c{ci}_p1"] = np.array([a[1] if a[1] is not None else [np.nan] * 3 for a in script], np.float64)
        out[f"c{ci}_p2"] = np.array([a[2] if a[2] is not None else [np.nan] * 3 for a in script], np.float64)
        out[f"c{ci}_g1"] = np.array([bool(a[3]) for a in script])
        out[f"c{ci}_g2"] = np.array([bool(a[4]) for a in script])
        log = {k: [] for k in ("prev", "curr", "reward", "terminate", "timestep", "sim_steps", "grasp", "returned_reset", "pos",
                               "shapes")}
        for k in range(len(script)):
            counter["steps"] = 0
            del covs[:]
            ret = env.step(None)
            log["prev"].append(covs[0])
            log["curr"].append(covs[1])
            log["reward"].append(covs[1] - covs[0])
            log["terminate"].append(bool(env.terminate))
            log["timestep"].append(int(env.current_timestep))
            log["sim_steps"].append(counter["steps"])
            log["grasp"].append([bool(g) for g in env.grasp_states])
            log["returned_reset"].append(ret == ("reset", None))
            log["pos"].append(orc.get_positions().copy())
            log["shapes"].append(orc.get_shape_states().copy())
            print("step case", ci, "action", script[k][0], "reward %.5f" % log["reward"][-1], "terminate", env.terminate,
                  "timestep", env.current_timestep, "sim steps", counter["steps"], "grasp", env.grasp_states)
            if env.terminate:
                break
        for key, v in log.items():
            out[f"c{ci}_{key}"] = np.array(v)
    np.savez_compressed(os.path.join(HERE, "step_golden.npz"), **out)


def picker_vectors():
    """Reference Picker / PickerPickPlace (environment/flex_utils.py) driven through a `pyflex` stub that is backed by
    the CPU oracle; the movep loop is simEnv.py:739-769 verbatim in behaviour (SimEnv itself needs ray/h5py/trimesh to
    import, so its 30-line loop is driven from here).  Records the full particle / shape trajectory."""
    sys.path.insert(0, ROOT)
    from oracle import OracleSim

    if not hasattr(np, "alltrue"):  # the reference targets numpy 1.x (flex_utils.py:245,251); same function
        np.alltrue = np.all
    orc = OracleSim()
    pf = stub("pyflex")
    for name in ("get_positions", "set_positions", "get_velocities", "set_velocities", "get_shape_states",
                 "set_shape_states", "add_sphere", "get_phases", "set_phases"):
        setattr(pf, name, getattr(orc, name))
    pf.step = lambda *a, **k: orc.step(1)
    stub("cv2")
    sys.path.insert(0, os.path.join(REF, "environment"))
    import importlib
    import flex_utils
    importlib.reload(flex_utils)  # bind to the oracle-backed stub

    sp = np.array([0, 0.2, 0, 24, 24, 0.9, 0.9, 0.9, 2, 0, 2, 0, np.pi / 2, -np.pi / 2, 0, 720, 720, 0.3, 0])
    orc.set_scene(sp)
    orc.step(1)
    n = orc.n
    w = orc.get_positions().reshape(-1, 4)[0, 3]
    xs = (np.arange(24) - 11.5) * 0.00625
    xx, zz = np.meshgrid(xs, xs)
    pos = np.zeros((n, 4), np.float32)
    pos[:, 0], pos[:, 1], pos[:, 2], pos[:, 3] = xx.ravel(), 0.0125, zz.ravel(), w
    orc.set_positions(pos.ravel())
    orc.set_velocities(np.zeros(3 * n, np.float32))

    tool = flex_utils.PickerPickPlace(num_picker=2, particle_radius=0.00625, picker_radius=0.02,
                                      picker_low=(-5, 0, -5), picker_high=(5, 5, 5))
    tool.reset([0.0, 0.1, 0.0])
    grasp_states = [False, False]
    log = {"pos": [], "shapes": [], "picked": [], "iters": []}

    def movep(target, speed, limit=1000, min_steps=None, eps=1e-4):
        target_pos = np.array(target)
        for step in range(limit):
            curr_pos = tool._get_pos()[0]
            deltas = [(targ - curr) for targ, curr in zip(target_pos, curr_pos)]
            dists = [np.linalg.norm(delta) for delta in deltas]
            if all([dist < eps for dist in dists]) and (min_steps is None or step > min_steps):
                log["iters"].append(step)
                return
            action = []
            for targ, curr, delta, dist, gs in zip(target_pos, curr_pos, deltas, dists, grasp_states):
                if dist < speed:
                    action.extend([*targ, float(gs)])
                else:
                    delta = delta / dist
                    action.extend([*(curr + delta * speed), float(gs)])
            tool.step(np.array(action), step_sim_fn=lambda: orc.step(1))
            log["pos"].append(orc.get_positions().copy())
            log["shapes"].append(orc.get_shape_states().copy())
            log["picked"].append([-1 if q is None else q for q in tool.picked_particles])
        raise RuntimeError("limit")

    p0 = pos[0, :3].astype(np.float64) + [0, 0.02, 0]
    p1 = pos[23, :3].astype(np.float64) + [0, 0.02, 0]
    program = [([p0, p1], 0.1, None, [False, False]),                               # approach (simEnv.py:297)
               ([p0 + [0, 0.12, 0], p1 + [0, 0.12, 0]], 5e-3, None, [True, True]),   # grasp + lift (:299-304)
               ([p0 + [0, 0.12, 0.02], p1 + [0, 0.12, 0.02]], 5e-4, 20, [True, True]),  # stretch-like, min_steps
               ([p0 + [0, 0.12, -0.06], p1 + [0, 0.12, -0.06]], 6e-3, None, [True, True]),  # fling back
               ([p0 + [0, 0.05, -0.06], p1 + [0, 0.05, -0.06]], 6e-3, None, [True, False])]  # release one picker
    for target, speed, min_steps, gs in program:
        grasp_states[:] = gs
        movep(target, speed, min_steps=min_steps)
    np.savez_compressed(os.path.join(HERE, "picker_golden.npz"), scene_params=sp, init_pos=pos,
                        targets=np.array([t for t, _, _, _ in program]), speeds=np.array([s for _, s, _, _ in program]),
                        min_steps=np.array([-1 if m is None else m for _, _, m, _ in program]),
                        grasp=np.array([g for _, _, _, g in program]), iters=np.array(log["iters"]),
                        picked=np.array(log["picked"]), shapes=np.array(log["shapes"]),
                        pos_every_10=np.array(log["pos"][::10]), pos_last=log["pos"][-1])
    print("picker:", len(log["pos"]), "sim steps, iters", log["iters"], "picked", log["picked"][-1])


def picker_edge_vectors():
    """The constructed particle sets of tests/picker_cases.py (ties, the inclusive threshold, contested and released
    particles, empty searches, 1 to 16 pickers, 1 to 272 particles) run through the reference's own PickerPickPlace on the
    oracle-backed `pyflex` stub, with the movep loop of picker_vectors().  Each case's picker count and radii go to the
    constructor; Picker.reset places the spheres by its own rule, then the case's centres are set through the stub.
    Records, per case and simulated step, the picked indices, the shape states and the particle positions with w, and per
    movep the iteration count."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle import OracleSim
    import picker_cases as pc

    if not hasattr(np, "alltrue"):
        np.alltrue = np.all
    box = {}
    pf = stub("pyflex")
    for name in ("get_positions", "set_positions", "get_velocities", "set_velocities", "get_shape_states",
                 "set_shape_states", "add_sphere", "get_phases", "set_phases"):
        setattr(pf, name, (lambda nm: lambda *a, **k: getattr(box["o"], nm)(*a, **k))(name))
    pf.step = lambda *a, **k: box["o"].step(1)
    stub("cv2")
    sys.path.insert(0, os.path.join(REF, "environment"))
    import importlib
    import flex_utils
    importlib.reload(flex_utils)  # bind to the oracle-backed stub

    out = {"names": np.array([c["name"] for c in pc.CASES])}
    for case in pc.CASES:
        orc = OracleSim()
        box["o"] = orc
        pc.setup(orc, case)
        tool = flex_utils.PickerPickPlace(num_picker=case["num_picker"], particle_radius=case["particle_radius"],
                                          picker_radius=case["picker_radius"], picker_threshold=case["picker_threshold"],
                                          picker_low=(-5, 0, -5), picker_high=(5, 5, 5))
        tool.reset([0.0, 0.1, 0.0])
        pc.set_centres(pf, case)
        log = {"pos": [], "shapes": [], "picked": [], "iters": []}

        def movep(target, grasp_states, speed, limit=1000, min_steps=None, eps=1e-4):
            target_pos = np.array(target)
            for step in range(limit):
                curr_pos = tool._get_pos()[0]
                deltas = [(targ - curr) for targ, curr in zip(target_pos, curr_pos)]
                dists = [np.linalg.norm(delta) for delta in deltas]
                if all([dist < eps for dist in dists]) and (min_steps is None or step > min_steps):
                    log["iters"].append(step)
                    return
                action = []
                for targ, curr, delta, dist, gs in zip(target_pos, curr_pos, deltas, dists, grasp_states):
                    if dist < speed:
                        action.extend([*targ, float(gs)])
                    else:
                        delta = delta / dist
                        action.extend([*(curr + delta * speed), float(gs)])
                if tool.step(np.array(action), step_sim_fn=lambda: orc.step(1)):  # None / 0: no simulated step was taken
                    log["pos"].append(orc.get_positions().reshape(-1, 4).copy())
                    log["shapes"].append(orc.get_shape_states().copy())
                    log["picked"].append([-1 if q is None else q for q in tool.picked_particles])
            raise RuntimeError("limit")

        for m in case["program"]:
            movep(m["targets"], [bool(g) for g in m["grasp"]], m["speed"], min_steps=m["min_steps"])
        name = case["name"]
        out[name + ":picked"] = np.array(log["picked"], np.int32)
        out[name + ":shapes"] = np.array(log["shapes"], np.float32)
        out[name + ":pos"] = np.array(log["pos"], np.float32)
        out[name + ":iters"] = np.array(log["iters"], np.int32)
        assert np.isfinite(out[name + ":pos"]).all(), name
        print("picker edge", name, "steps", len(log["picked"]), "iters", log["iters"], "picked", log["picked"])
    np.savez_compressed(os.path.join(HERE, "picker_edges_golden.npz"), **out)
    print("picker edges:", len(pc.CASES), "cases,", os.path.getsize(os.path.join(HERE, "picker_edges_golden.npz")), "bytes")


def fling_vectors():
    """The reference's SimEnv.pick_and_fling_primitive (with stretch_cloth, lift_cloth, fling_primitive, movep,
    is_cloth_grasped, reset_end_effectors: environment/simEnv.py:140-318,739-813) followed by
    flex_utils.wait_until_stable (flex_utils.py:430-441), executed by the reference's own code on a `pyflex` stub that is
    backed by the CPU oracle.  SimEnv is instantiated without __init__ (which needs ray / HDF5 task files); every module
    the import chain wants but this image lacks is replaced by an empty stub."""
    sys.path.insert(0, ROOT)
    from oracle import OracleSim

    if not hasattr(np, "alltrue"):
        np.alltrue = np.all
    import torch  # noqa: F401  (before the stubs: its import machinery inspects sys.modules)
    import scipy.ndimage  # noqa: F401

    class _Any:
        def __init__(self, *a, **k): pass
        def __call__(self, *a, **k): return _Any()
        def __getattr__(self, name): return _Any()

    def anystub(name):
        m = types.ModuleType(name)

        def _ga(attr):
            if attr.startswith("__"):
                raise AttributeError(attr)
            return _Any()
        m.__getattr__ = _ga
        m.__path__ = []
        m.__file__ = "<stub %s>" % name
        sys.modules[name] = m
        return m

    for name in ("h5py", "filelock", "imageio", "trimesh", "OpenEXR", "Imath", "cv2", "PIL", "skimage", "skimage.morphology",
                 "matplotlib", "matplotlib.pyplot", "ray", "pyflex"):
        if name not in ("pyflex",):
            try:
                __import__(name)
                continue
            except Exception:
                pass
        anystub(name)
    sys.modules["ray"].remote = lambda f: f
    orc_box = {}
    pf = sys.modules["pyflex"]
    for name in ("get_positions", "set_positions", "get_velocities", "set_velocities", "get_shape_states",
                 "set_shape_states", "add_sphere", "get_phases", "set_phases"):
        setattr(pf, name, (lambda nm: lambda *a, **k: getattr(orc_box["o"], nm)(*a, **k))(name))
    counter = {"steps": 0}

    def _step(*a, **k):
        counter["steps"] += 1
        orc_box["o"].step(1)
    pf.step = _step
    for m in [k for k in sys.modules if k == "environment" or k.startswith("environment.") or k in ("flex_utils", "nets")]:
        del sys.modules[m]
    sys.path.insert(0, REF)
    from environment import simEnv as ref_simenv
    from environment import flex_utils as ref_fu
    SimEnv = ref_simenv.SimEnv

    sp = np.array([0, 0.2, 0, 32, 32, 0.9, 0.9, 0.9, 2, 0, 2, 0, np.pi / 2, -np.pi / 2, 0, 720, 720, 0.3, 0])
    dim = 32
    xs = (np.arange(dim) - (dim - 1) / 2) * 0.00625
    xx, zz = np.meshgrid(xs, xs)
    cases = [  # (p1, p2, p1_grasp, p2_grasp): corners of the sheet / one-handed / a grasp that misses the cloth
        ([xs[0], 0.0, xs[0]], [xs[-1], 0.0, xs[0]], True, True),
        ([xs[2], 0.0, xs[5]], [xs[-8], 0.0, xs[-3]], True, False),
        ([xs[0] - 0.05, 0.0, xs[0] - 0.05], [xs[-1] + 0.05, 0.0, xs[0] - 0.05], True, True),
        ([xs[4], 0.0, xs[0]], [xs[-5], 0.0, xs[0]], False, False),
    ]
    rec = {k: [] for k in ("dist", "height", "terminate", "steps_fling", "stable", "steps_stable", "pos_fling", "pos_final",
                           "shapes_final", "stretch_ret", "lift_ret")}
    init_pos = None
    for p1, p2, g1, g2 in cases:
        orc = OracleSim()
        orc_box["o"] = orc
        orc.set_scene(sp)
        orc.step(1)
        n = orc.n
        w = orc.get_positions().reshape(-1, 4)[0, 3]
        pos = np.zeros((n, 4), np.float32)
        pos[:, 0], pos[:, 1], pos[:, 2], pos[:, 3] = xx.ravel(), 0.0125, zz.ravel(), w
        init_pos = pos
        orc.set_positions(pos.ravel())
        orc.set_velocities(np.zeros(3 * n, np.float32))
        env = SimEnv.__new__(SimEnv)
        env.gui = False
        env.gui_step = 0
        env.dump_visualizations = False
        env.default_speed = 1e-2
        env.grasp_height = 0.02
        env.fling_speed = 6e-3
        env.fixed_fling_height = -1
        env.particle_radius = 0.00625
        env.terminate = False
        env.grasp_states = [False, False]
        env.env_video_frames = {}
        env.action_tool = ref_fu.PickerPickPlace(num_picker=2, particle_radius=0.00625, picker_radius=0.02,
                                                 picker_low=(-5, 0, -5), picker_high=(5, 5, 5))
        env.action_tool.reset([0.0, 0.1, 0.0])
        rets = {"stretch": None, "lift": None}
        o_stretch, o_lift = SimEnv.stretch_cloth, SimEnv.lift_cloth

        def stretch(self, *a, _o=o_stretch, **k):
            rets["stretch"] = _o(self, *a, **k)
            return rets["stretch"]

        def lift(self, *a, _o=o_lift, **k):
            rets["lift"] = _o(self, *a, **k)
            return rets["lift"]
        SimEnv.stretch_cloth, SimEnv.lift_cloth = stretch, lift
        counter["steps"] = 0
        try:
            env.pick_and_fling_primitive(np.array(p1, np.float64), np.array(p2, np.float64), g1, g2)
        finally:
            SimEnv.stretch_cloth, SimEnv.lift_cloth = o_stretch, o_lift
        rec["terminate"].append(bool(env.terminate))
        rec["stretch_ret"].append(np.nan if rets["stretch"] is None else float(rets["stretch"]))
        rec["lift_ret"].append(np.nan if rets["lift"] is None else float(rets["lift"]))
        rec["steps_fling"].append(counter["steps"])
        rec["pos_fling"].append(orc.get_positions().copy())
        counter["steps"] = 0
        stable = ref_fu.wait_until_stable(max_steps=150, tolerance=1e-2, step_sim_fn=env.step_simulation)
        rec["stable"].append(bool(stable))
        rec["steps_stable"].append(counter["steps"])
        # wait_until_stable with something to wait for: the cloth as it lies, lifted by 0.25 and dropped
        lifted = orc.get_positions().reshape(-1, 4).copy()
        lifted[:, 1] += np.float32(0.25)
        orc.set_positions(lifted.ravel())
        vel = np.zeros((n, 3), np.float32)
        vel[:, 1] = -0.5  # moving: the test that precedes every step must fail at first
        orc.set_velocities(vel.ravel())
        counter["steps"] = 0
        stable2 = ref_fu.wait_until_stable(max_steps=60 + 30 * len(rec["stable"]), tolerance=2e-2,
                                           step_sim_fn=env.step_simulation)
        rec.setdefault("stable_drop", []).append(bool(stable2))
        rec.setdefault("steps_drop", []).append(counter["steps"])
        rec["pos_final"].append(orc.get_positions().copy())
        rec["shapes_final"].append(orc.get_shape_states().copy())
        print("fling case", len(rec["stable"]), "terminate", env.terminate, "stretch", rets["stretch"], "lift", rets["lift"],
              "steps", rec["steps_fling"][-1], "stable", stable, "| drop: stable", stable2, "after", counter["steps"])
    # ---- the other manipulation primitives (simEnv.py:320-428) on the same sheet
    pcases = [("drag", [xs[3], 0.0, xs[4]], [xs[3] + 0.08, 0.0, xs[4] + 0.03], True, True),
              ("place", [xs[-4], 0.0, xs[6]], [xs[8], 0.0, xs[-6]], True, False),
              ("stretchdrag", [xs[1], 0.0, xs[2]], [xs[-2], 0.0, xs[2]], True, True),
              ("stretchdrag", [xs[1], 0.0, xs[-3]], [xs[-2] + 0.06, 0.0, xs[-3]], True, False),
              ("drag", [xs[3], 0.0, xs[4]], [xs[9], 0.0, xs[4]], False, True)]
    prec = {"pos": [], "shapes": [], "steps": [], "stretch_ret": []}
    for kind, p1, p2, g1, g2 in pcases:
        orc = OracleSim()
        orc_box["o"] = orc
        orc.set_scene(sp)
        orc.step(1)
        orc.set_positions(init_pos.ravel())
        orc.set_velocities(np.zeros(3 * init_pos.shape[0], np.float32))
        env = SimEnv.__new__(SimEnv)
        env.gui = False
        env.gui_step = 0
        env.dump_visualizations = False
        env.default_speed = 1e-2
        env.grasp_height = 0.02
        env.stretchdrag_dist = 0.1
        env.particle_radius = 0.00625
        env.terminate = False
        env.grasp_states = [False, False]
        env.env_video_frames = {}
        env.action_tool = ref_fu.PickerPickPlace(num_picker=2, particle_radius=0.00625, picker_radius=0.02,
                                                 picker_low=(-5, 0, -5), picker_high=(5, 5, 5))
        env.action_tool.reset([0.0, 0.1, 0.0])
        rets = {"stretch": None}
        o_stretch = SimEnv.stretch_cloth

        def stretch2(self, *a, _o=o_stretch, **k):
            rets["stretch"] = _o(self, *a, **k)
            return rets["stretch"]
        SimEnv.stretch_cloth = stretch2
        counter["steps"] = 0
        try:
            fn = {"drag": env.pick_and_drag_primitive, "place": env.pick_and_place_primitive,
                  "stretchdrag": env.pick_stretch_drag_primitive}[kind]
            fn(np.array(p1, np.float64), np.array(p2, np.float64), g1, g2)
        finally:
            SimEnv.stretch_cloth = o_stretch
        prec["pos"].append(orc.get_positions().copy())
        prec["shapes"].append(orc.get_shape_states().copy())
        prec["steps"].append(counter["steps"])
        prec["stretch_ret"].append(np.nan if rets["stretch"] is None else float(rets["stretch"]))
        print("primitive", kind, g1, g2, "steps", counter["steps"], "stretch", rets["stretch"])
    np.savez_compressed(os.path.join(HERE, "primitives_golden.npz"), scene_params=sp, init_pos=init_pos,
                        kind=np.array([c[0] for c in pcases]), p1=np.array([c[1] for c in pcases]),
                        p2=np.array([c[2] for c in pcases]), g1=np.array([c[3] for c in pcases]),
                        g2=np.array([c[4] for c in pcases]), steps=np.array(prec["steps"]),
                        stretch_ret=np.array(prec["stretch_ret"]), pos=np.array(prec["pos"]),
                        shapes=np.array(prec["shapes"]), stretchdrag_dist=np.array(0.1))
    np.savez_compressed(os.path.join(HERE, "fling_golden.npz"), scene_params=sp, init_pos=init_pos,
                        p1=np.array([c[0] for c in cases]), p2=np.array([c[1] for c in cases]),
                        g1=np.array([c[2] for c in cases]), g2=np.array([c[3] for c in cases]),
                        terminate=np.array(rec["terminate"]), stretch_ret=np.array(rec["stretch_ret"]),
                        lift_ret=np.array(rec["lift_ret"]), steps_fling=np.array(rec["steps_fling"]),
                        stable=np.array(rec["stable"]), steps_stable=np.array(rec["steps_stable"]),
                        stable_drop=np.array(rec["stable_drop"]), steps_drop=np.array(rec["steps_drop"]),
                        pos_fling=np.array(rec["pos_fling"]), pos_final=np.array(rec["pos_final"]),
                        shapes_final=np.array(rec["shapes_final"]))


def action_vectors():
    """The reference's SimEnv.get_max_value_valid_action (environment/simEnv.py:560-661, with check_action :202-260,
    get_action_params :517-537, check_action_reachability :542-558 and environment/utils.py pixels_to_3d_positions /
    get_transform_matrix / pixel_to_3d / compute_pose) on synthetic value maps and depth images.  SimEnv is instantiated
    without __init__; conservative_grasp_radius = 0 (the cloth-mask circles need cv2, absent here, and do not take part in
    the selection); visualisation / logging hooks are no-ops."""
    import torch
    import scipy.ndimage  # noqa: F401

    class _Any:
        def __init__(self, *a, **k): pass
        def __call__(self, *a, **k): return _Any()
        def __getattr__(self, name): return _Any()

    def anystub(name):
        m = types.ModuleType(name)

        def _ga(attr):
            if attr.startswith("__"):
                raise AttributeError(attr)
            return _Any()
        m.__getattr__ = _ga
        m.__path__ = []
        m.__file__ = "<stub %s>" % name
        sys.modules[name] = m
        return m

    for name in ("h5py", "filelock", "imageio", "trimesh", "OpenEXR", "Imath", "cv2", "PIL", "skimage", "skimage.morphology",
                 "matplotlib", "matplotlib.pyplot", "ray", "pyflex"):
        if name != "pyflex":
            try:
                __import__(name)
                continue
            except Exception:
                pass
        anystub(name)
    sys.modules["ray"].remote = lambda f: f
    for m in [k for k in sys.modules if k == "environment" or k.startswith("environment.") or k in ("flex_utils", "nets")]:
        del sys.modules[m]
    sys.path.insert(0, REF)
    from environment import simEnv as ref_simenv
    ref_simenv.visualize_action = lambda **k: None
    SimEnv = ref_simenv.SimEnv

    rng = np.random.default_rng(7)
    cases = []
    # (primitives, obs_dim D, pretransform S, pix distances, reach limit, scales)
    setups = [(["fling"], 32, 100, (8, 8, 5), 0.8, [0.75, 1.0, 1.5, 2.0]),
              (["fling", "drag", "place"], 24, 72, (4, 6, 3), 0.7, [1.0, 1.25, 2.5]),
              (["stretchdrag", "fling"], 24, 60, (5, 5, 5), 0.75, [1.0, 2.0]),
              (["fling"], 32, 100, (8, 8, 5), 0.45, [1.0, 2.75])]
    out = {}
    for ci, (prims, D, S, (gd, dd, pd), reach, scales) in enumerate(setups):
        env = SimEnv.__new__(SimEnv)
        num_rot = 6
        env.rotations = [(2 * i / (num_rot - 1) - 1) * 90 for i in range(num_rot)]
        if "fling" not in prims:
            env.rotations = [(2 * i / num_rot - 1) * 180 for i in range(num_rot)]
        env.adaptive_scale_factors = np.array(scales)
        env.obs_dim = D
        env.pix_grasp_dist, env.pix_drag_dist, env.pix_place_dist = gd, dd, pd
        env.conservative_grasp_radius = 0
        env.left_arm_base = np.array([0.765, 0, 0])
        env.right_arm_base = np.array([-0.765, 0, 0])
        env.reach_distance_limit = reach
        env.stretchdrag_dist = 0.3
        env.grasp_height = 0.02
        env.log_step_stats = lambda kw: None
        T = num_rot * len(scales)
        # depth: plane at 2.0 (camera height) with a cloth blob closer to the camera
        yy, xx = np.mgrid[0:S, 0:S]
        depth = np.full((S, S), 2.0, np.float32)
        blob = ((xx - S * 0.55) ** 2 + (yy - S * 0.45) ** 2) < (S * 0.3) ** 2
        depth[blob] = (1.98 - 0.05 * rng.random(blob.sum())).astype(np.float32)
        env.pretransform_depth = depth
        env.pretransform_rgb = np.zeros((S, S, 3), np.float32)
        env.transformed_obs = torch.zeros(T, 4, D, D)
        value_maps = {p: torch.tensor(rng.random((T, D, D)).astype(np.float32)) for p in prims}
        if ci == 1:  # ties: quantised values, the first in flattened order must win
            value_maps = {p: torch.round(v * 6) / 6 for p, v in value_maps.items()}
        action, params = env.get_max_value_valid_action(value_maps)
        out[f"c{ci}_prims"] = np.array(prims)
        out[f"c{ci}_cfg"] = np.array([D, S, gd, dd, pd, num_rot], np.int64)
        out[f"c{ci}_reach"] = np.array([reach, 0.3, 0.02])
        out[f"c{ci}_scales"] = np.array(scales)
        out[f"c{ci}_rotations"] = np.array(env.rotations)
        out[f"c{ci}_depth"] = depth
        out[f"c{ci}_values"] = np.stack([value_maps[p].numpy() for p in prims])
        out[f"c{ci}_action"] = np.array("" if action is None else action)
        if action is not None:
            out[f"c{ci}_p1"] = np.array(params["p1"], np.float64)
            out[f"c{ci}_p2"] = np.array(params["p2"], np.float64)
            out[f"c{ci}_g"] = np.array([params["p1_grasp_cloth"], params["p2_grasp_cloth"]])
        print("action case", ci, "->", action, None if params is None else (params["p1"], params["p2"]))
    np.savez_compressed(os.path.join(HERE, "action_golden.npz"), **out)


def task_vectors():
    """The reference's task generator generate_randomization(task_difficulty='hard', grid cloth)
    (environment/tasks.py:105-275, with flex_utils set_scene / set_to_flatten / center_object / wait_until_stable /
    get_current_covered_area) on the oracle-backed `pyflex` stub, for seeded random draws and a reduced cloth-size range
    (the generator's own min/max arguments) so the CPU oracle finishes in seconds."""
    sys.path.insert(0, ROOT)
    from oracle import OracleSim
    import random
    import torch  # noqa: F401
    import scipy.ndimage  # noqa: F401

    if not hasattr(np, "alltrue"):
        np.alltrue = np.all
    if not hasattr(np, "float"):
        np.float = float  # flex_utils.py:406 (numpy 1.x alias)

    class _Any:
        def __init__(self, *a, **k): pass
        def __call__(self, *a, **k): return _Any()
        def __getattr__(self, name): return _Any()

    def anystub(name):
        m = types.ModuleType(name)

        def _ga(attr):
            if attr.startswith("__"):
                raise AttributeError(attr)
            return _Any()
        m.__getattr__ = _ga
        m.__path__ = []
        m.__file__ = "<stub %s>" % name
        sys.modules[name] = m
        return m

    for name in ("h5py", "filelock", "imageio", "trimesh", "OpenEXR", "Imath", "cv2", "PIL", "skimage", "skimage.morphology",
                 "matplotlib", "matplotlib.pyplot", "ray", "pyflex"):
        if name != "pyflex":
            try:
                __import__(name)
                continue
            except Exception:
                pass
        anystub(name)
    sys.modules["ray"].remote = lambda f: f
    box = {}
    pf = sys.modules["pyflex"]
    for name in ("get_positions", "set_positions", "get_velocities", "set_velocities", "get_shape_states",
                 "set_shape_states", "add_sphere", "get_phases", "set_phases"):
        setattr(pf, name, (lambda nm: lambda *a, **k: getattr(box["o"], nm)(*a, **k))(name))
    counter = {"steps": 0}

    def _step(*a, **k):
        counter["steps"] += 1
        box["o"].step(1)
    pf.step = _step
    pf.set_scene = lambda scene_idx=0, scene_params=None, vertices=(), stretch_edges=(), bend_edges=(), shear_edges=(), \
        faces=(), thread_idx=0: box["o"].set_scene(scene_params, vertices, stretch_edges, bend_edges, shear_edges, faces)
    for m in [k for k in sys.modules if k == "environment" or k.startswith("environment.") or k in ("flex_utils", "nets")]:
        del sys.modules[m]
    sys.path.insert(0, REF)
    from environment import tasks as ref_tasks
    from environment import flex_utils as ref_fu

    out = {}
    # load_cloth (environment/tasks.py:39-103) on a small synthetic quad mesh (ours: a 6 x 5 vertex sheet with a notch cut
    # out, OBJ faces in v/vt form, shuffled face order): vertices, triangles, stretch / bend / shear edge lists in the
    # reference's own order (the order of its Python sets), which fixes the spring ids the solver accumulates in.
    rng = np.random.RandomState(4)
    nx, ny = 6, 5
    lines = ["# synthetic quad mesh for tests/golden (not reference data)"]
    for j in range(ny):
        for i in range(nx):
            lines.append("v %.6f %.6f %.6f" % (0.02 * i, 0.003 * ((i * 7 + j * 3) % 5), 0.025 * j))
    for j in range(ny):
        for i in range(nx):
            lines.append("vt %.4f %.4f" % (i / (nx - 1), j / (ny - 1)))
    quads = [(i, j) for j in range(ny - 1) for i in range(nx - 1) if not (i >= 3 and j >= 2)]
    for q in rng.permutation(len(quads)):
        i, j = quads[q]
        ids = [j * nx + i + 1, j * nx + i + 2, (j + 1) * nx + i + 2, (j + 1) * nx + i + 1]
        lines.append("f " + " ".join("%d/%d" % (v, v) for v in ids))
    obj_text = "\n".join(lines) + "\n"
    import tempfile
    with tempfile.NamedTemporaryFile("w", suffix="_processed.obj", delete=False) as fh:
        fh.write(obj_text)
        obj_path = fh.name
    verts, tri_faces, stretch, bend, shear = ref_tasks.load_cloth(obj_path)
    os.unlink(obj_path)
    out["obj_text"] = np.array(obj_text)
    out["obj_vertices"], out["obj_faces"] = np.asarray(verts), np.asarray(tri_faces)
    out["obj_stretch"], out["obj_bend"], out["obj_shear"] = np.asarray(stretch), np.asarray(bend), np.asarray(shear)
    print("load_cloth:", verts.shape, tri_faces.shape, stretch.shape, bend.shape, shear.shape)
    for ci, (seed, difficulty) in enumerate(((3, "hard"), (11, "hard"), (5, "easy"))):
        random.seed(seed)
        np.random.seed(seed)
        box["o"] = OracleSim()
        tool = ref_fu.PickerPickPlace(num_picker=2, particle_radius=0.00625, picker_radius=0.05,
                                      picker_low=(-5, 0, -5), picker_high=(5, 5, 5))
        counter["steps"] = 0
        task = ref_tasks.generate_randomization(tool, min_cloth_size=20, strict_min_edge_length=20, max_cloth_size=30,
                                                task_difficulty=difficulty, cloth_type="grid")
        print("task", ci, "seed", seed, None if task is None else (task["cloth_size"], float(task["cloth_mass"]),
              float(task["initial_coverage"]), float(task["flatten_area"])), "steps", counter["steps"])
        assert task is not None
        out[f"t{ci}_seed"] = np.array(seed)
        out[f"t{ci}_difficulty"] = np.array(difficulty)
        out[f"t{ci}_steps"] = np.array(counter["steps"])
        for k in ("particle_pos", "particle_vel", "shape_pos", "phase", "cloth_size", "cloth_stiff"):
            out[f"t{ci}_{k}"] = np.asarray(task[k])
        for k in ("initial_coverage", "flatten_area", "cloth_mass"):
            out[f"t{ci}_{k}"] = np.array(float(task[k]))
    np.savez_compressed(os.path.join(HERE, "task_golden.npz"), **out)


def replay_vectors():
    """utils.collect_stats (utils.py:186-390) -- the function run_sim.py prints its evaluation statistics with -- run on a
    synthetic episode log: the reference's OWN code walks the groups of an in-memory stand-in for the HDF5 file (h5py is absent;
    only `for k in file`, `file.get(k)` and `group.attrs[...]` are served, which is all collect_stats touches before its
    try / except image block) and its return values are stored next to the log.  flingbot_amd.taskio.collect_stats must give
    the same numbers from the same log written by taskio.save_replay.  This pins the STATISTICS (filters, per-level lists, the
    best-coverage bookkeeping, the 128-point window), not the HDF5 container."""
    _import_reference_env_utils()
    import h5py as h5stub          # the stub module installed above (or the real one, if this machine has it)

    class _Any:
        def __init__(self, *a, **k): pass
        def __call__(self, *a, **k): return _Any()
        def __getattr__(self, name): return _Any()

    for name in ("torchvision", "torchvision.transforms", "tensorboardX"):     # what utils.py / learning/utils.py import on top
        try:
            __import__(name)
        except Exception:
            m = types.ModuleType(name)
            m.__getattr__ = lambda attr: (_ for _ in ()).throw(AttributeError(attr)) if attr.startswith("__") else _Any()
            m.__path__ = []
            sys.modules[name] = m
    rng = np.random.RandomState(7)
    episodes = []                  # (task name, difficulty, max coverage, init coverage, [(pre, post, primitive)])
    for i in range(90):
        level = "hard" if i % 3 else "easy"
        mx = 0.05 + 0.1 * rng.rand()
        cov = mx * (0.2 + 0.3 * rng.rand())
        init = cov
        steps = []
        for k in range(int(rng.randint(1, 5))):
            post = min(mx, max(0.0, cov + mx * (rng.rand() - 0.35) * 0.5))
            if i == 7 and k == 0:
                post = 0.01 * mx                        # below 5 % of the flattened area: collect_stats skips the entry
            steps.append((float(cov), float(post), "fling" if (i + k) % 4 else "drag"))
            cov = post
        episodes.append(("task%03d" % i, level, float(mx), float(init), steps))
    groups = {}
    for i, (name, level, mx, init, steps) in enumerate(episodes):
        for k, (pre, post, prim) in enumerate(steps):
            key = "%09d_step%02d" % (i, k) + ("_last" if k == len(steps) - 1 else "")
            groups[key] = {"preaction_coverage": pre, "postaction_coverage": post, "max_coverage": mx, "init_coverage": init,
                           "task_difficulty": level, "action_primitive": prim, "task_name": name}

    class Group:
        def __init__(self, attrs): self.attrs = attrs
        def __getitem__(self, k): raise KeyError(k)     # no datasets: the image block of collect_stats falls into its except

    class File:
        def __init__(self, path, mode="r"): pass
        def __enter__(self): return self
        def __exit__(self, *a): return False
        def __iter__(self): return iter(sorted(groups))          # HDF5 lists group names in sorted order
        def get(self, k): return Group(groups[k])

    h5stub.File = File
    for m in [k for k in sys.modules if k == "utils" or k.startswith("learning")]:
        del sys.modules[m]
    import random
    import tempfile
    cwd = os.getcwd()
    os.chdir(REF)
    try:
        import utils as ref_top
    finally:
        os.chdir(cwd)
    ref_top.h5py.File = File
    out = {"n_groups": np.array(len(groups))}
    with tempfile.TemporaryDirectory() as tmp:
        for tag, kw in (("latest128", {}), ("all", {"num_points": 10 ** 6})):
            random.seed(0)
            res = ref_top.collect_stats(os.path.join(tmp, "replay_buffer.hdf5"), **kw)
            for k, v in res.items():
                if "_steps" in k or k.startswith("img_"):
                    continue
                out[f"{tag}:{k}"] = np.asarray(v, np.float64)
    keys = sorted(groups)
    out["keys"] = np.array(keys)
    for f in ("preaction_coverage", "postaction_coverage", "max_coverage", "init_coverage", "task_difficulty", "action_primitive",
              "task_name"):
        out["log:" + f] = np.array([groups[k][f] for k in keys])
    np.savez_compressed(os.path.join(HERE, "replay_golden.npz"), **out)
    print("replay:", len(groups), "groups;", len([k for k in out if k.startswith("all:")]), "statistics of the reference's collect_stats")


if __name__ == "__main__":
    which = sys.argv[1:] or ["coverage", "coverage_edges", "camera", "sphere", "nets", "envutils", "picker", "picker_edges", "fling", "action", "task", "step", "replay"]
    if "replay" in which:
        replay_vectors()
    if "coverage" in which:
        coverage_vectors()
    if "coverage_edges" in which:
        coverage_edge_vectors()
    if "camera" in which:
        camera_vectors()
    if "sphere" in which:
        sphere_vectors()
    if "nets" in which and "nets_vectors" in globals():
        nets_vectors()
    if "envutils" in which:
        envutils_vectors()
    if "picker" in which:
        picker_vectors()
    if "picker_edges" in which:
        picker_edge_vectors()
    if "fling" in which:
        fling_vectors()
    if "action" in which:
        action_vectors()
    if "task" in which:
        task_vectors()
    if "step" in which:
        step_vectors()
