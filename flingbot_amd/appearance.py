"""Domain-randomised appearance: what the renderer draws an episode's cloth and ground with (include/flingsim.h
fs_appearance; FlingSim.set_appearance).

The reference's paper configuration renders through Blender "with domain randomization to help with sim2real transfer"
(README.md:178-184): every render call draws a fresh cloth colour, hsv = (U(0, 1), U(0, 1), U(0.5, 1)) turned into RGB
(render_rgbd.py:30-32), and shows a fresh slice of a procedural noise texture on the ground plane (render_rgbd.py:26-37).
`draw` restates the colour draw; the ground -- two albedos and the parameters of the fractal value noise of
csrc/fs_raster_kernels.h -- is this project's own rule, as the texture is.

An appearance is a plain dictionary: cloth_rgb float32 [3], ground_rgb float32 [2, 3] (linear albedos where the noise is
0 / 1), ground_seed int, ground_cells_per_m float, ground_octaves int (0: a flat ground of ground_rgb[0]).

Why the ground's ranges are what they are: the reference's cloth mask (simEnv.py:699-707) calls a pixel background only when
its 8-bit H, S and V are all <= 100.  Under the top-down camera a fully lit ground of albedo c shades to
(1.021 c)^(1 / 2.2), so V <= 100 / 255 needs c <= 0.125: the value stops at 0.1 (V = 90).  Hues near red wrap to H ~ 179
under the ambient term's tint, and greys can do the same at a rounding boundary, hence a hue range in the yellows and
greens and a saturation floor that keeps the channel order fixed.  tests/test_appearance_cpu.py checks the whole range.
"""
import colorsys

import numpy as np

TAG = 0x61707072   # "appr": the fourth word of every key, so that these draws never coincide with the exploration's
                   # (nets.MaximumValuePolicy._explore draws from default_rng((seed, task, step)))
ROW = 12           # floats of an appearance as a row of a record (as_row)
GROUND_HUE, GROUND_SATURATION, GROUND_VALUE = (1.0 / 12.0, 5.0 / 12.0), (0.1, 0.3), (0.02, 0.1)
GROUND_CELLS_PER_M, GROUND_OCTAVES = (2.0, 16.0), 4
MODES = ("observation", "episode")


def default():
    """The constants of csrc/fs_camera.h:114-115 -- the reference's OpenGL look: one pink cloth, a black ground."""
    f = np.float32
    return dict(cloth_rgb=np.array([f(0.612) * f(1.5), f(0.194) * f(1.5), f(0.394) * f(1.5)], np.float32),
                ground_rgb=np.full((2, 3), 0.001, np.float32), ground_seed=0, ground_cells_per_m=0.0, ground_octaves=0)


def draw(key):
    """The appearance of key (a sequence of non-negative integers, e.g. (seed, task index, timestep)): a pure function of
    it, every draw from np.random.default_rng([*key, TAG]) in this order -- cloth h in [0, 1), s in [0, 1), v in [0.5, 1)
    (the reference's three uniforms, then colorsys.hsv_to_rgb); for each of the two ground albedos hue, saturation, value
    in the ranges above; the seed (below 2^24: exact in a float32 row); log2 of cells_per_m."""
    rng = np.random.default_rng([*(int(k) for k in key), TAG])
    h, s, v = rng.uniform(0.0, 1.0), rng.uniform(0.0, 1.0), rng.uniform(0.5, 1.0)
    cloth = colorsys.hsv_to_rgb(h, s, v)
    ground = [colorsys.hsv_to_rgb(rng.uniform(*GROUND_HUE), rng.uniform(*GROUND_SATURATION), rng.uniform(*GROUND_VALUE))
              for _ in range(2)]
    seed = int(rng.integers(0, 1 << 24))
    cells = float(2.0 ** rng.uniform(np.log2(GROUND_CELLS_PER_M[0]), np.log2(GROUND_CELLS_PER_M[1])))
    return dict(cloth_rgb=np.array(cloth, np.float32), ground_rgb=np.array(ground, np.float32), ground_seed=seed,
                ground_cells_per_m=float(np.float32(cells)), ground_octaves=GROUND_OCTAVES)


def key_of(mode, seed, task, timestep):
    """The key of an observation: (seed, task index, timestep) with "observation" -- a fresh draw at every observation, as
    the reference draws at every render_cloth() -- and (seed, task index, 0) with "episode"."""
    if mode not in MODES:
        raise ValueError(f"randomize_appearance: {mode!r} is none of {MODES}")
    return (int(seed), int(task), int(timestep) if mode == "observation" else 0)


def as_row(a):
    """float32 [12]: cloth_rgb, ground_rgb[0], ground_rgb[1], seed, cells_per_m, octaves -- the record's 'appearance' row."""
    return np.array([*np.asarray(a["cloth_rgb"], np.float32), *np.asarray(a["ground_rgb"], np.float32).ravel(),
                     a["ground_seed"], a["ground_cells_per_m"], a["ground_octaves"]], np.float32)


def to_struct(a):
    from .sim import Appearance
    s = Appearance()
    cloth, ground = np.asarray(a["cloth_rgb"], np.float32).reshape(3), np.asarray(a["ground_rgb"], np.float32).reshape(2, 3)
    for k in range(3):
        s.cloth_rgb[k] = cloth[k]
        s.ground_rgb[0][k], s.ground_rgb[1][k] = ground[0, k], ground[1, k]
    s.ground_seed = int(a.get("ground_seed", 0)) & 0xFFFFFFFF
    s.ground_cells_per_m = float(a.get("ground_cells_per_m", 0.0))
    s.ground_octaves = int(a.get("ground_octaves", 0))
    return s


def from_struct(s):
    return dict(cloth_rgb=np.array(list(s.cloth_rgb), np.float32),
                ground_rgb=np.array([list(s.ground_rgb[0]), list(s.ground_rgb[1])], np.float32),
                ground_seed=int(s.ground_seed), ground_cells_per_m=float(s.ground_cells_per_m),
                ground_octaves=int(s.ground_octaves))


def check(a):
    """fs_appearance_check (no GPU needed): raises ValueError with the library's message for a value the setter refuses."""
    import ctypes as C

    from .sim import load_library
    lib = load_library()
    if lib.fs_appearance_check(C.byref(to_struct(a))) != 0:
        raise ValueError(lib.fs_last_error().decode())


def host_ground_texture(a, hx, hz):
    """fs_host_ground_texture (no GPU needed): the kernels' texture function, compiled for the host, at float32 points."""
    import ctypes as C

    from .sim import load_library
    lib = load_library()
    hx, hz = (np.ascontiguousarray(np.asarray(v, np.float32).ravel()) for v in (hx, hz))
    assert hx.size == hz.size
    t = np.empty(hx.size, np.float32)
    fp = lambda v: v.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    if lib.fs_host_ground_texture(C.byref(to_struct(a)), int(hx.size), fp(hx), fp(hz), fp(t)) != 0:
        raise ValueError(lib.fs_last_error().decode())
    return t


def equal(a, b):
    return bool(np.array_equal(as_row(a), as_row(b)) and int(a["ground_seed"]) == int(b["ground_seed"]))
