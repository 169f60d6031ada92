"""Synthetic scenes of the rasteriser tests (tests/test_raster_reference_cpu.py, tests/test_raster_synthetic_gpu.py).

Every scene is small, seeded and fixed: a grid cloth from cloth_params(dimx, dimz) whose particles are placed with
set_positions, an optional set of picker spheres, a camera.  install() drives a duck-typed sim (oracle.OracleSim or
flingbot_amd.sim.EnvView); reference() renders the scene with tests/raster_reference.py once and keeps the result.

`colour` says whether a test may compare colours on the scene: only where surfaces that shadow each other are at least 0.05 m
apart along the light (about 230 steps of the shadow map's 24-bit depth), or coincide, so that every PCF compare is far from
its threshold whatever the last bit of a float32 says.  `why` notes it per scene.
"""
import functools

import numpy as np

import raster_reference as rr
from scenarios import cloth_params

TOP_DOWN = (np.pi / 2, -np.pi / 2, 0.0)  # FlingBot's camera angles: looking straight down, +x -> -y_ndc, +z -> -x_ndc
SCENE_POS = (0.0, -0.2, 0.0)


class Scene:
    def __init__(self, name, dimx, dimz, pos, W, H, cam_pos=(0.0, 2.0, 0.0), cam_angle=TOP_DOWN, spheres=(), colour=True,
                 why=""):
        self.name, self.dimx, self.dimz = name, dimx, dimz
        self.pos = np.ascontiguousarray(pos, np.float32).reshape(dimx * dimz, 4)
        self.W, self.H, self.cam_pos, self.cam_angle = W, H, tuple(cam_pos), tuple(cam_angle)
        self.spheres = tuple(spheres)  # (radius, current xyz, previous xyz)
        self.colour, self.why = colour, why

    def at(self, W, H):
        """The same scene at another frame size."""
        return Scene(f"{self.name}@{W}x{H}", self.dimx, self.dimz, self.pos, W, H, self.cam_pos, self.cam_angle, self.spheres,
                     self.colour, self.why)

    def __repr__(self):
        return self.name


def install(sim, sc):
    """Put scene `sc` into `sim`; sets the camera where the sim has one (the oracle has none)."""
    sim.set_scene(cloth_params(sc.dimx, sc.dimz, pos=SCENE_POS))
    p = sc.pos.copy()
    p[:, 3] = sim.get_positions().reshape(-1, 4)[:, 3]
    sim.set_positions(p.ravel())
    if hasattr(sim, "clear_shapes"):
        sim.clear_shapes()
    for radius, cur, _ in sc.spheres:
        sim.add_sphere(radius, list(cur), [1, 0, 0, 0])
    if sc.spheres:
        st = np.array(sim.get_shape_states(), np.float32).reshape(-1, 14).copy()
        for q, (_, _, prev) in enumerate(sc.spheres):
            st[q, 3:6] = prev
        sim.set_shape_states(st.ravel())
    if hasattr(sim, "set_camera_params"):
        sim.set_camera_params([*sc.cam_pos, *sc.cam_angle, sc.W, sc.H])


def frame_of(sc, lower, upper):
    """The reference's Frame of the scene: matrices from fs_camera_matrices (host code, pinned to the reference's maths.h by
    tests/test_oracle_cpu.py)."""
    from flingbot_amd import sim as fsim

    m = fsim.camera_matrices(sc.cam_pos, sc.cam_angle, sc.W, sc.H, lower, upper)
    return rr.Frame(m["view"], m["proj"], m["light"], m["lightdir"], sc.cam_pos, sc.W, sc.H), m


@functools.lru_cache(maxsize=None)
def _oracle_side(sc):
    from oracle import OracleSim
    from oracle.render import sphere_mesh

    orc = OracleSim()
    install(orc, sc)
    lo, up = orc.get_scene_bounds()
    faces = np.array(orc.get_faces(), np.int32).reshape(-1, 3)
    radii = [s[0] for s in sc.spheres]
    mesh = sphere_mesh(orc.get_shape_states(), radii) if sc.spheres else (None, None, None)
    return orc, lo, up, faces, mesh


@functools.lru_cache(maxsize=None)
def reference(sc, want_color=True):
    """The reference's render of the scene (computed once per scene and process): dict of raster_reference.render plus
    frame, mats (fs_camera_matrices' dict), faces, sphere mesh."""
    orc, lo, up, faces, mesh = _oracle_side(sc)
    fr, mats = frame_of(sc, lo, up)
    out = rr.render(fr, sc.pos, faces, *mesh, want_color=want_color)
    out.update(frame=fr, mats=mats, faces=faces, mesh=mesh, lower=lo, upper=up)
    return out


# ------------------------------------------------------------------------------------------------ scene builders
def _grid(dimx, dimz, spacing, x0=0.0, z0=0.0):
    ix, iz = np.meshgrid(np.arange(dimx), np.arange(dimz))  # particle = iz * dimx + ix
    return (ix.ravel() - (dimx - 1) / 2) * spacing + x0, (iz.ravel() - (dimz - 1) / 2) * spacing + z0


def _pack(x, y, z):
    p = np.ones((len(x), 4), np.float32)
    p[:, 0], p[:, 1], p[:, 2] = x, y, z
    return p


def _unproject(vp, W, H, fx, fy, h):
    """float64 world (x, z) at height h whose window coordinates are (fx, fy) under the row-major matrix vp."""
    vp = np.asarray(vp, np.float64)
    nx, ny = 2 * fx / W - 1, 2 * fy / H - 1
    r0, r1 = vp[0] - nx * vp[3], vp[1] - ny * vp[3]
    A = np.array([[r0[0], r0[2]], [r1[0], r1[2]]])
    b = -np.array([r0[1] * h + r0[3], r1[1] * h + r1[3]])
    return np.linalg.solve(A, b)


def lattice(shift_half):
    """Flat 9 x 9 cloth at y = 0.3 whose SNAPPED window coordinates are 28 + 5 i, 12 + 5 j (+ 1/2: on pixel centres; with
    shift_half on pixel corners, so that no centre lies on an edge) at 96 x 64.  float64 inverse projection, then the float32
    neighbours are walked until the float32 vertex stage lands on the target."""
    W, H, h, k = 96, 64, np.float32(0.3), 5
    sc = Scene("tmp", 9, 9, np.zeros((81, 4)), W, H)
    _, lo, up, _, _ = _oracle_side(sc)
    fr, _ = frame_of(sc, lo, up)
    off = 0.0 if shift_half else 0.5
    pos = np.zeros((81, 4), np.float32)
    for iz in range(9):
        for ix in range(9):
            # top-down camera: window x runs against world z, window y against world x
            tx, ty = 28 + k * (8 - iz) + off, 12 + k * (8 - ix) + off
            x, z = (np.float32(v) for v in _unproject(fr.vp, W, H, tx, ty, float(h)))
            for _ in range(64):
                vs = rr.vertex_stage(fr.vp, W, H, np.array([[x, h, z]], np.float32))
                ex, ey = int(vs["X"][0]) - int(round(tx * 256)), int(vs["Y"][0]) - int(round(ty * 256))
                if ex == 0 and ey == 0:
                    break
                if ex:
                    z = np.nextafter(z, np.float32(np.inf if ex > 0 else -np.inf))
                if ey:
                    x = np.nextafter(x, np.float32(np.inf if ey > 0 else -np.inf))
            else:
                raise AssertionError("lattice vertex did not land on its target")
            pos[iz * 9 + ix] = (x, h, z, 1.0)
    return Scene("lattice_corners" if shift_half else "lattice_centres", 9, 9, pos, W, H,
                 why="one flat layer 0.3 m above the ground")


def tilted_fold(W=96, H=64):
    """12 x 12 mesh on a tilted plane (heights 0.2 .. 0.5), jittered in the plane; the four columns of lowest x are folded
    back over the next four onto a parallel plane 0.11 m above, so front and back faces both show.  The strip that joins the layers leans
    outwards under the upper layer and faces away from the light, so no visible point has an occluder nearer than 0.1 m."""
    rng = np.random.RandomState(1234)
    gx, gz = _grid(12, 12, 0.05)
    ix = np.tile(np.arange(12), 12)
    folded = ix <= 3
    gx4, gx3 = (4 - 5.5) * 0.05, (3 - 5.5) * 0.05
    x = np.where(folded, gx4 - 0.015 + (gx3 - gx), gx) + rng.uniform(-0.006, 0.006, 144)
    z = gz + rng.uniform(-0.006, 0.006, 144)
    y = 0.285 + 0.2 * x + 0.1 * z + np.where(folded, 0.11, 0.0)  # each layer is one plane: jitter moves particles within it
    return Scene("tilted_fold", 12, 12, _pack(x, y, z), W, H, why="layers 0.11 m apart, 0.19 m or more above the ground")


def borders_and_planes():
    """A 4.4 m mesh under a camera raised to y = 3.5: it overhangs all four borders, its outer cells lie wholly outside, the
    ground (3.5 m away) is beyond the far plane (3 m), and so is the part of the mesh with z > 1.2 (y < 0.5): discarded per
    pixel.  One vertex is lifted behind the camera (y = 3.6): its six triangles are dropped whole."""
    rng = np.random.RandomState(99)
    gx, gz = _grid(12, 12, 0.4, x0=0.2)
    x = gx + rng.uniform(-0.05, 0.05, 144)
    z = gz + rng.uniform(-0.05, 0.05, 144)
    y = 0.62 - 0.1 * z
    y[2 * 12 + 2] = 3.6  # particle (ix 2, iz 2) at x = -1.2, z = -1.4: its cone's shadow falls out of the frame
    return Scene("borders_and_planes", 12, 12, _pack(x, y, z), 96, 64, cam_pos=(0.0, 3.5, 0.0),
                 why="one layer; the ground is never seen; the lifted cone's shadow falls on dropped triangles or outside")


def ties_and_degenerates():
    """10 x 12 grid: rows 0-4 a tilted plane; rows 5-9 the same particles in reverse row order (bit-identical positions: a
    second layer of the same surface with the other quad diagonal, depth ties nearly everywhere -> the lower id must win; the
    strip between rows 4 and 5 has zero area); row 10 = row 0 moved 1 mm outwards (a sliver 0.05 pixel wide that covers no
    centre), row 11 = row 10 (zero area again)."""
    ix, iz = np.meshgrid(np.arange(10), np.arange(5))
    x = ((ix - 4.5) * 0.05).astype(np.float32)
    z = ((iz - 2.0) * 0.05 + 0.004).astype(np.float32)
    y = (0.3 + 0.3 * x + 0.2 * z).astype(np.float32)
    rows = [np.stack([x[r], y[r], z[r]], 1) for r in range(5)]
    order = [0, 1, 2, 3, 4, 4, 3, 2, 1, 0]
    layers = [rows[r] for r in order]
    sliver = rows[0].copy()
    sliver[:, 2] -= np.float32(0.001)
    p = np.concatenate(layers + [sliver, sliver]).astype(np.float32)
    return Scene("ties_and_degenerates", 10, 12, _pack(p[:, 0], p[:, 1], p[:, 2]), 96, 64,
                 why="coincident layers: every compare is decided by the polygon offset (8 steps or more)")


def ground_coplanar():
    """A 6 x 6 cloth lying exactly in the ground plane y = 0."""
    gx, gz = _grid(6, 6, 0.08)
    return Scene("ground_coplanar", 6, 6, _pack(gx, np.zeros(36), gz), 96, 64,
                 why="cloth and ground coincide: decided by the polygon offset")


def pickers():
    """8 x 8 tilted cloth at y ~ 0.3 and four spheres drawn at their PREVIOUS position (the current one is elsewhere): one
    half outside the frame, one under the cloth's edge (partly hidden, 0.07 m below it), one sunk into the ground, and one
    around the camera: all its triangles face away (culled: it must not show; without culling it would fill the frame)."""
    gx, gz = _grid(8, 8, 0.06)
    y = 0.3 + 0.1 * gx
    sph = ((0.06, (0.0, 1.0, 0.0), (0.1, 0.35, -0.8)),     # window x ~ 48 + 0.8 / 0.0215: crosses the right border
           (0.05, (0.3, 1.0, 0.3), (0.05, 0.16, 0.24)),    # top at 0.21, the cloth above it at ~0.3; peeks out past z = 0.21
           (0.08, (-0.3, 1.0, -0.3), (-0.4, 0.03, -0.2)),  # centre 0.03 above the ground: more than half of it is below
           (0.08, (0.3, 1.0, -0.3), (0.0, 1.97, 0.0)))     # the camera (0, 2, 0) is inside it
    return Scene("pickers", 8, 8, _pack(gx, y, gz), 96, 64, spheres=sph, colour=False,
                 why="the sunk sphere meets the ground: occluder distances go to 0 along the contact circle")


def sphere_tie():
    """A 3 x 3 cloth whose particles sit exactly on nine vertices of a picker's mesh, cell diagonals along the mesh's: its
    eight triangles coincide with eight sphere triangles vertex for vertex, every depth ties, and the sphere -- drawn first,
    lower ids -- must keep all of those pixels (grey where the cloth would be pink)."""
    from oracle.render import sphere_mesh

    radius, centre = 0.3, (0.0, 0.4, 0.0)
    st = np.array([[1.0, 1.0, 1.0, *centre, 1, 0, 0, 0, 1, 0, 0, 0]], np.float32)
    verts = sphere_mesh(st, [radius])[0].reshape(21, 21, 4)  # [slice i, segment j]
    i0 = 2 if verts[2, 0, 1] > verts[18, 0, 1] else 16        # three rings near the pole that looks at the camera
    pos = np.ones((9, 4), np.float32)
    for iz in range(3):
        for ix in range(3):
            pos[iz * 3 + ix, :3] = verts[i0 + ix, 7 - iz, :3]  # sphere quads split from (i - 1, j) to (i, j - 1)
    return Scene("sphere_tie", 3, 3, pos, 96, 64, spheres=((radius, (1.0, 1.0, 1.0), centre),), colour=False,
                 why="cloth and sphere coincide; the sphere shadows itself along its terminator")


def tent():
    """A 3 x 3 cloth, 0.5 m wide, whose centre particle is pulled up to y = 1.2: clip w runs from 0.8 at the apex to 1.8 at the
    rim inside every triangle and the vertex normals differ, so affine weights instead of perspective-correct ones (or a
    wrong vertex order after the orientation swap) change the shading visibly.  It stands 20 m from the origin, camera above
    it: outside the light's map, where the shader takes no PCF sample at all (shadow term 1, attenuation at its floor), so
    no compare can sit near its threshold on the steep faces."""
    gx, gz = _grid(3, 3, 0.25, x0=20.03, z0=-0.02)
    y = np.full(9, 0.2)
    y[4] = 1.2
    return Scene("tent", 3, 3, _pack(gx, y, gz), 96, 64, cam_pos=(20.0, 2.0, 0.0), why="outside the shadow map: no PCF compare")


@functools.lru_cache(maxsize=None)
def all_scenes():
    fold = tilted_fold()
    return (lattice(False), lattice(True), fold, fold.at(64, 96), fold.at(33, 17), fold.at(16, 16), fold.at(1, 1),
            borders_and_planes(), ties_and_degenerates(), ground_coplanar(), pickers(), sphere_tie(), tent())


def fold_720():
    return tilted_fold(720, 720)


# ------------------------------------------------------------------------------------------------ vertex normals
def normals_input(name):
    """(dimx, dimz, positions) of the three inputs of the normals tests: the folded mesh (opposing triangles meet along the
    fold), a cloth whose particles all coincide (every sum vanishes: (0, 1, 0)), a 17 x 16 grid (272 particles: the second
    256-thread block is partly filled)."""
    if name == "tilted_fold":
        return 12, 12, tilted_fold().pos
    if name == "coincident":
        return 6, 6, np.tile(np.array([[0.1, 0.3, -0.2, 1.0]], np.float32), (36, 1))
    rng = np.random.RandomState(7)
    x, z = _grid(17, 16, 0.02)
    return 17, 16, _pack(x, 0.2 + rng.uniform(0, 0.05, 272), z)


def check_normals(got, pos, faces):
    """|dn| <= 4 2^-24 sum_t |a_t| |b_t| / |sum_t a_t x b_t| + 2^-22 per component (raster_reference.vertex_normals64);
    (0, 1, 0) where the float64 sum vanishes exactly."""
    ref, bound = rr.vertex_normals64(pos, faces)
    assert (got[:, 3] == 0).all()
    err = np.abs(got[:, :3].astype(np.float64) - ref).max(1)
    finite = np.isfinite(bound)
    print("normals: max error / bound", (err[finite] / bound[finite]).max(initial=0), "max error", err.max())
    assert (err[finite] <= bound[finite]).all(), (err[finite] / bound[finite]).max()
    assert np.array_equal(got[~finite, :3], np.tile(np.array([0, 1, 0], np.float32), ((~finite).sum(), 1)))
    return err, bound
