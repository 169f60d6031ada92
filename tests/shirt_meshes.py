"""Synthetic quad-mesh shirts as OBJ text (test helper; the project's own meshes, not CLOTH3D data).

The outline is a T on a square lattice of 6.25 mm edges: a body of body_w x body_h quads with a sleeve of sleeve_w x sleeve_h
quads on either side of its top.  The mesh lies in the xz-plane (y is up), which is how the task generator drops it.

    shirt_a()   two such layers 5 mm apart, joined along the side seams, the undersides of the sleeves and the shoulders
                (seam vertices are shared by both layers and sit half way between them), open at the hem, the cuffs and the
                neck.  Most vertices have more than 16 others within the solver's rest-pose filter radius (their own layer's
                eight plus the nine opposite), so the host cannot pack the filter sets and the kernels test rest positions.
                The four armpit / sleeve-end seam corners are interior vertices of valence 6.
    shirt_b()   one layer of the same outline; its filter sets are the in-layer neighbours and pack.  One lattice edge in the
                middle of the body is rotated (the two quads on it are re-cut along the other diagonal of their hexagon, the
                edge's end points pulled apart so that no quad is degenerate): two interior vertices of valence 3, two of 5.

Faces are written in shuffled order and vertices are numbered by a random permutation (both seeded), so that nothing that
holds for a row-major grid holds here.
"""
import numpy as np

EDGE = 0.00625
GAP = 0.005


def _outline_quads(body_w, body_h, sleeve_w, sleeve_h):
    """Lattice cells (i, j) of the T: body columns 0 .. body_w-1, sleeves to the left and right of its top sleeve_h rows."""
    cells = [(i, j) for j in range(body_h) for i in range(body_w)]
    for j in range(body_h - sleeve_h, body_h):
        cells += [(i, j) for i in range(-sleeve_w, 0)] + [(i, j) for i in range(body_w, body_w + sleeve_w)]
    return cells


def _seam(i, j, body_w, body_h, sleeve_w, sleeve_h, neck):
    """Is lattice point (i, j) on a seam (shared by both layers)?  Side seams, sleeve undersides, shoulders without the neck."""
    arm = body_h - sleeve_h
    if i in (0, body_w) and j <= arm and j > 0:           # side seams (the hem corner itself stays open)
        return True
    if j == arm and (-sleeve_w < i <= 0 or body_w <= i < body_w + sleeve_w):   # sleeve undersides (cuff corners open)
        return True
    lo, hi = (body_w - neck) // 2, (body_w - neck) // 2 + neck
    if j == body_h and (-sleeve_w < i <= lo or hi <= i < body_w + sleeve_w):   # shoulders, neck lo .. hi open
        return True
    return False


def _obj_text(points, quads, seed, comment):
    rng = np.random.RandomState(seed)
    number = rng.permutation(len(points))                 # new id of vertex k
    placed = [None] * len(points)
    for k, p in enumerate(points):
        placed[number[k]] = p
    lines = ["# " + comment]
    lines += ["v %.6f %.6f %.6f" % tuple(p) for p in placed]
    for q in rng.permutation(len(quads)):
        lines.append("f " + " ".join(str(int(number[v]) + 1) for v in quads[q]))
    return "\n".join(lines) + "\n"


def shirt_a(body_w=12, body_h=16, sleeve_w=5, sleeve_h=5, neck=4, seed=7):
    cells = _outline_quads(body_w, body_h, sleeve_w, sleeve_h)
    ids, points, quads = {}, [], []

    def vertex(i, j, layer):
        seam = _seam(i, j, body_w, body_h, sleeve_w, sleeve_h, neck)
        key = (i, j, -1 if seam else layer)
        if key not in ids:
            ids[key] = len(points)
            points.append((i * EDGE, GAP / 2 if seam else layer * GAP, j * EDGE))
        return ids[key]

    for layer in (1, 0):
        for i, j in cells:
            ring = [vertex(i, j, layer), vertex(i, j + 1, layer), vertex(i + 1, j + 1, layer), vertex(i + 1, j, layer)]
            quads.append(ring if layer == 1 else ring[::-1])   # normals point out of the garment
    return _obj_text(points, quads, seed, "synthetic two-layer quad-mesh shirt (tests/shirt_meshes.py)")


def shirt_b(body_w=12, body_h=16, sleeve_w=5, sleeve_h=5, seed=11):
    cells = _outline_quads(body_w, body_h, sleeve_w, sleeve_h)
    ci, cj = body_w // 2, body_h // 2                     # the rotated edge: (ci, cj) - (ci, cj + 1), between cells (ci-1, cj), (ci, cj)
    ids, points, quads = {}, [], []

    def vertex(i, j):
        if (i, j) not in ids:
            ids[(i, j)] = len(points)
            dz = -0.3 if (i, j) == (ci, cj) else 0.3 if (i, j) == (ci, cj + 1) else 0.0
            points.append((i * EDGE, 0.0, (j + dz) * EDGE))
        return ids[(i, j)]

    for i, j in cells:
        if (i, j) in ((ci - 1, cj), (ci, cj)):
            continue
        quads.append([vertex(i, j), vertex(i, j + 1), vertex(i + 1, j + 1), vertex(i + 1, j)])
    # hexagon p a r s b q of the two cells left out (a - b was their common edge); re-cut along p - s
    p, a, r = vertex(ci - 1, cj), vertex(ci, cj), vertex(ci + 1, cj)
    s, b, q = vertex(ci + 1, cj + 1), vertex(ci, cj + 1), vertex(ci - 1, cj + 1)
    quads += [[p, s, r, a], [p, q, b, s]]
    return _obj_text(points, quads, seed, "synthetic one-layer quad-mesh shirt (tests/shirt_meshes.py)")


def parse(obj_text):
    """(vertices float64 [V, 3], quads int [F, 4]) of OBJ text written here."""
    verts = [[float(t) for t in ln.split()[1:]] for ln in obj_text.splitlines() if ln.startswith("v ")]
    quads = [[int(t.split("/")[0]) - 1 for t in ln.split()[1:]] for ln in obj_text.splitlines() if ln.startswith("f ")]
    return np.array(verts), np.array(quads)


def valences(obj_text):
    """(valence per vertex, is-interior per vertex): an interior vertex has as many quads around it as lattice edges."""
    v, q = parse(obj_text)
    edges = set()
    fan = np.zeros(len(v), int)
    for f in q:
        fan[f] += 1
        for k in range(4):
            edges.add((min(f[k], f[(k + 1) % 4]), max(f[k], f[(k + 1) % 4])))
    val = np.zeros(len(v), int)
    for a, b in edges:
        val[a] += 1
        val[b] += 1
    return val, val == fan
