"""Packed mesh words of the host scene builder (fs_scene.h build_mesh_words; FS_SCENE_MESH_WORDS / FS_SCENE_MESH_STIFFNESS):
a cloth without one-byte stream codes gets two words per spring slot -- j | stiffness index << 30, bits of the rest length --
which decode to exactly the particle's CSR row in slot order; a coded cloth gets none.  No GPU."""
import numpy as np
import pytest

import shirt_meshes

STIFF = (0.9, 0.7, 0.5)   # stretch / bend / shear: three distinct bit patterns


def _scene_params(dimx=-1, dimz=-1):
    return np.array([0, 0.15, 0, dimx, dimz, *STIFF, 2, 0, 2, 0, np.pi / 2, -np.pi / 2, 0, 720, 720, 0.5, 0], np.float32)


def _mesh_scene(obj_text, tmp_path):
    from flingbot_amd import sim as fsim, tasks as ftasks

    path = tmp_path / "shirt_processed.obj"
    path.write_text(obj_text)
    verts, faces, stretch, bend, shear = ftasks.load_cloth(str(path))
    return fsim.host_scene(_scene_params(), verts.reshape(-1), stretch.reshape(-1), bend.reshape(-1), shear.reshape(-1),
                           faces.reshape(-1))


def _csr_rows(h):
    """Per particle: (neighbour ids, rest-length bits, stiffness bits) in ascending spring id, rebuilt from the spring list."""
    n, springs = h["n"], h["springs"].reshape(-1, 2)
    len_bits, k_bits = h["spring_lengths"].view(np.uint32), h["spring_stiffness"].view(np.uint32)
    rows = [([], [], []) for _ in range(n)]
    for e, (a, b) in enumerate(springs):
        for i, j in ((a, b), (b, a)):
            rows[i][0].append(int(j))
            rows[i][1].append(int(len_bits[e]))
            rows[i][2].append(int(k_bits[e]))
    return rows


@pytest.mark.parametrize("shirt", ["shirt_a", "shirt_b"])
def test_mesh_words_decode_to_the_csr_rows(shirt, tmp_path):
    h = _mesh_scene(getattr(shirt_meshes, shirt)(), tmp_path)
    n, deg = h["n"], h["max_deg"]
    assert not (h["stream_dict"] != 0xffffffff).any()                  # vertices numbered at random: no stream codes
    assert h["mesh_ok"] == 1
    words, stiff = h["mesh_words"], h["mesh_stiffness"].view(np.uint32)
    assert words.shape == (deg, n, 2) and words.dtype == np.uint32 and stiff.shape == (4,)
    # the stiffness table: the distinct bit patterns in order of first use by spring id, the rest zero
    k_bits = h["spring_stiffness"].view(np.uint32)
    first_use = [int(k_bits[i]) for i in sorted(np.unique(k_bits, return_index=True)[1])]
    assert len(first_use) == 3 and stiff.tolist() == first_use + [0] * (4 - len(first_use))
    off, adj = h["adj_offsets"], h["adj_neighbors"]
    rows = _csr_rows(h)
    for i in range(n):
        nbr, length, k = rows[i]
        d = len(nbr)
        assert d == off[i + 1] - off[i] and nbr == adj[off[i]:off[i + 1]].tolist()      # (the builder's own CSR agrees)
        w0, w1 = words[:d, i, 0], words[:d, i, 1]
        assert (w0 & 0x3fffffff).tolist() == nbr, i
        assert w1.tolist() == length, i
        assert stiff[w0 >> 30].tolist() == k, i
        assert (words[d:, i, 0] == 0xffffffff).all() and (words[d:, i, 1] == 0).all(), i   # empty slots beyond the row
    assert max(len(r[0]) for r in rows) == deg


def test_coded_grid_has_no_mesh_words():
    from flingbot_amd import sim as fsim

    h = fsim.host_scene(_scene_params(8, 9))
    assert h["n"] == 72 and (h["stream_dict"] != 0xffffffff).any()      # a grid has stream codes ...
    assert h["mesh_ok"] == 0 and h["mesh_words"].size == 0 and h["mesh_stiffness"].size == 0   # ... and needs no words
    assert len(np.unique(h["spring_stiffness"].view(np.uint32))) == 3
