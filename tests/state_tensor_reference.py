"""The packed layout of fs_state_gather / FlingSim.state_tensors (include/flingsim.h), stated in numpy: what the GPU tests
compare the gathered tensors with, and what the CPU tests check ParticleState's views against.

Row k of a packed array holds episode k's particles 0 .. N_k-1 exactly as the per-episode getters return them, rows
N_k .. n_max-1 are zeros.  Comparisons are made on the uint32 views, so -0.0, NaN payloads and denormals count."""
import numpy as np


def pack_rows(rows, n_max=None, dtype=np.float32):
    """rows: one [N_k, ...] array per listed episode -> (packed [n, n_max, ...] zero-padded, counts int32 [n])."""
    rows = [np.asarray(r, dtype) for r in rows]
    counts = np.array([r.shape[0] for r in rows], np.int32)
    n_max = int(counts.max()) if n_max is None else int(n_max)
    if n_max < int(counts.max()):
        raise ValueError("n_max below the largest count")
    out = np.zeros((len(rows), n_max) + rows[0].shape[1:], dtype)
    for k, r in enumerate(rows):
        out[k, :r.shape[0]] = r
    return out, counts


def pack_from_getters(sim, envs, n_max=None):
    """The per-episode getters of `sim` (FlingSim or anything with its method names) for the listed episodes, packed:
    dict(pos4 [n, n_max, 4], vel3 [n, n_max, 3] -- the getter drops the fourth lane --, phase [n, n_max], counts [n])."""
    pos, counts = pack_rows([sim.get_positions(e).reshape(-1, 4) for e in envs], n_max)
    vel, _ = pack_rows([sim.get_velocities(e).reshape(-1, 3) for e in envs], n_max)
    phase, _ = pack_rows([sim.get_phases(e).reshape(-1) for e in envs], n_max, np.int32)
    return dict(pos4=pos, vel3=vel, phase=phase, counts=counts)


def mask(counts, n_max):
    """bool [n, n_max]: True for rows below the episode's count."""
    return np.arange(int(n_max))[None, :] < np.asarray(counts)[:, None]


def bits(a):
    """The uint32 view of a float32 / int32 array (contiguous copy when needed)."""
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4, a.dtype
    return a.view(np.uint32)
