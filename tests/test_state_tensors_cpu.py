"""fs_state_gather / fs_state_scatter and their Python face without a GPU: the header and the library agree, the entry points
refuse null arguments before they touch anything, FlingSim.state_tensors / set_state_tensors refuse a tensor that does not fit
BEFORE the library is called (the library handle is a stub that fails the test when a state call reaches it), and
ParticleState's views are the numpy statement of the layout (tests/state_tensor_reference.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import state_tensor_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS_ERR_ARG = -1


# ---- header and library -------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_both_context_calls():
    from flingbot_amd import build, sim as fsim

    with open(os.path.join(ROOT, "include", "flingsim.h")) as fh:
        header = fh.read()
    gather = re.search(r"^int fs_state_gather\(fs_ctx \*ctx, int n, const int \*envs, int n_max,\s*float \*d_pos4, "
                       r"float \*d_vel4, int \*d_phase, int \*counts\);", header, re.M)
    scatter = re.search(r"^int fs_state_scatter\(fs_ctx \*ctx, int n, const int \*envs, int n_max,\s*const float \*d_pos4, "
                        r"const float \*d_vel4\);", header, re.M)
    assert gather and scatter
    for m in (gather, scatter):   # context calls: no stream argument (tests/test_guarded_calls_cpu.py keys on it)
        assert not re.search(r"void \*stream\)\s*;$", m.group(0))
    rule = header[header.index("particle state as batched device tensors"):scatter.end()]
    for text in ("[n][n_max][4]", "inverse mass", "ZEROS", "counts[k] = N_k", "RETURNS WHEN ITS LAUNCH HAS FINISHED",
                 "event", "n_max below the largest N_k", "listed twice", "stored as 0", "not read", "FS_ERR_STATE"):
        assert text in rule, text
    lib = fsim.load_library()
    for name in ("fs_state_gather", "fs_state_scatter"):
        assert getattr(lib, name) is not None and name in lib._fs_symbols
    assert "fs_state.hip" in build.LIB_SOURCES and os.path.exists(os.path.join(build.CSRC, "fs_state.hip"))


def test_entry_points_refuse_null_arguments():
    """FS_ERR_ARG with the reason, before the context is read or a HIP call is made: `ctx` below is host memory that is not a
    context, the field pointers are host addresses, and none of them is dereferenced."""
    from flingbot_amd import sim as fsim

    lib = fsim.load_library()
    not_a_ctx = np.zeros(1 << 16, np.uint8)
    ctx = C.c_void_p(not_a_ctx.ctypes.data)
    ids, counts = np.zeros(2, np.int32), np.zeros(2, np.int32)
    field = np.zeros(64, np.float32)
    p = C.c_void_p(field.ctypes.data)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))   # noqa: E731
    err = lambda: lib.fs_last_error().decode()   # noqa: E731
    assert lib.fs_state_gather(None, 2, ip(ids), 4, p, p, None, ip(counts)) == FS_ERR_ARG and "null context" in err()
    assert lib.fs_state_gather(ctx, 2, None, 4, p, p, None, ip(counts)) == FS_ERR_ARG and "null list" in err()
    assert lib.fs_state_gather(ctx, 0, ip(ids), 4, p, p, None, ip(counts)) == FS_ERR_ARG and "n < 1" in err()
    assert lib.fs_state_gather(ctx, 2, ip(ids), 4, None, None, None, ip(counts)) == FS_ERR_ARG and "all null" in err()
    assert lib.fs_state_scatter(None, 2, ip(ids), 4, p, p) == FS_ERR_ARG and "null context" in err()
    assert lib.fs_state_scatter(ctx, 2, None, 4, p, p) == FS_ERR_ARG and "null list" in err()
    assert lib.fs_state_scatter(ctx, 2, ip(ids), 4, None, None) == FS_ERR_ARG and "both null" in err()
    assert not not_a_ctx.any() and not counts.any()


# ---- the Python-side checks -----------------------------------------------------------------------------------------------------
class StubLibrary:
    """Stands in for the ctypes handle: answers the host-side particle count, and fails the test when anything else is asked of
    it -- so a check that passes its bad argument on to the library is seen."""

    def __init__(self, counts):
        self.counts = dict(counts)

    def fs_n_particles(self, handle, env):
        return self.counts[int(env)]

    def __getattr__(self, name):
        pytest.fail(f"the library was reached: {name}")


def _stub_sim(counts):
    from flingbot_amd import sim as fsim

    s = fsim.FlingSim.__new__(fsim.FlingSim)   # no context: every check under test comes before the first library call
    s.lib, s.h, s.n_envs, s.device = StubLibrary(counts), None, len(counts), 0
    return s


COUNTS = {0: 15, 1: 64, 2: 63}


def _out(n=3, n_max=64, **over):
    from flingbot_amd import sim as fsim

    t = dict(pos4=torch.zeros(n, n_max, 4), vel4=torch.zeros(n, n_max, 4), phase=torch.zeros(n, n_max, dtype=torch.int32))
    t.update(over)
    return fsim.ParticleState(t["pos4"], t["vel4"], t["phase"], None)


@pytest.mark.parametrize("case, field, out, message", [
    ("dtype", "pos4", lambda: _out(pos4=torch.zeros(3, 64, 4, dtype=torch.float64)), "out.pos4: dtype"),
    ("dtype of the phases", "phase", lambda: _out(phase=torch.zeros(3, 64, dtype=torch.int64)), "out.phase: dtype"),
    ("rows", "vel4", lambda: _out(vel4=torch.zeros(2, 64, 4)), "out.vel4: shape"),
    ("n_max", "pos4", lambda: _out(pos4=torch.zeros(3, 65, 4)), "out.pos4: shape"),
    ("three lanes", "pos4", lambda: _out(pos4=torch.zeros(3, 64, 3)), "out.pos4: shape"),
    ("not contiguous", "vel4", lambda: _out(vel4=torch.zeros(3, 64, 8)[..., ::2]), "out.vel4: the tensor is not contiguous"),
    ("transposed", "phase", lambda: _out(phase=torch.zeros(64, 3, dtype=torch.int32).t()), "out.phase: the tensor is not contiguous"),
    ("on the host", "pos4", lambda: _out(), "out.pos4: the tensor lives on cpu"),
    ("on the host, phases", "phase", lambda: _out(), "out.phase: the tensor lives on cpu"),
    ("missing", "vel4", lambda: _out(vel4=None), "out.vel4: a torch tensor is needed"),
])
def test_state_tensors_refuses_an_out_that_does_not_fit(case, field, out, message):
    """One field asked for per case (this machine has no device, so a tensor that fits in every other respect still lives on
    the host: the device is the last thing checked)."""
    s = _stub_sim(COUNTS)
    with pytest.raises(ValueError, match=re.escape(message)):
        s.state_tensors([0, 1, 2], positions=field == "pos4", velocities=field == "vel4", phases=field == "phase", out=out())


def test_state_tensors_refuses_a_small_n_max_and_an_empty_request():
    s = _stub_sim(COUNTS)
    with pytest.raises(ValueError, match="n_max 63 is below the 64 particles"):
        s.state_tensors([2, 1, 0], n_max=63)
    with pytest.raises(ValueError, match="n_max 14 is below the 15 particles"):
        s.state_tensors([0, 0], n_max=14)
    with pytest.raises(ValueError, match="no field"):
        s.state_tensors([0], positions=False, velocities=False, phases=False)


@pytest.mark.parametrize("case, envs, kw, message", [
    ("duplicate destination", [0, 1, 0], lambda: dict(pos4=torch.zeros(3, 64, 4)), "listed twice"),
    ("nothing given", [0, 1], lambda: dict(), "neither pos4 nor vel4"),
    ("dtype", [0, 1], lambda: dict(pos4=torch.zeros(2, 64, 4, dtype=torch.float16)), "pos4: dtype"),
    ("[n, n_max, 3]", [0, 1], lambda: dict(vel4=torch.zeros(2, 64, 3)), "vel4: shape"),
    ("flat", [0, 1], lambda: dict(pos4=torch.zeros(2, 256)), "pos4 must be a [n, n_max, 4] tensor"),
    ("rows", [0, 1], lambda: dict(pos4=torch.zeros(3, 64, 4)), "pos4: shape"),
    ("two n_max", [0, 1], lambda: dict(pos4=torch.zeros(2, 64, 4), vel4=torch.zeros(2, 65, 4)), "vel4: shape"),
    ("not contiguous", [0, 1], lambda: dict(pos4=torch.zeros(2, 64, 8)[..., ::2]), "pos4: the tensor is not contiguous"),
    ("on the host", [0, 1], lambda: dict(pos4=torch.zeros(2, 64, 4)), "pos4: the tensor lives on cpu"),
    ("a numpy array", [0, 1], lambda: dict(pos4=np.zeros((2, 64, 4), np.float32)), "pos4 must be a [n, n_max, 4] tensor"),
])
def test_set_state_tensors_refuses_what_does_not_fit(case, envs, kw, message):
    s = _stub_sim(COUNTS)
    with pytest.raises(ValueError, match=re.escape(message)):
        s.set_state_tensors(envs, **kw())


def test_batched_env_passes_its_own_episodes_only():
    from flingbot_amd import env as fenv

    class Sim:
        def state_tensors(self, envs, **kw):
            return ("state", list(envs), kw)

    e = fenv.BatchedFlingEnv.__new__(fenv.BatchedFlingEnv)
    e.sim, e.envs = Sim(), [4, 2, 7]
    assert e.particle_state() == ("state", [4, 2, 7], {})
    assert e.particle_state([7, 4], phases=True) == ("state", [7, 4], dict(phases=True))
    with pytest.raises(ValueError, match=re.escape("[3]")):
        e.particle_state([4, 3])


# ---- ParticleState ----------------------------------------------------------------------------------------------------------------
def test_particle_state_views_and_mask_are_the_numpy_layout():
    from flingbot_amd import sim as fsim

    rng = np.random.RandomState(5)
    rows_p = [rng.randn(n, 4).astype(np.float32) for n in (3, 7, 1, 5)]
    rows_v = [rng.randn(n, 4).astype(np.float32) for n in (3, 7, 1, 5)]
    rows_p[1][2, 3] = 0.0   # a grasped particle
    pos, counts = ref.pack_rows(rows_p, 9)
    vel, _ = ref.pack_rows(rows_v, 9)
    phase, _ = ref.pack_rows([np.arange(n) + 10 for n in (3, 7, 1, 5)], 9, np.int32)
    st = fsim.ParticleState(torch.from_numpy(pos), torch.from_numpy(vel), torch.from_numpy(phase), counts)
    assert tuple(st) == (st.pos4, st.vel4, st.phase, st.counts) and st.n_max == 9
    assert np.array_equal(st.positions.numpy(), pos[..., :3]) and st.positions.data_ptr() == st.pos4.data_ptr()   # views, no copy
    assert np.array_equal(st.inv_mass.numpy(), pos[..., 3]) and st.inv_mass[1, 2] == 0
    assert np.array_equal(st.velocities.numpy(), vel[..., :3])
    assert st.mask.dtype == torch.bool and np.array_equal(st.mask.numpy(), ref.mask(counts, 9))
    assert st.mask.sum(1).tolist() == [3, 7, 1, 5]
    assert not st.pos4[~st.mask].any() and not st.phase[~st.mask].any()
    only_v = fsim.ParticleState(None, st.vel4, None, counts)
    assert only_v.n_max == 9 and np.array_equal(only_v.mask.numpy(), ref.mask(counts, 9))
    with pytest.raises(ValueError):
        fsim.ParticleState(None, None, None, counts).mask
