"""fs_sample_actions without a GPU: the hash against values worked out with Python integers, the header and the library's
host-side refusals, the restatement (tests/sample_reference.py) as the distribution it claims to be -- a Plackett-Luce draw
with probability ~ exp(value / tau) -- and its switchable mistakes, each of which must change the cases that name it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sample_cases as sc
import sample_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hash_by_hand(c, lo, hi):
    h = (c * 0x9E3779B1 + lo * 0x85EBCA77 + hi * 0xC2B2AE3D) & 0xFFFFFFFF
    h ^= h >> 16; h = (h * 0x7FEB352D) & 0xFFFFFFFF; h ^= h >> 15; h = (h * 0x846CA68B) & 0xFFFFFFFF; h ^= h >> 16   # noqa: E702
    return h


def test_hash_equals_python_integers():
    for c, lo, hi in ((0, 0, 0), (1, 2, 3), (221183, 0xFFFFFFFF, 0x80000001)):
        assert int(sr.hash32(c, lo, hi)) == _hash_by_hand(c, lo, hi)
    assert _hash_by_hand(0, 0, 0) == 0 and _hash_by_hand(1, 2, 3) != _hash_by_hand(1, 3, 2)
    got = sr.hash32(np.arange(5), 9, 7)
    assert got.dtype == np.uint32 and [int(v) for v in got] == [_hash_by_hand(c, 9, 7) for c in range(5)]


def test_gumbel_table():
    from flingbot_amd.action import gumbel_table

    table = gumbel_table()
    assert table.dtype == np.float32 and table.shape == (65536,) and (np.diff(table) > 0).all()
    for i in (0, 1, 32767, 65535):
        assert table[i] == np.float32(-np.log(-np.log((i + 0.5) / 65536)))
    assert gumbel_table() is table


# ---- header and library ---------------------------------------------------------------------------------------------------
def _call(lib, **kw):
    """fs_sample_actions with valid host arguments and made-up device addresses (never dereferenced: a refusal comes before
    anything is enqueued), one of them replaced."""
    dp, fp, ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int)
    n, k = 2, kw.get("k", 4)
    host = dict(kinds=np.zeros(1, np.int32), mats=np.zeros((n, 6, 9)), pose=np.eye(4), left=np.zeros(3), right=np.zeros(3),
                keys=np.zeros((n, 2), np.uint32), index=np.zeros((n, 16), np.int64), value=np.zeros((n, 16), np.float32),
                key=np.zeros((n, 16), np.float32), pix=np.zeros((n, 16, 4), np.int32))
    a = dict(values=0x10000, n=n, P=1, kinds=host["kinds"].ctypes.data_as(ip), T=6, D=32, g=4, drag=4, place=4,
             mats=host["mats"].ctypes.data_as(dp), depth=0x20000, S=48, fx=1.0, pose=host["pose"].ctypes.data_as(dp),
             left=host["left"].ctypes.data_as(dp), right=host["right"].ctypes.data_as(dp), reach=1.0, sd=0.3, gh=0.02, k=k,
             noise=0x30000, noise_bits=16, inv_tau=1.0, keys=host["keys"].ctypes.data_as(C.POINTER(C.c_uint)), first_greedy=1,
             on_cloth=1, radius=1, separation=0, index=host["index"].ctypes.data_as(C.POINTER(C.c_longlong)),
             value=host["value"].ctypes.data_as(fp), key=host["key"].ctypes.data_as(fp), pix=host["pix"].ctypes.data_as(ip),
             work=0x40000, stream=None)
    a.update(kw)
    return lib.fs_sample_actions(*a.values())


def test_header_declares_and_library_exports_the_entry_points():
    from flingbot_amd import sim as fsim

    with open(os.path.join(ROOT, "include", "flingsim.h")) as fh:
        header = fh.read()
    assert re.search(r"\bint fs_sample_actions\(const float \*d_values, int n, int n_primitives,", header)
    assert re.search(r"\bsize_t fs_sample_actions_work_bytes\(int n, int n_primitives, int n_transforms, int obs_dim, "
                     r"int pix_grasp_dist, int k\);", header)
    lib = fsim.load_library()
    for name in ("fs_sample_actions", "fs_sample_actions_work_bytes"):
        assert hasattr(lib, name) and name in lib._fs_symbols
    need = lib.fs_sample_actions_work_bytes(3, 2, 6, 32, 4, 16)
    assert need >= 3 * 6 * 9 * 8 + 3 * 8 + 3 * sc.TOTAL * 5 + 3 * 16 * 32     # matrices, keys, float + byte per candidate, picks
    for shape in ((0, 2, 6, 32, 4, 4), (3, 0, 6, 32, 4, 4), (3, 2, 0, 32, 4, 4), (3, 2, 6, 8, 4, 4), (3, 2, 6, 32, 4, 0),
                  (3, 2, 6, 32, 4, 17), (1, 8, 4096, 4096, 0, 4)):                # the last: 2^39 candidates
        assert lib.fs_sample_actions_work_bytes(*shape) == 0, shape


@pytest.mark.parametrize("kw, word", [
    (dict(values=None), b"null"), (dict(noise=None), b"null"), (dict(keys=None), b"null"), (dict(pix=None), b"null"),
    (dict(work=None), b"null"), (dict(k=0), b"k must be"), (dict(k=17), b"k must be"), (dict(noise_bits=15), b"noise_bits"),
    (dict(noise_bits=17), b"noise_bits"), (dict(inv_tau=-1.0), b"inv_tau"), (dict(inv_tau=float("inf")), b"inv_tau"),
    (dict(inv_tau=float("nan")), b"inv_tau"), (dict(separation=-1), b"separation"), (dict(work=0x40008), b"aligned"),
    (dict(P=8, T=4096, D=4096, g=0), b"2^31"), (dict(first_greedy=2), b"0 or 1")])
def test_refusals_need_no_device(kw, word):
    from flingbot_amd import sim as fsim

    lib = fsim.load_library()
    if "P" in kw:   # as many kinds and matrices as the shape names
        kinds, mats = np.zeros(8, np.int32), np.zeros((2, 4096, 9))
        kw = dict(kw, kinds=kinds.ctypes.data_as(C.POINTER(C.c_int)), mats=mats.ctypes.data_as(C.POINTER(C.c_double)))
    assert _call(lib, **kw) == -1
    err = lib.fs_last_error()
    assert b"fs_sample_actions" in err and word in err, err


# ---- the restatement is the distribution it claims to be ---------------------------------------------------------------------
TRIALS = 20000


def _open_table(n):
    """n always-valid candidates of one primitive with pairwise different pixels: nothing but a pick itself is suppressed."""
    pixels = np.stack([np.arange(n)] * 4, axis=1).astype(np.int32)
    return dict(valid=np.ones(n, bool), pixels=pixels)


@pytest.mark.parametrize("inv_tau", [4.0, 0.0])
def test_top_two_follow_plackett_luce(inv_tau):
    """chi^2 of the first pick against softmax(inv_tau v) (15 degrees of freedom, 99.9 % quantile 37.70) and of the second
    pick given the most frequent first one against the renormalised softmax (14 degrees, 36.12), over the keys (j, 7),
    j < 20 000.  The inputs are fixed, so the test is deterministic."""
    from flingbot_amd.action import gumbel_table

    values = (np.round(np.random.default_rng(5).random(16) * 64) / 64).astype(np.float32)
    noise = gumbel_table()
    h = sr.hash32(np.arange(16)[None, :], np.arange(TRIALS)[:, None], 7)
    keys = ((values * np.float32(inv_tau)).astype(np.float32)[None, :] + noise[h >> np.uint32(16)]).astype(np.float32)
    order = np.lexsort((np.broadcast_to(np.arange(16), keys.shape), -keys.astype(np.float64)), axis=1)
    first, second = order[:, 0], order[:, 1]
    table = _open_table(16)
    for j in range(0, TRIALS, 97):   # the vectorised draw above is the restatement's
        got, _ = sr.sample(values, table, None, 1, 2, inv_tau, noise, (j, 7), False, False, 0)
        assert list(got["index"]) == [first[j], second[j]] and got["key"][0] == keys[j, first[j]]
    p = np.exp(np.float64(inv_tau) * values.astype(np.float64))
    p /= p.sum()
    counts = np.bincount(first, minlength=16)
    chi_first = float(((counts - TRIALS * p) ** 2 / (TRIALS * p)).sum())
    top = int(np.argmax(counts))
    rest = np.arange(16) != top
    q = p[rest] / p[rest].sum()
    counts2 = np.bincount(second[first == top], minlength=16)[rest]
    chi_second = float(((counts2 - counts2.sum() * q) ** 2 / (counts2.sum() * q)).sum())
    print(f"inv_tau {inv_tau}: chi^2 first {chi_first:.2f}, second given {top} {chi_second:.2f} ({counts2.sum()} draws)")
    assert chi_first < 37.70 and chi_second < 36.12


# ---- every switchable mistake changes the cases that name it -----------------------------------------------------------------
def _run(e, mistake=None, k=16, inv_tau=1.0, noise=None, first_greedy=True, on_cloth=True, radius=1, separation=0):
    case = sc.case()
    noise = sc.four_level_table() if noise is None else noise
    cloth = sr.cloth_table(case["tables"][e], case["depth"][e], sc.PRIMS, radius, mistake) if radius > 0 else None
    got, _ = sr.sample(case["crop"][e], case["tables"][e], cloth, len(sc.PRIMS), k, inv_tau, noise, sc.key_of(e), first_greedy,
                       on_cloth, separation, mistake)
    return got


def _differs(a, b):
    return any(not np.array_equal(a[f].view(np.uint32) if a[f].dtype == np.float32 else a[f], b[f].view(np.uint32)
                                  if b[f].dtype == np.float32 else b[f]) for f in ("index", "value", "key", "pixels"))


@pytest.mark.parametrize("mistake, kw", [
    ("noise_per_pick", dict(inv_tau=0.0, first_greedy=False)),
    ("ties_high", dict(inv_tau=1.0)),                                   # the four-level table: exact key ties
    ("suppress_one_point", dict(inv_tau=20.0, separation=3)),
    ("fused_key", dict(inv_tau=1.0 / 0.07, noise="gumbel")),           # a product that rounds (1 and 20 times n / 64 do not)
    ("greedy_on_cloth", dict(inv_tau=1.0, radius=2)),
    ("second_point", dict(inv_tau=0.0, radius=2))])
def test_mistake_changes_its_cases(mistake, kw):
    from flingbot_amd.action import gumbel_table

    assert mistake in sr.MISTAKES
    kw = dict(kw)
    if kw.get("noise") == "gumbel":
        kw["noise"] = gumbel_table()
    changed = [e for e in range(3) if _differs(_run(e, None, **kw), _run(e, mistake, **kw))]
    assert changed, f"{mistake} changes nothing on {kw}"
