"""fs_sample_actions (csrc/fs_action.hip, ActionSelector.sample) against the restatement of its rules
(tests/sample_reference.py) on the inputs of tests/sample_cases.py, BIT FOR BIT: indices, pretransform pixel pairs, and values
and keys as uint32 views."""
import itertools

import numpy as np
import pytest
import torch

import sample_cases as sc
import sample_reference as sr

pytestmark = pytest.mark.gpu

K_MAX = 16


def _keys(salt=0):
    return np.stack([sc.key_of(e, salt) for e in range(sc.N)])


def _reference(crop, inv_tau, noise, keys, first_greedy, on_cloth, radius, separation, k=K_MAX, observations=None):
    """The restatement for every observation: dict of [N, k] arrays and the summed `info` counters.  (Pick j of the rules does
    not depend on k, so the answer for a smaller k is a prefix of this one.)"""
    case = sc.case()
    observations = range(sc.N) if observations is None else observations
    outs, infos = [], dict(tie_decided=0, suppressed=0, cloth_only=0, tail=0)
    for e in observations:
        cloth = _cloth(e, radius) if radius > 0 else None
        got, info = sr.sample(crop[e], case["tables"][e], cloth, len(sc.PRIMS), k, inv_tau, noise, keys[e], first_greedy, on_cloth,
                              separation)
        outs.append(got)
        for name in infos:
            infos[name] += info[name]
    return {f: np.stack([o[f] for o in outs]) for f in ("index", "value", "key", "pixels")}, infos


_cloth_tables = {}


def _cloth(e, radius):
    if (e, radius) not in _cloth_tables:
        case = sc.case()
        _cloth_tables[e, radius] = sr.cloth_table(case["tables"][e], case["depth"][e], sc.PRIMS, radius)
    return _cloth_tables[e, radius]


def _device(values, depth, noise, k, inv_tau, keys, first_greedy, on_cloth, radius, separation, scales=None):
    sel = sc.case()["sel"]
    index, value, key, pixels = sel.sample(values, sc.SCALES if scales is None else scales, depth, k, keys, inv_tau, noise,
                                           first_greedy=first_greedy, on_cloth=on_cloth, radius=radius, separation=separation)
    return dict(index=index, value=value, key=key, pixels=pixels.reshape(len(index), k, 4))


def _assert_equal(got, want, k, what):
    assert got["index"].dtype == np.int64 and got["index"].shape == want["index"][:, :k].shape, what
    assert np.array_equal(got["index"], want["index"][:, :k]), what
    assert np.array_equal(got["pixels"], want["pixels"][:, :k]), what
    for f in ("value", "key"):
        assert np.array_equal(got[f].view(np.uint32), want[f][:, :k].view(np.uint32)), (what, f)


@pytest.fixture(scope="module")
def dev(gpu_required):
    from flingbot_amd.action import gumbel_table

    case = sc.case()
    return dict(values=torch.tensor(case["values"]).cuda(), depth=torch.tensor(case["depth"]).cuda(),
                tables={"gumbel": (gumbel_table(), gumbel_table("cuda:0")),
                        "four": (sc.four_level_table(), torch.tensor(sc.four_level_table()).cuda())})


CLOTH = ((False, 1), (True, 1), (True, 2))       # (on_cloth, r)


def test_inputs_are_not_vacuous():
    """On the restatement alone: the index rule, suppression, the on-cloth filter and the -1 tail all decide something."""
    case = sc.case()
    assert np.isnan(case["values"]).mean() > 0.05 and np.isinf(case["crop"]).sum() >= 20
    assert (case["depth"] == 0.0).any() and (case["depth"] == 2.0).any()
    assert not case["tables"][sc.NONE]["valid"].any() and case["tables"][sc.FEW]["valid"].sum() > K_MAX
    few = case["tables"][sc.FEW]["valid"] & _cloth(sc.FEW, 1) & ~np.isnan(case["crop"][sc.FEW])
    assert 1 <= few.sum() < K_MAX, "fewer than k eligible candidates on the tiny blob"
    want, info = _reference(case["crop"], 1.0, sc.four_level_table(), _keys(), True, True, 1, 3)
    assert info["tie_decided"] >= 1, "at least one pick decided by the lowest-index rule"
    assert info["suppressed"] >= 1, "at least one candidate that suppression removed from a winning position"
    assert info["cloth_only"] >= 1, "at least one candidate that only the on-cloth filter excluded"
    assert info["tail"] >= 1 and (want["index"][sc.NONE] == -1).all() and (want["index"][sc.FEW] == -1).any()
    assert (want["index"][sc.FEW] >= 0).any() and (want["index"][:3, :6] >= 0).all()
    # the same keys on the Gumbel table tie nowhere: the four-level table is what makes ties
    _, info = _reference(case["crop"], 0.0, sc.four_level_table(), _keys(), False, False, 1, 0)
    assert info["tie_decided"] >= K_MAX


@pytest.mark.parametrize("table", ["gumbel", "four"])
@pytest.mark.parametrize("inv_tau", [0.0, 1.0, 20.0, 1.0 / 0.07])
def test_device_equals_the_restatement_bit_for_bit(dev, table, inv_tau):
    """k in {1, 6, 16} x first_greedy x on_cloth (r in {1, 2}) x separation in {0, 3}, for one table and one inv_tau (1 / 0.07
    on top of the round ones: a product that rounds, which is where a fused key would show)."""
    case = sc.case()
    host, device = dev["tables"][table]
    keys = _keys()
    for first_greedy, (on_cloth, radius), separation in itertools.product((True, False), CLOTH, (0, 3)):
        want, _ = _reference(case["crop"], inv_tau, host, keys, first_greedy, on_cloth, radius, separation)
        for k in (1, 6, 16):
            got = _device(dev["values"], dev["depth"], device, k, inv_tau, keys, first_greedy, on_cloth, radius, separation)
            _assert_equal(got, want, k, (table, inv_tau, first_greedy, on_cloth, radius, separation, k))
            empty = got["index"] < 0
            assert (got["value"][empty] == 0).all() and (got["key"][empty] == 0).all() and (got["pixels"][empty] == 0).all()


def test_zero_table_single_pick_is_select(dev):
    case, sel = sc.case(), sc.case()["sel"]
    zero = torch.zeros(65536, device="cuda:0")
    got = _device(dev["values"], dev["depth"], zero, 1, 1.0, _keys(), False, False, 1, 0)
    for e in range(sc.N):
        action, params = sel.select(dev["values"][e], sc.SCALES[e], case["depth"][e])
        if action is None:
            assert got["index"][e, 0] == -1 and e == sc.NONE
            continue
        assert got["index"][e, 0] == params["flat_index"] and np.float32(params["value"]) == got["value"][e, 0]
        assert np.array_equal(got["pixels"][e, 0], np.ravel(params["pretransform_pixels"]))
    # ... and so is the greedy pick, whatever the table and the temperature
    got = _device(dev["values"], dev["depth"], dev["tables"]["gumbel"][1], 4, 0.0, _keys(), True, True, 2, 3)
    for e in range(3):
        action, params = sel.select(dev["values"][e], sc.SCALES[e], case["depth"][e])
        assert got["index"][e, 0] == params["flat_index"] and got["key"][e, 0] == got["value"][e, 0]


def test_picks_depend_on_map_and_key_only(dev):
    """Two observations with equal maps and equal keys get equal picks; with different keys the picks differ."""
    values = torch.stack([dev["values"][1]] * 3)
    depth = torch.stack([dev["depth"][1]] * 3)
    keys = np.stack([sc.key_of(1), sc.key_of(1), sc.key_of(1, salt=1)])
    got = _device(values, depth, dev["tables"]["gumbel"][1], 8, 1.0, keys, False, True, 1, 0, scales=[sc.SCALES[1]] * 3)
    for f in ("index", "value", "key", "pixels"):
        assert np.array_equal(got[f][0], got[f][1]), f
    assert not np.array_equal(got["index"][0], got["index"][2])
    case = sc.case()
    for row in (0, 2):
        want, _ = sr.sample(case["crop"][1], case["tables"][1], _cloth(1, 1), len(sc.PRIMS), 8, 1.0, dev["tables"]["gumbel"][0],
                            keys[row], False, True, 0)
        assert np.array_equal(got["index"][row], want["index"]), row


@pytest.mark.parametrize("where", [0, sc.TOTAL - 1, sc.BLOCK - 1, sc.BLOCK + 1, 4 * sc.BLOCK - 1, 4 * sc.BLOCK + 1])
def test_best_key_at_the_ends_of_a_threads_range(dev, where):
    """The best key planted at flat index `where` -- the first and the last candidate, and either side of a thread's and of the
    workgroup's trip (1024 threads x 4 candidates) -- of an observation in which every candidate is valid: a flat cloth in
    reach of both arms, scales that keep every turned pixel inside the image, a place that ends inside the map."""
    from flingbot_amd.action import ActionSelector

    assert sc.TOTAL > 4 * sc.BLOCK + 1
    sel = ActionSelector(sc.PRIMS, sc.ROTATIONS, sc.D, sc.G, sc.DRAG, sc.G, 10.0)   # (a place as long as the margin is wide)
    scales = np.array([0.5, 0.6])
    depth = np.full((sc.S, sc.S), 1.9, np.float32)
    values = (np.round(np.random.default_rng(where).random((len(sc.PRIMS), sc.T, sc.D, sc.D)) * 64) / 64).astype(np.float32)
    p, t, yy, zz = (int(v) for v in np.unravel_index(where, (len(sc.PRIMS), sc.T, sc.W, sc.W)))
    values[p, t, yy + sc.G, zz + sc.G] = np.float32(9.0)       # beyond what the four-level table (< 1) can make up
    want = sel._candidate(sc.PRIMS[p], t, yy + sc.G, zz + sc.G, scales, depth)
    assert want is not None
    host, device = dev["tables"]["four"]
    key = sc.key_of(0, salt=where)
    index, value, got_key, pixels = sel.sample(torch.tensor(values).cuda()[None], [scales], torch.tensor(depth).cuda()[None], 1,
                                               key[None], 1.0, device, first_greedy=False, on_cloth=False, separation=0)
    assert index[0, 0] == where and value[0, 0] == np.float32(9.0)
    assert got_key[0, 0] == np.float32(9.0) + host[int(sr.hash32(where, key[0], key[1])) >> 16]
    assert np.array_equal(pixels[0, 0], want["pretransform_pixels"])


def test_sampled_returns_candidates_with_select_first(dev):
    """ActionSelector.sampled on the same inputs: what `candidates` returns plus 'sample_key'; candidate 0 is select's action;
    no identity twice; a temperature that is not positive is refused."""
    case, sel = sc.case(), sc.case()["sel"]
    keys = _keys()
    got = sel.sampled(dev["values"], sc.SCALES, list(case["depth"]), 4, keys, 0.5, separation=2, radius=1)
    assert len(got) == sc.N and got[sc.NONE] == []
    for e in range(3):
        action, params = sel.select(dev["values"][e], sc.SCALES[e], case["depth"][e])
        assert got[e][0][0] == action and got[e][0][1]["flat_index"] == params["flat_index"]
        assert np.array_equal(got[e][0][1]["p1"], params["p1"]) and np.array_equal(got[e][0][1]["p2"], params["p2"])
        assert len(got[e]) == 4
        ident = {(c[0], tuple(np.ravel(c[1]["pretransform_pixels"]))) for c in got[e]}
        assert len(ident) == 4
        for prim, c in got[e]:
            assert {"flat_index", "transform_index", "value", "sample_key", "p1", "p2", "max_indices"} <= set(c)
            assert c["transform_index"] == int(c["max_indices"][0]) and prim in sc.PRIMS
    again = sel.sampled(dev["values"], sc.SCALES, list(case["depth"]), 4, keys, 0.5, separation=2, radius=1)
    assert [[c[1]["flat_index"] for c in row] for row in again] == [[c[1]["flat_index"] for c in row] for row in got]
    uniform = sel.sampled(dev["values"], sc.SCALES, list(case["depth"]), 4, keys, float("inf"), first_greedy=False)
    assert all(len(row) == 4 for row in uniform[:3])
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            sel.sampled(dev["values"], sc.SCALES, list(case["depth"]), 4, keys, bad)
