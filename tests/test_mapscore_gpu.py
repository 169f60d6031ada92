"""fs_map_score (csrc/fs_mapscore.hip) on the GPU against the float64 restatement of mapscore_reference.py, launched through
trainops.map_score on predictions scattered into zero-filled [G, 4096] maps, and train.score_maps end to end.

Columns 0-8 (counts, indices and the integer rank sums) and column 10 (regret, one exact subtraction) must have the restatement's
bits.  Column 9 (Spearman) is three roundings -- product, root, quotient -- on exact integers: 2 ulp of double are allowed, equal
bits are expected.  Column 11 is a sum of n non-negative addends in another order: (n + 16) 2^-53 A, A the sum of the addends.
Largest distance of column 9 observed on an MI355X over all cases of this file: 0 ulp."""
import numpy as np
import pytest
import torch

import maploss_reference as mref
import mapscore_reference as sref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

MANY = [int(k) for k in np.random.default_rng(300).integers(1, 6, 300)] + [300]   # more images than a workgroup has threads
LAYOUTS = {**{str(k): [k] for k in (1, 2, 5, 64, 65, 255, 256, 257, 1024, 4096)},  # the wave, stride and cap boundaries
           "empties": [0, 3, 0, 0, 7, 0],
           "many": MANY,
           "mixed": [4096, 1, 257, 0, 64],
           "2x4096": [4096, 4096]}
KINDS = {"untied": False, "quarters": True}
_cases, _worst = {}, [0]


def _case(name, kind):
    """(inputs, restatement rows, se addend sums) of a layout, made once."""
    if (name, kind) not in _cases:
        inputs = sref.scattered(LAYOUTS[name], len(name) + sum(LAYOUTS[name]), KINDS[kind])
        _cases[(name, kind)] = (inputs,) + sref.score_rows(*inputs[:4])
    return _cases[(name, kind)]


def _launch(value, offsets, pix, label, gap=0.0):
    from flingbot_amd import trainops

    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    rows = trainops.map_score(up(value), np.asarray(offsets), up(pix), up(label), gap)
    assert rows.dtype == torch.float64 and tuple(rows.shape) == (len(offsets) - 1, 12) and rows.device == torch.device(DEV)
    return rows.cpu().numpy()


def _compare(name, rows, ref, sums):
    assert rows.shape == ref.shape, name
    assert np.array_equal(rows[:, :9], ref[:, :9]), (name, np.argwhere(rows[:, :9] != ref[:, :9])[:5])
    assert sref.same_bits(rows[:, 10], ref[:, 10]), name
    far = max([sref.ulps(float(a), float(b)) for a, b in zip(rows[:, 9], ref[:, 9])], default=0)
    _worst[0] = max(_worst[0], far)
    print(f"{name}: spearman at most {far} ulp from the restatement; largest so far {_worst[0]}")
    assert far <= 2, name
    tol = (ref[:, 0] + 16.0) * 2.0 ** -53 * sums
    assert (np.abs(rows[:, 11] - ref[:, 11]) <= tol).all(), (name, float(np.abs(rows[:, 11] - ref[:, 11]).max()))


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_kernel_against_the_float64_restatement(gpu_required, name, kind):
    (value, offsets, pix, label, pred), ref, sums = _case(name, kind)
    assert {0, 4095} & set(pix.tolist()) and (len(pix) < 2 or {0, 4095} <= set(pix.tolist()))
    rows = _launch(value, offsets, pix, label)
    _compare(f"{name} {kind}", rows, ref, sums)
    if max(LAYOUTS[name]) > 4:                                                      # no case passes vacuously
        assert ref[:, 4].sum() > 0 and np.isfinite(ref[:, 9]).any()
    if KINDS[kind] and max(LAYOUTS[name]) >= 64:   # some 17 quarter values over 64 and more draws: ranks tie on both sides
        b = int(np.argmax(LAYOUTS[name]))
        assert sref.has_ties(pred[offsets[b]:offsets[b + 1]]) and sref.has_ties(label[offsets[b]:offsets[b + 1]])
    if not KINDS[kind]:
        assert all(not sref.has_ties(pred[offsets[b]:offsets[b + 1]]) for b in range(len(offsets) - 1))
    assert sref.same_bits(rows, _launch(value, offsets, pix, label))                # equal inputs: equal bits


@pytest.mark.parametrize("gap", [0.0, 0.05])
@pytest.mark.parametrize("name", ["empties", "mixed"])
def test_pairs_are_fs_map_loss_pairs(gpu_required, name, gap):
    """Columns 4-5 against the table columns P_b, C_b of fs_map_loss on the gathered predictions (finite inputs); the
    restatement with the same gap in between."""
    from flingbot_amd import trainops

    (value, offsets, pix, label, pred), _, _ = _case(name, "untied")                 # labels 1 / 128 apart: 0.05 separates few
    rows = _launch(value, offsets, pix, label, gap)
    ref, sums = sref.score_rows(value, offsets, pix, label, gap)
    _compare(f"{name} gap {gap}", rows, ref, sums)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    _, stats, table = trainops.MapLossFunction._launch(up(pred), up(label), up(offsets.astype(np.int32)), 0.5, 0.1, gap, False)
    table = table.cpu().numpy().astype(np.float64)
    assert np.array_equal(rows[:, 4:6], table[:, 2:4]) and rows[:, 4].sum() == stats[3].item()
    assert rows[:, 4].sum() > 0 or (gap and name == "empties")                      # (7 labels 1 / 128 apart: none 0.05 from another)
    if gap:
        assert rows[:, 4].sum() < _launch(value, offsets, pix, label)[:, 4].sum()   # the gap drops pairs


# where the arg-max reductions can go wrong: (lower k, higher k) of two equal largest values -- first and last lane of a wave, the
# stride boundary 255 / 256 (k = 256 is thread 0's SECOND sample: the higher k on the lower lane), another wave, the last index
PLACES = [(0, 200), (63, 64), (64, 300), (255, 256), (256, 700), (70, 1023), (1023, None), (300, 1022), (4000, 4095), (4095, None)]


def _placed(n, chosen, best, seed=4):
    """An image of n positions with distinct small values and the largest p at the k of `chosen`, the largest y at those of
    `best` (None: no partner), its pixels in list order k -> pixel (k * 2731) % 4096 (a bijection: 2731 is odd)."""
    rng = np.random.default_rng(seed)
    p = (rng.permutation(n) / n).astype(np.float32)
    y = (rng.permutation(n) / n).astype(np.float32)
    for v, places in ((p, chosen), (y, best)):
        for k in places:
            if k is not None:
                v[k] = 5.0
    pix = ((np.arange(n, dtype=np.int64) * 2731) % 4096).astype(np.int32)
    value = np.zeros((1, 4096), np.float32)
    value[0, pix] = p
    return value, np.array([0, n]), pix, y


@pytest.mark.parametrize("k", range(len(PLACES)))
def test_arg_max_ties_go_to_the_lowest_k_wherever_they_sit(gpu_required, k):
    chosen, best = PLACES[k], PLACES[(k + 3) % len(PLACES)]
    n = 4096 if max(v for v in chosen + best if v is not None) >= 1024 else 1024
    inputs = _placed(n, chosen, best)
    rows = _launch(*inputs)
    assert rows[0, 1] == chosen[0] and rows[0, 2] == best[0] and rows[0, 0] == n
    _compare(f"places {k}", rows, *sref.score_rows(*inputs))


@pytest.mark.parametrize("k", range(len(PLACES)))
def test_non_finite_values_at_those_places_are_left_out(gpu_required, k):
    places = [v for v in PLACES[k] + PLACES[(k + 3) % len(PLACES)] if v is not None]
    n = 4096 if max(places) >= 1024 else 1024
    value, offsets, pix, y = _placed(n, (5, 6), (7, 8))
    bad = [np.nan, np.inf, -np.inf]
    for i, at in enumerate(places):
        if i % 2:
            y[at] = bad[i % 3]
        else:
            value[0, pix[at]] = bad[i % 3]
    rows = _launch(value, offsets, pix, y)
    ref, sums = sref.score_rows(value, offsets, pix, y)
    assert ref[0, 0] == n - len(set(places)) and np.isfinite(ref[0, 9:]).all()
    _compare(f"non-finite {k}", rows, ref, sums)
    everything = _launch(np.full((1, 4096), np.nan, np.float32), offsets, pix, y)
    assert everything[0, :9].tolist() == sref.EMPTY[:9] and np.isnan(everything[0, 9:11]).all() and everything[0, 11] == 0.0


def test_a_row_depends_on_neither_place_nor_company(gpu_required):
    """Permuting the images permutes the rows bit for bit; an image alone has the row it has in the batch."""
    (value, offsets, pix, label, _), ref, _ = _case("mixed", "quarters")
    rows = _launch(value, offsets, pix, label)
    order = [3, 2, 0, 4, 1]
    gather = np.concatenate([np.arange(offsets[b], offsets[b + 1]) for b in order])
    moved = _launch(value[order], mref.offsets_of(np.diff(offsets)[order]), pix[gather], label[gather])
    assert sref.same_bits(moved, rows[order])
    alone = _launch(value[2:3], np.array([0, 257]), pix[offsets[2]:offsets[3]], label[offsets[2]:offsets[3]])
    assert sref.same_bits(alone, rows[2:3]) and rows[2, 0] == 257


def test_a_malformed_table_is_refused_and_clamped(gpu_required):
    """trainops.map_score refuses each defect (ValueError); the kernel, given them all at once, clamps and returns: offsets as
    fs_map_loss clamps them, pixels into [0, 4096).  One launch."""
    from flingbot_amd import sim as fsim, trainops

    L, G = 6000, 4
    rng = np.random.default_rng(2)
    value = rng.standard_normal((G, 4096)).astype(np.float32)
    pix = rng.integers(-50, 4150, L).astype(np.int32)
    label = (np.round(rng.standard_normal(L) * 4) / 4).astype(np.float32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    for bad in ([0, 3000, 2000, 5000, L], [0, -5, 100, 200, L], [0, 100, 200, 300, L + 100], [0, 5000, 5100, 5200, L]):
        with pytest.raises(ValueError):
            trainops.map_score(up(value), np.array(bad), up(pix), up(label))
    bad = np.int32([-3, 5000, 40, 100000, 60])
    assert mref.clamp_offsets(bad, L) == [(0, 4096), (5000, 0), (40, 4096), (6000, 0)]
    rows = torch.empty((G, 12), dtype=torch.float64, device=DEV)
    fsim.stream_call("fs_map_score", torch.device(DEV), up(value), 4096, up(pix), up(label), up(bad), G, L, 0.0, rows)
    ref, sums = sref.score_rows(value, bad, pix, label)
    assert ref[:, 0].tolist() == [4096, 0, 4096, 0] and ref[0, 4] > 0
    _compare("clamped", rows.cpu().numpy(), ref, sums)
    assert torch.zeros(1, device=DEV).item() == 0.0


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def _held_out():
    from flingbot_amd.replay import MapSet

    counts = [17, 0, 40, 5, 1]
    rng = np.random.default_rng(8)
    images = rng.random((5, 4, 64, 64), dtype=np.float32)
    pixels = np.concatenate([np.sort(rng.choice(4096, n, replace=False)) for n in counts]).astype(np.int32)
    labels = (rng.standard_normal(len(pixels)) * 0.1).astype(np.float32)
    labels[20] = np.nan
    return MapSet.from_arrays(images, mref.offsets_of(counts), pixels, labels)


def test_score_maps_end_to_end(gpu_required):
    """score_maps on a seeded random-weight policy against the restatement applied to the dense maps the device forward itself
    produced, read back (a second forward IMPLEMENTATION could flip near-ties); the flags, parameters and generators untouched;
    the same summary whatever images_per_batch."""
    from flingbot_amd import nets, train, trainops

    torch.manual_seed(31)
    policy = nets.MaximumValuePolicy(action_primitives=["fling"], num_rotations=12, scale_factors=[1.0], obs_dim=64, pix_grasp_dist=8,
                                     pix_drag_dist=8, pix_place_dist=5, rgb_only=True, depth_only=False, action_expl_prob=0.0,
                                     action_expl_decay=1.0, value_expl_prob=0.0, value_expl_decay=1.0, device=DEV)
    net = policy.value_nets["fling"]
    maps = _held_out().to_device(DEV)
    policy.train()
    state = {k: v.clone() for k, v in policy.state_dict().items()}
    seeds = (torch.random.get_rng_state(), torch.cuda.get_rng_state(0))
    assert net._hip is None
    out = train.score_maps(policy, {"fling": maps}, images_per_batch=2, min_gap=0.01)["fling"]
    assert net._hip is not None and all(m.training for m in policy.modules())      # folded for the HIP forward; the flags it found
    assert torch.equal(torch.random.get_rng_state(), seeds[0]) and torch.equal(torch.cuda.get_rng_state(0), seeds[1])
    assert all(torch.equal(v, state[k]) for k, v in policy.state_dict().items())
    whole = train.score_maps(policy, {"fling": maps}, images_per_batch=64, min_gap=0.01)["fling"]
    assert whole == out
    policy.eval()
    obs, offsets, pix, label = maps.take_maps(np.arange(5))
    with torch.no_grad():
        dense = net(obs)
    assert tuple(dense.shape) == (5, 1, 64, 64)
    rows = trainops.map_score(dense, offsets, pix, label, 0.01).cpu().numpy()
    ref, sums = sref.score_rows(dense.reshape(5, 4096).cpu().numpy(), offsets, pix.cpu().numpy(), label.cpu().numpy(), 0.01)
    assert ref[:, 0].tolist() == [17, 0, 39, 5, 1] and ref[:, 4].sum() > 0
    _compare("end to end", rows, ref, sums)
    want = trainops.summarize_scores(ref)
    for k, v in want.items():
        assert out[k] == (pytest.approx(v, rel=1e-13) if k in ("spearman", "mse") else v), k
    assert out["n_maps"] == 4 and out["labels"] == 62 and out["maps_with_spearman"] == 3
