"""flingbot_amd.replay on the host: the numpy restatement of torchvision's ColorJitter chain for PIL inputs against what
Pillow itself computes (tests/golden/jitter_golden.npz, made by tests/golden/make_jitter_golden.py), the replay file round
trip through taskio.save_replay -> ExperienceSet, and MaximumValuePolicy's keyed exploration."""
import os
import random

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jitter_golden.npz")


def golden_cases():
    z = np.load(GOLDEN, allow_pickle=False)
    imgs = z["images"][z["image_index"]]
    return imgs, {"order": z["order"], "factors": z["factors"]}, z["outputs"]


# ---- the jitter ------------------------------------------------------------------------------------------------------
def test_color_jitter_host_equals_the_pillow_fixture_exactly():
    from flingbot_amd import replay

    imgs, params, want = golden_cases()
    assert len(want) >= 40 and len({tuple(o) for o in params["order"]}) == 24       # every order at least once
    f = params["factors"]
    for op, (lo, hi) in enumerate(replay.JITTER_RANGES):                                # both ends of every range
        assert (f[:, op] == np.float32(lo)).any() and (f[:, op] == np.float32(hi)).any()
    assert (f[:, 3] == 0).any() and ((f[:, 3] < 0) & (f[:, 3] > -0.01)).any()
    # float input whose quantisation is the fixture's uint8 image: (v + 0.5) / 255 truncates back to v
    rgb = ((imgs.astype(np.float32) + np.float32(0.5)) / np.float32(255.0)).transpose(0, 3, 1, 2)
    assert (replay.quantize(rgb).transpose(0, 2, 3, 1) == imgs).all()
    got = replay.color_jitter_host(rgb, params)
    assert got.dtype == np.float32 and got.shape == rgb.shape
    for k in range(len(want)):
        assert (got[k] == want[k].transpose(2, 0, 1).astype(np.float32) / np.float32(255.0)).all(), (k, params["order"][k], f[k])
        assert (replay.jitter_uint8(imgs[k], params["order"][k], f[k]) == want[k]).all(), k


def test_quantize_clamps_what_the_spline_overshoots():
    from flingbot_amd import replay

    x = np.array([-0.25, -1e-9, 0.0, 0.5 / 255, 1.0 / 255, 0.999999, 1.0, 1.0000001, 1.3, 254.999 / 255], np.float32)
    assert replay.quantize(x).tolist() == [0, 0, 0, 0, 1, 254, 255, 255, 255, 254]


def test_draw_jitter_ranges_and_orders():
    from flingbot_amd import replay

    p = replay.draw_jitter(np.random.default_rng(3), 4000)
    assert p["order"].shape == (4000, 4) and p["order"].dtype == np.int32 and p["factors"].dtype == np.float32
    assert (np.sort(p["order"], axis=1) == np.arange(4)).all()
    assert len({tuple(o) for o in p["order"]}) == 24
    for op, (lo, hi) in enumerate(replay.JITTER_RANGES):
        f = p["factors"][:, op].astype(np.float64)
        assert f.min() >= lo - 1e-6 and f.max() <= hi + 1e-6 and f.min() < lo + 0.02 * (hi - lo) and f.max() > hi - 0.02 * (hi - lo)
    q = replay.draw_jitter(np.random.default_rng(3), 4000)
    assert (q["order"] == p["order"]).all() and (q["factors"] == p["factors"]).all()


def _pillow_chain(img, order, factors):
    """torchvision.transforms.ColorJitter.forward on a PIL image, as the Pillow calls of functional_pil."""
    from PIL import Image, ImageEnhance

    im = Image.fromarray(np.ascontiguousarray(img), "RGB")
    for op in order:
        if op == 0:
            im = ImageEnhance.Brightness(im).enhance(float(factors[0]))
        elif op == 1:
            im = ImageEnhance.Contrast(im).enhance(float(factors[1]))
        elif op == 2:
            im = ImageEnhance.Color(im).enhance(float(factors[2]))
        else:
            h, s, v = im.convert("HSV").split()
            shifted = (np.array(h, dtype=np.uint8).astype(np.int32) + int(float(factors[3]) * 255) % 256) % 256
            im = Image.merge("HSV", (Image.fromarray(shifted.astype(np.uint8), "L"), s, v)).convert("RGB")
    return np.array(im)


def test_hsv_round_trip_equals_pillow_on_all_colours():
    """(importorskip: the fixture test above pins the same code without Pillow and always runs.)"""
    pytest.importorskip("PIL")
    from PIL import Image

    from flingbot_amd import replay

    a = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    hsv = np.array(Image.fromarray(rgb, "RGB").convert("HSV"))
    assert (replay.rgb_to_hsv(rgb) == hsv).all()
    assert (replay.hsv_to_rgb(rgb) == np.array(Image.fromarray(rgb, "HSV").convert("RGB"))).all()   # all 2^24 HSV triples
    assert (replay.hsv_to_rgb(replay.rgb_to_hsv(rgb)) == np.array(Image.fromarray(hsv, "HSV").convert("RGB"))).all()


def test_fresh_draws_equal_the_live_pillow_chain():
    pytest.importorskip("PIL")
    from flingbot_amd import replay

    rng = np.random.default_rng(2024)
    for k in range(200):
        img = rng.integers(0, 256, (64, 64, 3)).astype(np.uint8)
        if k % 4 == 1:      # low-contrast, near-gray content: where the hue and the contrast mean are touchy
            img = np.clip(rng.integers(60, 70) + rng.integers(-2, 3, (64, 64, 3)), 0, 255).astype(np.uint8)
        p = replay.draw_jitter(rng, 1)
        want = _pillow_chain(img, p["order"][0], p["factors"][0])
        assert (replay.jitter_uint8(img, p["order"][0], p["factors"][0]) == want).all(), (k, p)


# ---- the replay file -------------------------------------------------------------------------------------------------
D = 64
TASK = {"cloth_mass": 0.5, "flatten_area": 2.0, "task_difficulty": "hard", "initial_coverage": 0.5}


def _arrays(rng, y, z, x=5):
    mask = np.zeros((D, D), bool)
    mask[y, z] = True
    return dict(observations=rng.random((4, D, D), dtype=np.float32), actions=mask, value_map=rng.random((D, D), dtype=np.float32),
                max_indices=np.array([x, y, z], np.int64), rotation=-30.0, scale=1.25)


def _records(rng, with_arrays=True):
    a = dict(coverage=[1.0, 1.25, 1.5, 1.5], actions=["fling", "drag", None], rewards=[0.25, 0.25, 0.0],
             preaction_coverage=[1.0, 1.25, 1.5])
    b = dict(coverage=[0.5, 0.25], actions=["fling"], rewards=[-0.25], preaction_coverage=[0.5])
    if with_arrays:
        a["experience"] = [_arrays(rng, 10, 20), _arrays(rng, 30, 40), None]
        b["experience"] = [_arrays(rng, 50, 9)]
    return [a, b]


def test_replay_round_trip(tmp_path):
    from flingbot_amd import replay, taskio

    rng = np.random.default_rng(0)
    recs = _records(rng)
    path, plain = str(tmp_path / "with.npz"), str(tmp_path / "plain.npz")
    assert taskio.save_replay(path, recs, [TASK, TASK]) == 4
    taskio.save_replay(plain, _records(rng, with_arrays=False), [TASK, TASK])
    z, zp = np.load(path), np.load(plain)
    # a file from records without arrays has exactly the entry names the parent writes
    want = {"format", "keys"} | {f"{k}/{f}" for k in zp["keys"] for f in taskio.REPLAY_SCALARS}
    assert set(zp.files) == want
    keys = [str(k) for k in z["keys"]]
    assert keys == ["000000000_step00", "000000000_step01", "000000000_step02_last", "000000001_step00_last"]
    with_arrays = [keys[0], keys[1], keys[3]]
    assert set(z.files) == want | {f"{k}/{f}" for k in with_arrays for f in taskio.REPLAY_ARRAYS}
    g = keys[1]
    assert z[f"{g}/observations"].dtype == np.float32 and z[f"{g}/observations"].shape == (4, D, D)
    assert z[f"{g}/actions"].dtype == bool and z[f"{g}/actions"].shape == (D, D) and z[f"{g}/actions"][30, 40]
    assert z[f"{g}/value_map"].dtype == np.float32 and z[f"{g}/value_map"].shape == (D, D)
    assert z[f"{g}/max_indices"].tolist() == [5, 30, 40] and float(z[f"{g}/rotation"]) == -30.0 and float(z[f"{g}/scale"]) == 1.25
    # collect_stats reads both kinds of file and gives the same result
    cs, cp = taskio.collect_stats(path), taskio.collect_stats(plain)
    assert set(cs) == set(cp) and all(np.array_equal(cs[k], cp[k]) for k in cs)

    full = replay.ExperienceSet([path], rgb_only=False, depth_only=False)
    assert len(full) == 3 and full.keys == with_arrays and full.n_without_arrays == 1 and full.n_invalid == 0
    assert full.observations.dtype == np.float32 and full.observations.shape == (3, 4, D, D)
    assert full.masks.dtype == bool and full.masks.shape == (3, D, D) and full.labels.dtype == np.float32
    assert (full.observations[1] == recs[0]["experience"][1]["observations"]).all()
    # label: (post - pre) / max_coverage, float64 arithmetic stored as float32
    assert full.labels.tolist() == [np.float32(0.25 / 2.0), np.float32(0.25 / 2.0), np.float32(-0.25 / 2.0)]
    minmax = replay.ExperienceSet(path, use_normalized_coverage=False)
    lo, hi = -0.11034914070874759, 0.20572495126190674
    assert minmax.labels.tolist() == [np.float32((0.25 - lo) / (hi - lo))] * 2 + [np.float32((-0.25 - lo) / (hi - lo))]
    # the primitive filter, over two files
    fling = replay.ExperienceSet([path, path], action_primitive="fling")
    assert fling.keys == [keys[0], keys[3]] * 2 and fling.n_filtered == 2
    # channels (utils.py:94-98) and where the jitter applies
    idx = np.array([2, 0])
    obs, mask, label = full.item_host(idx, replay.draw_jitter(rng, 2))
    assert obs.shape == (2, 4, D, D) and (obs == full.observations[idx]).all() and not full.jitters
    assert (mask == full.masks[idx]).all() and mask[0, 50, 9] and (label == full.labels[idx]).all()
    depth = replay.ExperienceSet(path, rgb_only=False, depth_only=True)
    assert (depth.item_host(idx)[0] == full.observations[idx, 3:4]).all() and not depth.jitters
    rgb = replay.ExperienceSet(path)
    p = replay.draw_jitter(rng, 2)
    assert rgb.jitters and (rgb.item_host(idx, p)[0] == replay.color_jitter_host(full.observations[idx, :3], p)).all()
    assert (replay.ExperienceSet(path, obs_color_jitter=False).item_host(idx, p)[0] == full.observations[idx, :3]).all()
    with pytest.raises(RuntimeError):
        rgb.sample(2, rng)                       # not uploaded: there is no host fallback behind sample()
    with pytest.raises(AssertionError):
        replay.ExperienceSet(path, rgb_only=True, depth_only=True)


def test_validity_rule_drops_and_counts(tmp_path):
    from flingbot_amd import replay, taskio

    rng = np.random.default_rng(1)
    recs = _records(rng)
    recs[0]["experience"][1]["actions"][0, 0] = True          # two true pixels
    recs[1]["experience"][0]["actions"][:] = False            # none
    path = str(tmp_path / "doctored.npz")
    taskio.save_replay(path, recs, [TASK, TASK])
    data = replay.ExperienceSet(path)
    assert len(data) == 1 and data.keys == ["000000000_step00"] and data.n_invalid == 2 and data.n_without_arrays == 1


def test_command_line_flags_default_to_todays_behaviour():
    from flingbot_amd.evaluate import build_parser

    a = build_parser().parse_args(["--tasks", "t.npz"])
    assert a.record_experience is False and a.action_expl_prob == 0.0 and a.value_expl_prob == 0.0 and a.seed is None
    b = build_parser().parse_args(["--tasks", "t.npz", "--record-experience", "--dump", "r.npz", "--action-expl-prob", "0.5",
                                   "--value-expl-prob", "0.25", "--seed", "3"])
    assert b.record_experience and b.action_expl_prob == 0.5 and b.value_expl_prob == 0.25 and b.seed == 3


# ---- keyed exploration -----------------------------------------------------------------------------------------------
def _policy(action_prob, value_prob, prims=("fling", "drag", "place")):
    from flingbot_amd import nets

    torch.manual_seed(0)
    policy = nets.MaximumValuePolicy(action_primitives=list(prims), num_rotations=2, scale_factors=[1.0, 1.5], obs_dim=16,
                                   pix_grasp_dist=2, pix_drag_dist=2, pix_place_dist=2, rgb_only=True, depth_only=False,
                                   action_expl_prob=action_prob, action_expl_decay=1.0, value_expl_prob=value_prob,
                                   value_expl_decay=1.0, device="cpu")
    # stand-ins for the networks that treat every image on its own, so that a map cannot depend on the batch it was in
    for n, net in enumerate(policy.value_nets.values()):
        net.forward = lambda batch, n=n: batch[:, :1] * (n + 1.0) + batch[:, 1:2]
    return policy


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_keyed_exploration_is_a_function_of_the_key():
    policy = _policy(0.5, 0.5)
    gen = torch.Generator().manual_seed(4)
    obs = [torch.rand(4, 4, 16, 16, generator=gen) for _ in range(6)]
    keys = [(3, i, 0) for i in range(6)]
    state = random.getstate()
    whole = policy.act(obs, keys=keys)
    assert random.getstate() == state                      # the global stream is not touched
    for i in (5, 2):                                       # alone, and in another order with other company
        assert _same(policy.act([obs[i]], keys=[keys[i]])[0], whole[i])
    perm = [4, 0, 5, 1]
    for got, i in zip(policy.act([obs[i] for i in perm], keys=[keys[i] for i in perm]), perm):
        assert _same(got, whole[i])
    # different keys differ: the same observation under 32 keys does not always get the same treatment
    many = policy.act([obs[0]] * 32, keys=[(3, 0, k) for k in range(32)])
    assert len({tuple(float(v.sum()) for v in m.values()) for m in many}) > 4
    sure = _policy(0.0, 1.0)
    assert not _same(sure.act([obs[0]], keys=[(3, 0, 0)])[0], sure.act([obs[0]], keys=[(3, 0, 1)])[0])
    assert not _same(sure.act([obs[0]], keys=[(3, 0, 0)])[0], sure.act([obs[0]], keys=[(4, 0, 0)])[0])
    assert _same(sure.act([obs[0]], keys=[(3, 0, 0)])[0], sure.act([obs[0]], keys=[(3, 0, 0)])[0])
    with pytest.raises(ValueError):
        policy.act(obs, keys=keys[:2])
    policy.decay_exploration()                             # stays callable


def test_keyed_exploration_follows_the_references_rule():
    """nets.py:279-293: a value-exploring net's map is uniform [0, 1) of shape [T, D, D]; action exploration keeps the
    chosen primitive's map and fills the others with its minimum."""
    gen = torch.Generator().manual_seed(5)
    obs = [torch.rand(4, 4, 16, 16, generator=gen)]
    plain = _policy(0.0, 0.0).act(obs)[0]
    assert _same(_policy(0.0, 0.0).act(obs, keys=[(1, 2, 3)])[0], plain)          # probabilities 0: nothing is replaced
    every = _policy(0.0, 1.0).act(obs, keys=[(1, 2, 3)])[0]
    for k, v in every.items():
        assert v.shape == (4, 16, 16) and v.dtype == torch.float32 and 0.0 <= float(v.min()) and float(v.max()) < 1.0
        assert not torch.equal(v, plain[k]) and 0.45 < float(v.mean()) < 0.55
    assert len({float(v.sum()) for v in every.values()}) == 3                     # one map per primitive, not one shared
    picked = set()
    for step in range(24):
        got = _policy(1.0, 0.0).act(obs, keys=[(1, 2, step)])[0]
        kept = [k for k in got if torch.equal(got[k], plain[k])]
        assert len(kept) == 1
        picked.add(kept[0])
        for k in got:
            if k != kept[0]:
                assert got[k].shape == plain[k].shape and bool((got[k] == plain[kept[0]].min()).all())
    assert picked == {"fling", "drag", "place"}
    both = _policy(1.0, 1.0).act(obs, keys=[(9, 9, 9)])[0]                         # the fill uses the EXPLORED map's minimum
    kept = [k for k in both if float(both[k].max()) != float(both[k].min())]
    assert len(kept) == 1 and all(bool((both[k] == both[kept[0]].min()).all()) for k in both if k != kept[0])


def test_unkeyed_exploration_consumes_the_global_stream_as_before():
    """keys=None: one random.random() per primitive, one for the action coin, one random.choice when it falls."""
    gen = torch.Generator().manual_seed(6)
    obs = [torch.rand(4, 4, 16, 16, generator=gen) for _ in range(2)]
    policy = _policy(0.5, 0.5)
    random.seed(12)
    torch.manual_seed(12)
    got = policy.act(obs)
    after = random.random()
    # replay of the parent's statements on the same streams
    random.seed(12)
    torch.manual_seed(12)
    plain = _policy_maps_without_exploration(policy, obs)
    for e in range(2):
        maps = {k: (v if not 0.5 > random.random() else torch.rand(4, 16, 16)) for k, v in plain[e].items()}
        if 0.5 > random.random():
            name, chosen = random.choice(list(maps.items()))
            maps = {k: (v if k == name else torch.ones(v.size()) * chosen.min()) for k, v in maps.items()}
        assert _same(got[e], maps)
    assert random.random() == after


def _policy_maps_without_exploration(policy, obs):
    with torch.no_grad():
        return [{k: net(o).squeeze(1) for k, net in policy.value_nets.items()} for o in obs]
