"""replay.MapSet, train.optimize_maps / train.fit_maps and the --fit-maps command line, the parts that need no GPU, on two
hand-made files written through lookahead.save_replay and taskio.save_replay:

  lanes.npz   map A  task 0 step 0   5 cells on one image, plus a 6th entry that repeats A's second pixel (dropped)
              map B  task 1 step 0   1 cell, primitive 'place'
              map C  task 0 step 1   4 cells on one image
              map D  task 1 step 1   3 cells with two DIFFERENT observations X, Y, X: two images of 2 and 1 pixels
  plain.npz   an episode of three steps -- a valid entry, one with two mask pixels, one without arrays -- and an episode of one
              step: 2 ordinary entries, with the SAME observation, which stay two images
"""
import json
import os

import numpy as np
import pytest
import torch

D = 64
TASKS = [dict(cloth_mass=0.5, flatten_area=2.0, task_difficulty="easy", initial_coverage=1.0),
         dict(cloth_mass=0.7, flatten_area=4.0, task_difficulty="hard", initial_coverage=1.2)]


def _image(seed):
    return np.random.default_rng(seed).random((4, D, D), dtype=np.float32)


def _arrays(pixels, image):
    mask = np.zeros((D, D), bool)
    for p in pixels:
        mask[p] = True
    return dict(observations=image, actions=mask, value_map=np.zeros((D, D), np.float32),
                max_indices=np.array([3, *pixels[0]], np.int64), rotation=10.0, scale=1.5)


def _cell(task, step, rank, pre, post, pixel, image, primitive="fling"):
    return dict(coverage=[pre, post], actions=[primitive], rewards=[post - pre], preaction_coverage=[pre],
                experience=[_arrays([pixel], image)], task=task, step=step, rank=rank)


A, B, C, X, Y, P = (_image(s) for s in range(6))
A_PIX = [(0, 0), (0, 1), (1, 0), (30, 31), (63, 63)]
C_PIX = [(8, 8), (8, 24), (24, 8), (24, 24)]
LANE_RECORDS = ([_cell(0, 0, r, 1.0, 1.0 + 0.1 * (r + 1), A_PIX[r], A) for r in range(5)]
                + [_cell(1, 0, 0, 1.2, 2.2, (20, 21), B, primitive="place")]
                + [_cell(0, 1, r, 1.5, 1.5 - 0.05 * r, C_PIX[r], C) for r in range(4)]
                + [_cell(0, 0, 5, 1.0, 1.9, A_PIX[1], A)]
                + [_cell(1, 1, 0, 1.3, 1.4, (40, 41), X), _cell(1, 1, 1, 1.3, 1.1, (42, 43), Y), _cell(1, 1, 2, 1.3, 1.7, (44, 45), X)])
PLAIN_RECORDS = [dict(coverage=[1.0, 1.5, 1.6, 1.7], actions=["fling"] * 3, rewards=[0.5, 0.1, 0.1], preaction_coverage=[1.0, 1.5, 1.6],
                      experience=[_arrays([(1, 2)], P), _arrays([(3, 4), (5, 6)], P), None]),
                 dict(coverage=[1.2, 2.2], actions=["fling"], rewards=[1.0], preaction_coverage=[1.2], experience=[_arrays([(5, 6)], P)])]
FLAT = lambda pixels: [y * D + x for y, x in pixels]   # noqa: E731
WANT_PIXELS = FLAT(A_PIX) + FLAT([(20, 21)]) + FLAT(C_PIX) + FLAT([(40, 41), (44, 45)]) + FLAT([(42, 43)]) + FLAT([(1, 2)]) + FLAT([(5, 6)])


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from flingbot_amd import lookahead, taskio

    d = tmp_path_factory.mktemp("maps")
    lanes, plain = str(d / "lanes.npz"), str(d / "plain.npz")
    assert lookahead.save_replay(lanes, dict(lane_records=LANE_RECORDS), TASKS) == 14
    assert taskio.save_replay(plain, PLAIN_RECORDS, TASKS, first_episode=100) == 4   # (keys apart from the lanes')
    return lanes, plain


def _same_sets(a, b):
    assert np.array_equal(a.images, b.images) and a.images.dtype == b.images.dtype == np.float32
    assert np.array_equal(a.offsets, b.offsets) and a.offsets.dtype == b.offsets.dtype == np.int64
    assert np.array_equal(a.pixels, b.pixels) and a.pixels.dtype == b.pixels.dtype == np.int32
    assert np.array_equal(a.labels.view(np.int32), b.labels.view(np.int32)) and a.labels.dtype == b.labels.dtype == np.float32
    assert a.entry_keys == b.entry_keys
    assert (a.n_duplicate, a.n_invalid, a.n_without_arrays, a.n_filtered) == (b.n_duplicate, b.n_invalid, b.n_without_arrays, b.n_filtered)


def _labels_of(paths, **kwargs):
    from flingbot_amd.replay import ExperienceSet

    entries = ExperienceSet(list(paths), **kwargs)
    assert len(set(entries.keys)) == len(entries.keys)
    return entries, dict(zip(entries.keys, entries.labels))


def test_images_pixels_and_labels(files):
    from flingbot_amd.replay import MapSet

    maps = MapSet(list(files), obs_color_jitter=False)
    assert len(maps) == 7 and maps.images.shape == (7, 4, D, D) and maps.images.dtype == np.float32
    for got, want in zip(maps.images, (A, B, C, X, Y, P, P)):          # in order of first appearance, each stored once
        assert np.array_equal(got, want)
    assert maps.offsets.dtype == np.int64 and maps.offsets.tolist() == [0, 5, 6, 10, 12, 13, 14, 15]
    assert maps.pixels.dtype == np.int32 and maps.pixels.tolist() == WANT_PIXELS
    assert maps.n_duplicate == 1 and maps.n_invalid == 1 and maps.n_without_arrays == 1 and maps.n_filtered == 0
    lane = lambda i: f"{i:09d}_step00_last"   # noqa: E731
    assert maps.entry_keys == ([lane(i) for i in range(10)] + [lane(11), lane(13), lane(12)]
                               + ["000000100_step00", "000000101_step00_last"])
    entries, label_of = _labels_of(files, obs_color_jitter=False)
    assert len(entries) == 16 and (entries.n_invalid, entries.n_without_arrays, entries.n_filtered) == (1, 1, 0)
    want = np.array([label_of[k] for k in maps.entry_keys], np.float32)
    assert maps.labels.dtype == np.float32 and np.array_equal(maps.labels.view(np.int32), want.view(np.int32))   # bit for bit
    assert np.array_equal(maps.labels[:2], np.array([0.1 / 2.0, (1.2 - 1.0) / 2.0], np.float64).astype(np.float32))
    # the min-max label form goes through the same code
    raw = MapSet(list(files), use_normalized_coverage=False)
    _, raw_of = _labels_of(files, use_normalized_coverage=False)
    assert np.array_equal(raw.labels.view(np.int32), np.array([raw_of[k] for k in raw.entry_keys], np.float32).view(np.int32))
    assert not np.array_equal(raw.labels, maps.labels)


def test_filters_act_as_in_experience_set(files):
    from flingbot_amd.replay import MapSet

    fling = MapSet(list(files), action_primitive="fling")
    entries, label_of = _labels_of(files, action_primitive="fling")
    assert len(fling) == 6 and fling.offsets.tolist() == [0, 5, 9, 11, 12, 13, 14] and fling.n_duplicate == 1
    assert (fling.n_filtered, fling.n_invalid, fling.n_without_arrays) == (entries.n_filtered, entries.n_invalid, entries.n_without_arrays) == (1, 1, 1)
    assert sorted(fling.entry_keys) == sorted(set(entries.keys) - {"000000010_step00_last"})      # all but the repeated pixel
    place = MapSet(list(files), action_primitive="place")
    assert len(place) == 1 and place.pixels.tolist() == [20 * D + 21] and place.n_filtered == 16 and place.n_invalid == 0
    assert np.array_equal(place.images[0], B)

    first = MapSet(list(files), lane_ranks=[0])
    entries, label_of = _labels_of(files, lane_ranks=[0])
    assert first.entry_keys == entries.keys and first.n_filtered == entries.n_filtered == 10 and first.n_duplicate == 0
    assert len(first) == 6 and first.offsets.tolist() == list(range(7))
    assert first.pixels.tolist() == FLAT([A_PIX[0], (20, 21), C_PIX[0], (40, 41), (1, 2), (5, 6)])
    assert np.array_equal(first.labels.view(np.int32), entries.labels.view(np.int32))
    rest = MapSet(list(files), lane_ranks=(1, 2))
    assert rest.offsets.tolist() == [0, 2, 4, 5, 6] and rest.pixels.tolist() == FLAT([A_PIX[1], A_PIX[2], C_PIX[1], C_PIX[2], (42, 43), (44, 45)])
    assert np.array_equal(rest.images[2], Y) and np.array_equal(rest.images[3], X)                # (Y appears first now)
    nothing = MapSet(list(files), action_primitive="drag")
    assert len(nothing) == 0 and nothing.offsets.tolist() == [0] and nothing.pixels.shape == (0,) and nothing.entry_keys == []


def test_extend_equals_building_at_once(files):
    from flingbot_amd.replay import MapSet

    lanes, plain = files
    at_once = MapSet([lanes, plain])
    grown = MapSet([lanes])
    assert len(grown) == 5 and grown.extend([plain]) == 2
    _same_sets(grown, at_once)
    from_nothing = MapSet([])
    assert len(from_nothing) == 0 and from_nothing.extend(lanes) == 5 and from_nothing.extend([plain]) == 2
    _same_sets(from_nothing, at_once)
    assert grown.extend([]) == 0
    # the same file twice is two files: an image never spans files
    twice = MapSet([lanes, lanes])
    assert len(twice) == 10 and twice.n_duplicate == 2 and twice.offsets.tolist() == [0, 5, 6, 10, 12, 13, 18, 19, 23, 25, 26]


def _restated_draw(maps, n, seed, pixels_per_image):
    """draw_maps as the class documents it, statement for statement."""
    from flingbot_amd.replay import draw_jitter

    rng = np.random.default_rng(seed)
    idx = rng.integers(0, len(maps), size=n)
    positions, offsets = [], [0]
    for i in idx:
        first, count = int(maps.offsets[i]), int(maps.offsets[i + 1] - maps.offsets[i])
        take = np.arange(count)
        if pixels_per_image is not None and count > pixels_per_image:
            take = np.sort(rng.choice(count, pixels_per_image, replace=False))
        positions += [first + int(t) for t in take]
        offsets.append(len(positions))
    params = draw_jitter(rng, n) if maps.jitters else None
    return idx, offsets, positions, params, rng


@pytest.mark.parametrize("pixels_per_image", [None, 2, 5, 64])
@pytest.mark.parametrize("jitter", [True, False])
def test_draw_maps_is_a_pure_function_of_the_rng(files, pixels_per_image, jitter):
    from flingbot_amd.replay import MapSet

    maps = MapSet(list(files), obs_color_jitter=jitter)
    n = 40
    rng = np.random.default_rng(9)
    idx, offsets, positions, params = maps.draw_maps(n, rng, pixels_per_image)
    again = maps.draw_maps(n, np.random.default_rng(9), pixels_per_image)
    want_idx, want_offsets, want_positions, want_params, want_rng = _restated_draw(maps, n, 9, pixels_per_image)
    assert np.array_equal(idx, want_idx) and np.array_equal(idx, again[0]) and idx.shape == (n,) and set(idx.tolist()) == set(range(7))
    assert offsets.tolist() == want_offsets and np.array_equal(offsets, again[1]) and offsets.shape == (n + 1,)
    assert positions.tolist() == want_positions and np.array_equal(positions, again[2])
    assert rng.bit_generator.state == want_rng.bit_generator.state                     # it took from the rng exactly that
    counts = np.diff(maps.offsets)[idx]
    limit = counts if pixels_per_image is None else np.minimum(counts, pixels_per_image)
    assert np.array_equal(np.diff(offsets), limit)
    for k, i in enumerate(idx):
        part = positions[offsets[k]:offsets[k + 1]]
        assert (np.diff(part) > 0).all() and part.min() >= maps.offsets[i] and part.max() < maps.offsets[i + 1]   # sorted subsets
    if jitter:      # one jitter per IMAGE
        assert params["order"].shape == (n, 4) and params["factors"].shape == (n, 4)
        assert np.array_equal(params["order"], want_params["order"]) and np.array_equal(params["factors"], want_params["factors"])
        assert np.array_equal(params["order"], again[3]["order"]) and np.array_equal(params["factors"], again[3]["factors"])
    else:
        assert params is None and want_params is None and again[3] is None
    if pixels_per_image == 2:     # the subsets differ from draw to draw
        a_parts = {tuple(positions[offsets[k]:offsets[k + 1]]) for k, i in enumerate(idx) if i == 0}
        assert len(a_parts) > 1 and all(len(p) == 2 for p in a_parts)


def test_draw_maps_refusals(files):
    from flingbot_amd.replay import MapSet

    with pytest.raises(ValueError):
        MapSet([]).draw_maps(2, np.random.default_rng(0))
    with pytest.raises(ValueError):
        MapSet(list(files)).draw_maps(2, np.random.default_rng(0), pixels_per_image=0)


@pytest.mark.parametrize("jitter", [True, False])
def test_sample_maps_on_the_host(files, jitter):
    from flingbot_amd.replay import MapSet, color_jitter_host

    maps = MapSet(list(files), obs_color_jitter=jitter)
    idx, offsets, positions, params = maps.draw_maps(6, np.random.default_rng(4), 3)
    obs, got_offsets, pix, labels = maps.sample_maps(6, np.random.default_rng(4), 3)
    want = maps.images[idx, :3]
    if jitter:
        want = color_jitter_host(want, params)
    assert obs.dtype == torch.float32 and tuple(obs.shape) == (6, 3, D, D) and np.array_equal(obs.numpy(), want)
    assert isinstance(got_offsets, np.ndarray) and np.array_equal(got_offsets, offsets)
    assert pix.dtype == torch.int32 and np.array_equal(pix.numpy(), maps.pixels[positions]) and np.array_equal(pix.host, maps.pixels[positions])
    assert labels.dtype == torch.float32 and np.array_equal(labels.numpy().view(np.int32), maps.labels[positions].view(np.int32))
    depth = MapSet(list(files), rgb_only=False, depth_only=True)
    obs, _, _, _ = depth.sample_maps(2, np.random.default_rng(4))
    assert tuple(obs.shape) == (2, 1, D, D)


def test_from_arrays_validates_the_table():
    from flingbot_amd.replay import MapSet

    images = np.zeros((2, 4, D, D), np.float32)
    maps = MapSet.from_arrays(images, [0, 2, 3], [5, 6, 5], [0.1, 0.2, 0.3])
    assert len(maps) == 2 and maps.offsets.tolist() == [0, 2, 3] and maps.labels.dtype == np.float32 and len(maps.entry_keys) == 3
    with pytest.raises(ValueError):
        MapSet.from_arrays(images, [0, 2, 3], [5, 5, 6], [0.1, 0.2, 0.3])


# ---- optimize_maps / fit_maps on a host policy --------------------------------------------------------------------------------
def _policy(primitives=("fling",)):
    from flingbot_amd import nets, train

    torch.manual_seed(3)
    policy = nets.MaximumValuePolicy(action_primitives=list(primitives), num_rotations=12, scale_factors=[1.0], obs_dim=64, pix_grasp_dist=8,
                                     pix_drag_dist=8, pix_place_dist=5, rgb_only=True, depth_only=False, action_expl_prob=0.0,
                                     action_expl_decay=1.0, value_expl_prob=0.0, value_expl_decay=1.0, device="cpu")
    return policy, train.make_optimizer(policy)


def test_optimize_maps_on_a_host_policy(files):
    from flingbot_amd import train
    from flingbot_amd.replay import MapSet

    policy, opt = _policy()
    net = policy.value_nets["fling"]
    maps = MapSet(list(files), action_primitive="fling")
    before = {k: v.clone() for k, v in net.state_dict().items()}
    policy.train()
    rows = []
    losses = train.optimize_maps("fling", net, opt, maps, 2, 3, np.random.default_rng(0), stats=rows)
    assert len(losses) == 2 and all(np.isfinite(losses)) and int(net.steps) == 2
    assert [r["loss"] for r in rows] == losses and all(r["images"] == 3 and 3 <= r["labels"] <= 15 for r in rows)
    assert set(rows[0]) == {"loss", "images", "labels"}
    changed = [k for k, v in net.state_dict().items() if not torch.equal(v, before[k])]
    assert len(changed) == len(before)
    # the first update, restated: the same batch, the dense forward gathered, mse over the labels
    policy2, _ = _policy()
    net2 = policy2.value_nets["fling"].train()
    obs, offsets, pix, label = maps.sample_maps(3, np.random.default_rng(0))
    image = np.repeat(np.arange(3), np.diff(offsets))
    with torch.no_grad():
        pred = net2(obs).squeeze(1).reshape(3, -1)[torch.from_numpy(image), pix.long()]
    assert losses[0] == float(torch.nn.functional.mse_loss(pred, label))
    # ranked: one segment per image
    rows = []
    ranked = train.optimize_maps("fling", net, opt, maps, 2, 3, np.random.default_rng(1), pixels_per_image=2, rank_weight=0.5, stats=rows)
    assert len(ranked) == 2 and set(rows[0]) == {"loss", "images", "labels", "mse", "rank", "pairs", "concordant"}
    assert all(r["labels"] <= 6 and 0 <= r["concordant"] <= r["pairs"] <= 3 for r in rows)     # at most one pair per image
    # fewer images than a batch: nothing happens
    assert train.optimize_maps("fling", net, opt, maps, 2, 7, np.random.default_rng(0)) == [] and int(net.steps) == 4
    assert train.optimize_maps("fling", net, None, maps, 2, 3, np.random.default_rng(0)) == []
    policy.eval()


def test_optimize_maps_refuses_ranking_without_a_fitting_pixels_per_image(files):
    from flingbot_amd import train
    from flingbot_amd.replay import MapSet

    policy, opt = _policy()
    net = policy.value_nets["fling"]
    maps = MapSet(list(files), action_primitive="fling")
    for kwargs in (dict(), dict(pixels_per_image=2000), dict(pixels_per_image=1366)):
        with pytest.raises(ValueError, match="4096"):
            train.optimize_maps("fling", net, opt, maps, 1, 3, np.random.default_rng(0), rank_weight=0.5, **kwargs)
    with pytest.raises(ValueError, match="4096"):       # refused up front, also where nothing would be done
        train.optimize_maps("fling", net, opt, maps, 1, 100, np.random.default_rng(0), rank_weight=0.5)
    for kwargs in (dict(rank_weight=-1.0), dict(rank_temperature=0.0), dict(rank_min_gap=float("nan")), dict(pixels_per_image=0)):
        with pytest.raises(ValueError):
            train.optimize_maps("fling", net, opt, maps, 1, 3, np.random.default_rng(0), **kwargs)
    assert int(net.steps) == 0


def test_fit_maps_files_and_log_lines(files, tmp_path):
    from flingbot_amd import train

    log = str(tmp_path / "run")
    policy, opt = _policy(("fling", "place"))
    out = train.fit_maps(policy, opt, list(files), log, 2, images_per_batch=3, seed=5)
    assert out["steps"] == 2 and out["primitives"]["fling"] == dict(images=6, labels=14, duplicates=1, updates=2,
                                                                    mean_loss=out["primitives"]["fling"]["mean_loss"])
    assert out["primitives"]["place"] == dict(images=1, labels=1, duplicates=0, updates=0, mean_loss=None)    # fewer images than a batch
    assert sorted(os.listdir(log)) == ["ckpt_000002.pth", "latest_ckpt.pth", "train_log.jsonl"]
    lines = [json.loads(l) for l in open(os.path.join(log, train.TRAIN_LOG))]
    assert len(lines) == 2 and [l["step"] for l in lines] == [1, 2]
    for l in lines:
        assert set(l) == {"fit", "primitive", "step", "loss", "images", "labels"} and l["fit"] is True and l["primitive"] == "fling"
        assert l["images"] == 3 and 3 <= l["labels"] <= 15 and np.isfinite(l["loss"])
    assert not policy.training
    # a second call resumes from latest_ckpt.pth, ranked this time
    policy2, opt2 = _policy(("fling", "place"))
    out = train.fit_maps(policy2, opt2, list(files), log, 1, images_per_batch=3, pixels_per_image=2, seed=5, rank_weight=0.5)
    assert out["steps"] == 3 and "ckpt_000003.pth" in os.listdir(log)
    lines = [json.loads(l) for l in open(os.path.join(log, train.TRAIN_LOG))]
    assert len(lines) == 3 and lines[2]["step"] == 3
    assert set(lines[2]) == {"fit", "primitive", "step", "loss", "images", "labels", "mse", "rank", "pairs", "pair_accuracy"}
    assert lines[2]["pair_accuracy"] is None or 0.0 <= lines[2]["pair_accuracy"] <= 1.0
    a = torch.load(os.path.join(log, "ckpt_000002.pth"))
    assert set(a) == {"net", "optimizer"}
    # the same call twice from scratch ends with the same bits
    logs = [str(tmp_path / "a"), str(tmp_path / "b")]
    for d in logs:
        policy, opt = _policy()
        train.fit_maps(policy, opt, list(files), d, 2, images_per_batch=3, seed=7)
    ca, cb = (torch.load(os.path.join(d, train.LATEST)) for d in logs)
    for k, v in ca["net"].items():
        assert torch.equal(v, cb["net"][k]), k


def test_command_line():
    from flingbot_amd import train

    ap = train.build_parser()
    with pytest.raises(SystemExit):
        ap.parse_args(["--log", "x"])                                   # without --fit-maps, --tasks is still demanded
    a = ap.parse_args(["--log", "x", "--tasks", "y"])
    assert a.fit_maps is None and a.tasks == "y" and a.updates == 500 and a.images_per_batch == 32 and a.pixels_per_image is None
    a = ap.parse_args(["--log", "x", "--fit-maps", "p.npz", "q.npz", "--updates", "7", "--images-per-batch", "4", "--pixels-per-image", "64",
                       "--hip-step", "--rank-weight", "0.5"])
    assert a.tasks is None and a.fit_maps == ["p.npz", "q.npz"] and (a.updates, a.images_per_batch, a.pixels_per_image) == (7, 4, 64)
    assert a.hip_step is True and a.rank_weight == 0.5
