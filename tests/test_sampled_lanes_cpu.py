"""The host side of sampled look-ahead lanes without a GPU: the sample key, the option checks of lookahead.run_episodes /
run_waves / train.run, and the command lines of evaluate and train."""
import numpy as np
import pytest


def test_sample_key_depends_on_seed_task_and_step_only():
    from flingbot_amd import lookahead

    key = lookahead.sample_key(3, 5, 1)
    want = np.random.SeedSequence([3, 5, 1, 0x5A]).generate_state(2, np.uint32)
    assert key.dtype == np.uint32 and key.shape == (2,) and np.array_equal(key, want)
    assert np.array_equal(key, lookahead.sample_key(3, 5, 1))
    others = [lookahead.sample_key(*k) for k in ((4, 5, 1), (3, 6, 1), (3, 5, 2))]
    assert all(not np.array_equal(key, o) for o in others)


def test_lane_options_are_checked():
    from flingbot_amd import lookahead

    lookahead.check_lanes("winners", 0.1, 0, None)
    lookahead.check_lanes("sampled", float("inf"), 0, 0)
    for bad in (("sampled", 0.1, 0, None), ("sampled", 0.0, 0, 1), ("sampled", float("nan"), 0, 1), ("sampled", 0.1, -1, 1),
                ("greedy", 0.1, 0, 1)):
        with pytest.raises(ValueError):
            lookahead.check_lanes(*bad)
    assert lookahead.lane_block("sampled", 0.25, 2) == dict(lanes="sampled", lane_temperature=0.25, refused=2)
    assert lookahead.lane_block("sampled", float("inf"), 0)["lane_temperature"] == "inf"


def test_evaluate_command_line():
    from flingbot_amd import evaluate

    ap = evaluate.build_parser()
    base = ["--tasks", "set.npz", "--slots", "8"]
    a = evaluate.parse_lookahead_options(ap, ap.parse_args(base + ["--lookahead", "4"]))
    assert a.lanes == "winners" and evaluate.lane_kwargs(a) == {}
    a = evaluate.parse_lookahead_options(ap, ap.parse_args(base + ["--lookahead", "4", "--lanes", "sampled", "--seed", "3",
                                                                   "--lane-temperature", "inf", "--lane-separation", "2",
                                                                   "--lanes-off-cloth", "--sample-first"]))
    assert evaluate.lane_kwargs(a) == dict(lanes="sampled", lane_temperature=float("inf"), lane_separation=2, lane_on_cloth=False,
                                           sample_first=True)
    for bad in (["--lanes", "sampled", "--seed", "3"], ["--lane-temperature", "0.5"], ["--sample-first"],   # no --lookahead
                ["--lookahead", "4", "--lanes", "sampled"],                                               # no --seed
                ["--lookahead", "4", "--lane-separation", "2"], ["--lookahead", "4", "--lanes-off-cloth"],  # not sampled
                ["--lookahead", "4", "--lanes", "sampled", "--seed", "3", "--lane-temperature", "0"],
                ["--lookahead", "4", "--lanes", "sampled", "--seed", "3", "--lane-separation", "-1"]):
        with pytest.raises(SystemExit):
            evaluate.parse_lookahead_options(ap, ap.parse_args(base + bad))


def test_train_command_line_and_run_refusals():
    from flingbot_amd import train

    ap = train.build_parser()
    a = ap.parse_args(["--tasks", "set.npz", "--log", "x", "--lookahead", "1", "--lanes", "sampled", "--sample-first"])
    assert a.lanes == "sampled" and a.sample_first and a.lane_temperature == 0.1
    for bad in (["--lanes", "sampled"], ["--lookahead", "2", "--sample-first"],
                ["--lookahead", "2", "--lanes", "sampled", "--lane-temperature", "-1"]):
        with pytest.raises(SystemExit):
            train.main(["--tasks", "set.npz", "--log", "x"] + bad)

    class Env:
        record_experience = True

    with pytest.raises(ValueError, match="lanes"):
        train.run(None, None, Env(), [dict()], "unused", 1, 1, 0, lanes="sampled")
