"""flingbot_amd.train without a GPU: `optimize` against a restatement of run_sim.optimize's loop, checkpoints,
ExperienceSet.extend, the argument checks of the fs_conv16_* entry points and the command line's flag names."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
D = 64
TASK = {"cloth_mass": 0.5, "flatten_area": 2.0, "task_difficulty": "hard", "initial_coverage": 0.5}
KW = dict(action_primitives=["fling"], num_rotations=12, scale_factors=[1.0, 1.25, 1.5, 1.75, 2.0, 2.25, 2.5, 2.75],
          obs_dim=64, pix_grasp_dist=8, pix_drag_dist=8, pix_place_dist=5, rgb_only=True, depth_only=False,
          action_expl_prob=0.5, action_expl_decay=0.9, value_expl_prob=0.25, value_expl_decay=0.9)


def _write_set(path, n, seed, first_episode=0, primitives=None, without_arrays=(), invalid=()):
    """A replay file of n one-action episodes; entry k may lack its arrays or carry a two-pixel (invalid) mask."""
    from flingbot_amd import taskio

    rng = np.random.default_rng(seed)
    records = []
    for k in range(n):
        obs = rng.random((4, D, D), dtype=np.float32)
        mask = np.zeros((D, D), bool)
        y, z = int(rng.integers(8, 56)), int(rng.integers(8, 56))
        mask[y, z] = True
        if k in invalid:
            mask[y, z + 1] = True
        pre, post = float(rng.random()), float(rng.random())
        arrays = dict(observations=obs, actions=mask, value_map=np.zeros((D, D), np.float32), max_indices=np.array([0, y, z]),
                      rotation=0.0, scale=1.0)
        records.append(dict(coverage=[pre, post], actions=[(primitives or ["fling"] * n)[k]], rewards=[post - pre],
                            preaction_coverage=[pre], experience=[None if k in without_arrays else arrays]))
    taskio.save_replay(path, records, [TASK] * n, first_episode=first_episode)


class HostSet:
    """ExperienceSet.sample for a machine without a GPU: the same draws, served by item_host."""

    def __init__(self, data):
        self.data = data

    def __len__(self):
        return len(self.data)

    def sample(self, batch_size, rng):
        idx, params = self.data.draw(batch_size, rng)
        obs, mask, label = self.data.item_host(idx, params)
        return torch.from_numpy(obs), torch.from_numpy(mask), torch.from_numpy(label)


def _policy(seed):
    from flingbot_amd import nets

    torch.manual_seed(seed)
    return nets.MaximumValuePolicy(device="cpu", **KW)


def _restated_loop(value_net, optimizer, batches):
    """What run_sim.optimize does with each (observation, mask, label) batch its loader yields, step by step."""
    losses = []
    for obs, mask, label in batches:
        dense = value_net(obs)
        picked = torch.masked_select(dense.squeeze(), mask)
        loss = torch.nn.functional.mse_loss(picked, label)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        value_net.steps += 1
        losses.append(loss.cpu().item())
    return losses


def _same_bits(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert sa[k].dtype == sb[k].dtype and torch.equal(sa[k], sb[k]), k


def test_optimize_equals_the_reference_loop(tmp_path):
    from flingbot_amd import replay, train

    path = str(tmp_path / "set.npz")
    _write_set(path, 6, seed=1)
    data = replay.ExperienceSet(path, action_primitive="fling")
    assert len(data) == 6 and data.jitters
    # the batches optimize will draw: same generator state, same calls
    rng = np.random.default_rng(11)
    batches = []
    for _ in range(3):
        idx, params = data.draw(4, rng)
        batches.append(tuple(torch.from_numpy(a) for a in data.item_host(idx, params)))

    mine, ref = _policy(3), _policy(3)
    _same_bits(mine, ref)
    opt_mine, opt_ref = train.make_optimizer(mine), train.make_optimizer(ref)
    assert len(opt_mine.param_groups) == 1 and len(opt_mine.param_groups[0]["params"]) == len(list(mine.parameters()))
    assert opt_mine.defaults["lr"] == 1e-3 and opt_mine.defaults["weight_decay"] == 1e-6
    mine.train(); ref.train()
    got = train.optimize("fling", mine.value_nets["fling"], opt_mine, HostSet(data), 3, 4, np.random.default_rng(11))
    want = _restated_loop(ref.value_nets["fling"], opt_ref, batches)
    mine.eval(); ref.eval()
    assert len(got) == 3 and got == want and all(np.isfinite(got))
    assert int(mine.value_nets["fling"].steps) == 3 == int(mine.steps())
    _same_bits(mine, ref)                     # parameters, BatchNorm buffers, steps
    fresh = _policy(3)
    moved = [k for k, v in mine.state_dict().items() if not torch.equal(v, fresh.state_dict()[k])]
    assert any(k.endswith("conv1.weight") for k in moved) and any(k.endswith("running_mean") for k in moved)


def test_optimize_does_nothing_below_one_batch(tmp_path):
    from flingbot_amd import replay, train

    path = str(tmp_path / "set.npz")
    _write_set(path, 3, seed=2)
    data = HostSet(replay.ExperienceSet(path))
    pol, fresh = _policy(4), _policy(4)
    opt = train.make_optimizer(pol)
    pol.train()
    assert train.optimize("fling", pol.value_nets["fling"], opt, data, 5, 4, np.random.default_rng(0)) == []
    assert train.optimize("fling", pol.value_nets["fling"], None, data, 5, 2, np.random.default_rng(0)) == []
    pol.eval()
    _same_bits(pol, fresh)
    assert len(opt.state_dict()["state"]) == 0


def test_checkpoint_round_trip(tmp_path):
    from flingbot_amd import replay, train

    path = str(tmp_path / "set.npz")
    _write_set(path, 6, seed=5)
    data = HostSet(replay.ExperienceSet(path))
    pol = _policy(6)
    opt = train.make_optimizer(pol, lr=2e-3, weight_decay=1e-5)
    pol.train()
    train.optimize("fling", pol.value_nets["fling"], opt, data, 2, 4, np.random.default_rng(1))
    pol.eval()
    pol.decay_exploration()
    ckpt_path = str(tmp_path / "latest_ckpt.pth")
    train.save_checkpoint(ckpt_path, pol, opt)

    ckpt = torch.load(ckpt_path, map_location="cpu")
    assert set(ckpt) == {"net", "optimizer"}
    with open(os.path.join(GOLD, "nets_state_dict_keys.json")) as fh:
        ref_keys = json.load(fh)
    assert list(ckpt["net"].keys()) == list(ref_keys.keys())
    assert {k: list(v.shape) for k, v in ckpt["net"].items()} == ref_keys
    assert set(ckpt["optimizer"]) == {"state", "param_groups"}
    assert len(ckpt["optimizer"]["param_groups"][0]["params"]) == len(list(pol.parameters()))

    other = _policy(99)                         # other weights, other probabilities
    other_opt = train.make_optimizer(other, lr=2e-3, weight_decay=1e-5)
    train.load_checkpoint(ckpt_path, other, other_opt)
    _same_bits(pol, other)
    assert float(other.action_expl_prob) == float(pol.action_expl_prob) == pytest.approx(0.45)
    assert int(other.steps()) == 2
    pol.train(); other.train()
    a = train.optimize("fling", pol.value_nets["fling"], opt, data, 2, 4, np.random.default_rng(2))
    b = train.optimize("fling", other.value_nets["fling"], other_opt, data, 2, 4, np.random.default_rng(2))
    pol.eval(); other.eval()
    assert a == b and len(a) == 2
    _same_bits(pol, other)                      # Adam's moments came along: the next updates give identical bits


def test_extend_equals_the_constructor_over_all_files(tmp_path):
    from flingbot_amd import replay

    paths = [str(tmp_path / f"replay_{k:05d}.npz") for k in range(3)]
    _write_set(paths[0], 4, seed=1, first_episode=0, primitives=["fling", "place", "fling", "fling"])
    _write_set(paths[1], 5, seed=2, first_episode=4, without_arrays=(1,), invalid=(3,))
    _write_set(paths[2], 3, seed=3, first_episode=9, primitives=["place", "fling", "fling"])
    for kwargs in (dict(action_primitive="fling"), dict(), dict(action_primitive="fling", rgb_only=False, use_normalized_coverage=False)):
        whole = replay.ExperienceSet(paths, **kwargs)
        grown = replay.ExperienceSet(paths[:1], **kwargs)
        assert grown.extend(paths[1]) == 3 and grown.extend(paths[2:]) == (2 if kwargs else 3)
        assert grown.keys == whole.keys and len(grown) == len(whole) == (8 if kwargs else 10)
        for name in ("observations", "masks", "labels"):
            a, b = getattr(grown, name), getattr(whole, name)
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), name
        for name in ("n_invalid", "n_without_arrays", "n_filtered"):
            assert getattr(grown, name) == getattr(whole, name), name
        assert whole.n_invalid == 1 and whole.n_without_arrays == 1 and whole.n_filtered == (2 if kwargs else 0)
        from_nothing = replay.ExperienceSet([], **kwargs)
        assert len(from_nothing) == 0 and from_nothing.extend(paths) == len(whole)
        assert from_nothing.keys == whole.keys and np.array_equal(from_nothing.observations, whole.observations)
        assert np.array_equal(from_nothing.labels, whole.labels) and from_nothing.labels.dtype == np.float32
        idx, params = whole.draw(5, np.random.default_rng(0))
        for x, y in zip(grown.item_host(idx, params), whole.item_host(idx, params)):
            assert np.array_equal(x, y)


def test_conv16_entry_points_refuse_what_they_do_not_serve():
    """dim = 32, batch = 0, a null pointer and a pointer 4 bytes off a 16-byte boundary: FS_ERR_ARG before any HIP call (this
    runs on a machine without a GPU; the pointers are host addresses that are never dereferenced)."""
    from flingbot_amd import sim as fsim

    lib = fsim.load_library()
    buf = np.zeros(1024, np.float32)
    base = (buf.ctypes.data + 63) // 64 * 64
    p, off, null = C.c_void_p(base), C.c_void_p(base + 4), C.c_void_p(None)
    ok_fwd = dict(x=p, w=p, transposed=0, batch=2, dim=64, y=C.c_void_p(base + 64))
    ok_wg = dict(x=p, g=p, batch=2, dim=64, dw=p, work=p)

    def fwd(**kw):
        a = {**ok_fwd, **kw}
        return lib.fs_conv16_forward(a["x"], a["w"], a["transposed"], a["batch"], a["dim"], a["y"], None)

    def wg(**kw):
        a = {**ok_wg, **kw}
        return lib.fs_conv16_wgrad(a["x"], a["g"], a["batch"], a["dim"], a["dw"], a["work"], None)

    bad = [dict(dim=32), dict(batch=0), dict(batch=-3)]
    for kw in bad + [dict(x=null), dict(w=null), dict(y=null), dict(x=off), dict(w=off), dict(y=off), dict(transposed=2)]:
        assert fwd(**kw) == -1, kw           # FS_ERR_ARG
        assert b"fs_conv16_forward" in lib.fs_last_error()
    for kw in bad + [dict(x=null), dict(g=null), dict(dw=null), dict(work=null), dict(x=off), dict(g=off), dict(dw=off), dict(work=off)]:
        assert wg(**kw) == -1, kw
        assert b"fs_conv16_wgrad" in lib.fs_last_error()
    assert lib.fs_conv16_work_bytes(0, 64) == 0 and lib.fs_conv16_work_bytes(3, 32) == 0
    assert lib.fs_conv16_work_bytes(3, 64) == 3 * 8 * 16 * 16 * 9 * 4


def test_parser_takes_the_reference_flag_names():
    from flingbot_amd import train

    ap = train.build_parser()
    a = ap.parse_args(["--log", "runs/a", "--tasks", "t.npz"])
    assert (a.seed, a.load, a.lr, a.batch_size, a.weight_decay) == (0, None, 1e-3, 128, 1e-6)
    assert (a.batches_per_update, a.update_frequency, a.warmup, a.save_ckpt) == (1, 1, 128, 512)
    assert (a.action_expl_prob, a.action_expl_decay, a.value_expl_prob, a.value_expl_decay) == (0.0, 0.9995, 0.0, 0.995)
    assert a.action_primitives == ["fling"]
    a = ap.parse_args("--log d --load c.pth --tasks t.npz --seed 4 --lr 0.01 --batch_size 8 --weight_decay 0 --batches_per_update 2 "
                      "--update_frequency 3 --warmup 16 --save_ckpt 64 --action_expl_prob 1 --action_expl_decay 0.5 "
                      "--value_expl_prob 0.75 --value_expl_decay 0.25 --action_primitives fling place --slots 12 --rounds 7 "
                      "--tasks-per-round 24".split())
    assert (a.log, a.load, a.tasks, a.seed, a.lr, a.batch_size, a.weight_decay) == ("d", "c.pth", "t.npz", 4, 0.01, 8, 0.0)
    assert (a.batches_per_update, a.update_frequency, a.warmup, a.save_ckpt) == (2, 3, 16, 64)
    assert (a.action_expl_prob, a.action_expl_decay, a.value_expl_prob, a.value_expl_decay) == (1.0, 0.5, 0.75, 0.25)
    assert a.action_primitives == ["fling", "place"] and (a.slots, a.rounds, a.tasks_per_round) == (12, 7, 24)
    with pytest.raises(SystemExit):
        ap.parse_args(["--tasks", "t.npz"])                      # --log is what a run is


def test_round_seed_is_a_function_of_seed_and_round():
    from flingbot_amd import train

    seen = {train.round_seed(s, r) for s in range(3) for r in range(4)}
    assert len(seen) == 12 and all(isinstance(v, int) and v >= 0 for v in seen)
    assert train.round_seed(1, 2) == train.round_seed(1, 2)


def test_deterministic_library_convs_touches_one_switch():
    """Inside the context the library is asked for deterministic algorithms and stays switched on; afterwards (also after an
    exception) the switch is what it was."""
    import torch
    from flingbot_amd import train

    enabled, before = torch.backends.cudnn.enabled, torch.backends.cudnn.deterministic
    with train.deterministic_library_convs():
        assert torch.backends.cudnn.deterministic is True and torch.backends.cudnn.enabled == enabled
    assert torch.backends.cudnn.deterministic == before
    with pytest.raises(KeyError):
        with train.deterministic_library_convs():
            raise KeyError
    assert torch.backends.cudnn.deterministic == before and torch.backends.cudnn.enabled == enabled
