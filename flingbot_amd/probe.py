"""Measured reward maps: a lattice of pick points of ONE value map executed from one identical state.

Look-ahead (flingbot_amd/lookahead.py) executes at most one action per rotation x scale map, because neighbouring pixels of
one map are near-copies of one action.  What the value net is trained to output, though, is the reward as a function of the
pixel INSIDE one map.  Here that function is measured: at the listed steps of an episode the map the policy chose from
(primitive p*, transform t*) is sampled on a lattice of stride `stride` that contains the chosen pixel,
`ActionSelector.lattice` (fs_lattice_actions) says which cells are valid actions and whether their grasp points are on cloth,
and every such cell is executed on a fork of the episode (`FlingSim.fork`) in a free slot of the context.  The episode itself
does not move while it is probed and then takes its own action through `env.step`: the followed trajectory is
evaluate.run_episodes' own.

What comes out, per (task, step): the predicted map next to the measured one on the lattice, rank statistics over all executed
cells (`map_stats`), and with BatchedFlingEnv(record_experience=True) one single-action record per executed cell in
lookahead.run_episodes' `lane_records` format -- lookahead.save_replay and replay.ExperienceSet take them unchanged, and a map
is one group for the ranking loss.
"""
import numpy as np
import torch


def lattice_axis(chosen, stride, g, D):
    """(origin, cells) of the lattice along one axis: origin = g + ((chosen - g) mod stride), as many cells as fit up to
    D - 1 - g -- the interior [g, D - 1 - g] fs_select_action indexes, so the chosen pixel is always a cell."""
    chosen, stride, g, D = int(chosen), int(stride), int(g), int(D)
    if stride < 1:
        raise ValueError(f"the probe stride must be at least 1, not {stride}")
    if not g <= chosen <= D - 1 - g:
        raise ValueError(f"pixel {chosen} is outside the interior [{g}, {D - 1 - g}]")
    origin = g + (chosen - g) % stride
    return origin, (D - 1 - g - origin) // stride + 1


def average_ranks(v):
    """1-based ranks of a float64 vector in ascending order, equal values sharing the mean of their positions."""
    v = np.asarray(v, np.float64)
    order = np.argsort(v, kind="stable")
    ranks = np.empty(len(v), np.float64)
    s = v[order]
    start = 0
    for k in range(1, len(v) + 1):
        if k == len(v) or s[k] != s[start]:
            ranks[order[start:k]] = 0.5 * (start + 1 + k)
            start = k
    return ranks


def map_stats(predicted, measured, chosen_cell, flatten_area):
    """The statistics of one map, float64 on the host, over the cells with finite `measured` (NaN = not executed) and finite
    `predicted`:
    chosen_reward / best_reward (as recorded), lattice_regret = (best - chosen) / flatten_area (>= 0; lookahead.summarize's
    unit), chosen_rank = the chosen cell's 0-based rank by measured reward, descending, ties to the chosen cell, spearman =
    Pearson correlation of the average ranks (None below 2 cells or at zero variance on either side), pairs / concordant =
    lookahead.pair_agreement's rule with min_gap 0: the ordered pairs (a, b) with measured_a > measured_b, and how many of them
    have predicted_a > predicted_b.  What needs the chosen cell is None when it is not among the counted cells."""
    p, r = np.asarray(predicted, np.float64), np.asarray(measured, np.float64)
    keep = np.isfinite(p) & np.isfinite(r)
    out = dict(n_cells=int(keep.sum()), chosen_reward=None, best_reward=None, lattice_regret=None, chosen_rank=None,
               spearman=None, pairs=0, concordant=0)
    if not keep.any():
        return out
    pv, rv = p[keep], r[keep]
    out["best_reward"] = float(rv.max())
    if chosen_cell is not None and keep[tuple(chosen_cell)]:
        chosen = float(r[tuple(chosen_cell)])
        out.update(chosen_reward=chosen, lattice_regret=(float(rv.max()) - chosen) / float(flatten_area),
                   chosen_rank=int((rv > chosen).sum()))
    if len(rv) >= 2:
        a, b = average_ranks(pv), average_ranks(rv)
        a, b = a - a.mean(), b - b.mean()
        den = np.sqrt((a * a).sum() * (b * b).sum())
        if den > 0:
            out["spearman"] = float((a * b).sum() / den)
    above = rv[:, None] > rv[None, :]
    out["pairs"] = int(above.sum())
    out["concordant"] = int((above & (pv[:, None] > pv[None, :])).sum())
    return out


def summarize(maps):
    """The means of a "probe" block over its maps: lattice_regret, chosen_rank and spearman over the maps that have one (None:
    no map has), pair_accuracy = concordant / pairs over all maps together, n_maps, n_executed."""
    def mean(key):
        v = [m["stats"][key] for m in maps if m["stats"][key] is not None]
        return float(np.mean(v)) if v else None
    pairs = int(sum(m["stats"]["pairs"] for m in maps))
    concordant = int(sum(m["stats"]["concordant"] for m in maps))
    return dict(lattice_regret=mean("lattice_regret"), chosen_rank=mean("chosen_rank"), spearman=mean("spearman"), pairs=pairs,
                concordant=concordant, pair_accuracy=concordant / pairs if pairs else None, n_maps=len(maps),
                n_executed=int(sum(m["n_executed"] for m in maps)))


def cell_ranks(predicted, executed):
    """{(i, j): rank} of the executed cells of one map: by predicted value descending (NaN last), flat cell index ascending."""
    cells = [tuple(int(v) for v in c) for c in np.argwhere(executed)]
    gz = executed.shape[1]
    key = lambda c: (not np.isfinite(predicted[c]), -float(predicted[c]) if np.isfinite(predicted[c]) else 0.0, c[0] * gz + c[1])  # noqa: E731
    return {c: k for k, c in enumerate(sorted(cells, key=key))}


def lane_records(maps, cells):
    """One single-action record per executed cell, in lookahead.run_episodes' lane_records format.  cells: per map
    {(i, j): dict(action, pre, post, reward, experience[, appearance])}."""
    out = []
    for m, done in zip(maps, cells):
        executed = np.zeros(np.shape(m["predicted"]), bool)
        for c in done:
            executed[c] = True
        ranks = cell_ranks(m["predicted"], executed)
        for c in sorted(done, key=lambda c: ranks[c]):
            d = done[c]
            out.append(dict(coverage=[d["pre"], d["post"]], actions=[d["action"]], rewards=[d["reward"]],
                            preaction_coverage=[d["pre"]], experience=[d["experience"]], task=int(m["task"]), step=int(m["step"]),
                            rank=ranks[c], **(dict(appearance=[d["appearance"]]) if "appearance" in d else {})))
    return out


def _empty_map(task, step):
    z = lambda dtype: np.zeros((0, 0), dtype)   # noqa: E731
    return dict(task=task, step=step, primitive=None, transform_index=-1, chosen_pixel=None, origin=None, shape=[0, 0],
                predicted=z(np.float32), valid=z(bool), on_cloth1=z(bool), on_cloth2=z(bool), measured=z(np.float32),
                terminated=z(bool), n_executed=0)


def _probe_step(env, run, stacks, value_maps, tasks_of, stride, skip_off_cloth, step, free, recording, looks, flat_of, draw=None):
    """The maps of one step for the running trunks `run`: select's action per trunk, ONE lattice call for all of them, then
    passes of ONE fork + ONE step_actions over as many cells as there are free slots.  The trunks are only read.
    draw: None, or (panel, the task indices to draw or None): the strips of those maps (report.compose_probe; after every
    pass ONE look_batch over the lanes that are the best of their map so far, ONE compose for all maps of the step).
    Returns (maps, cells, strips): the map entries, per map {(i, j): what a lane record needs}, {map index: strip}."""
    sel, sim = env.selector, env.sim
    g, D = sel.pix_grasp_dist, sel.obs_dim
    maps, cells, picked, requests = [], [], [], []
    for e in run:
        action, params = sel.select(value_maps[e], env.adaptive_scale_factors[e], env.pretransform_depth[e],
                                    depth_device=env.pretransform_depth_dev.get(e))
        if action is None:   # env.step settles such an episode and ends it; there is no map to probe
            maps.append(_empty_map(tasks_of[e], step))
            cells.append({})
            continue
        t, y, z = (int(v) for v in params["max_indices"])
        (y0, gy), (z0, gz) = lattice_axis(y, stride, g, D), lattice_axis(z, stride, g, D)
        if gy * gz > 4096:
            raise ValueError(f"a {gy} x {gz} lattice has more than 4096 cells: use a larger stride")
        requests.append((len(picked), sel.actions.index(action), t, y0, z0, stride, gy, gz))
        picked.append((e, len(maps), action))
        maps.append(dict(task=tasks_of[e], step=step, primitive=action, transform_index=t, chosen_pixel=[y, z], origin=[y0, z0],
                         shape=[gy, gz]))
        cells.append({})
    if not picked:
        return maps, cells, {}
    values = torch.stack([torch.stack(tuple(value_maps[e][a] for a in sel.actions)) for e, _, _ in picked])
    depth = torch.stack([env.pretransform_depth_dev[e].float() if env.pretransform_depth_dev.get(e) is not None
                         else torch.from_numpy(env.pretransform_depth[e]).to(values.device) for e, _, _ in picked])
    valid, on1, on2, value = sel.lattice(values, [env.adaptive_scale_factors[e] for e, _, _ in picked], depth, requests,
                                         env.conservative_grasp_radius)
    lanes = []   # (map index, cell, trunk, action, params)
    for k, (e, mi, action) in enumerate(picked):
        m = maps[mi]
        (y0, z0), (gy, gz), t = m["origin"], m["shape"], m["transform_index"]
        v, c1, c2 = valid[k, :gy, :gz].copy(), on1[k, :gy, :gz].copy(), on2[k, :gy, :gz].copy()
        chosen_cell = ((m["chosen_pixel"][0] - y0) // stride, (m["chosen_pixel"][1] - z0) // stride)
        for i, j in (tuple(c) for c in np.argwhere(v)):
            if skip_off_cloth and not (c1[i, j] or c2[i, j]) and (i, j) != chosen_cell:
                continue
            try:
                params = sel._candidate(action, t, y0 + i * stride, z0 + j * stride, env.adaptive_scale_factors[e],
                                        env.pretransform_depth[e])
            except ValueError:   # (zero depth under a grasp pixel)
                params = None
            if params is None:   # the host refuses what the device accepted: recorded as invalid, not executed
                v[i, j] = c1[i, j] = c2[i, j] = False
                continue
            params.update(p1_grasp_cloth=bool(c1[i, j]), p2_grasp_cloth=bool(c2[i, j]), value=float(value[k, i, j]),
                          transform_index=t)
            lanes.append((mi, (int(i), int(j)), e, action, params))
        m.update(predicted=value[k, :gy, :gz].copy(), valid=v, on_cloth1=c1, on_cloth2=c2,
                 measured=np.full((gy, gz), np.nan, np.float32), terminated=np.zeros((gy, gz), bool), n_executed=0,
                 chosen_cell=[int(chosen_cell[0]), int(chosen_cell[1])])
    if lanes and not free:
        raise ValueError("the probe executes its cells in free slots: the context has none beyond the tasks'")
    drawn = [mi for _, mi, _ in picked if draw is not None and (draw[1] is None or maps[mi]["task"] in draw[1])]
    best, afters = {}, {}
    for first in range(0, len(lanes), max(1, len(free))):
        batch = lanes[first:first + len(free)]
        src, dst = [lane[2] for lane in batch], free[:len(batch)]
        sim.fork(src, dst)
        for s, d in zip(src, dst):   # what the host keeps per episode
            env.prim.grasp_states[d] = list(env.prim.grasp_states[s])
            env.prim.terminate[d] = env.prim.terminate[s]
            env.timestep[d], env.terminate[d] = env.timestep[s], env.terminate[s]
        chosen = {d: (lane[3], lane[4]) for d, lane in zip(dst, batch)}
        experience = [None] * len(batch)
        if recording:   # every cell of a map shares its trunk's stack
            experience = env.gather_experience([(stacks[lane[2]], value_maps[lane[2]][lane[3]], lane[4]) for lane in batch])
        rewards, _ = env.step_actions(dst, chosen)
        for d, lane, exp in zip(dst, batch, experience):
            mi, cell, e, action, _ = lane
            maps[mi]["measured"][cell] = rewards[d]
            maps[mi]["terminated"][cell] = bool(env.terminate[d])
            maps[mi]["n_executed"] += 1
            pre, post = env.last_coverage[d]
            cells[mi][cell] = dict(action=action, pre=pre, post=post, reward=float(rewards[d]), experience=exp,
                                   **(dict(appearance=looks[e]) if e in looks else {}))
        better = {}   # the lanes of this pass that are their map's best so far (the first of equals stays)
        for d, lane in zip(dst, batch):
            if lane[0] in drawn and np.isfinite(rewards[d]) and (lane[0] not in best or rewards[d] > best[lane[0]]):
                best[lane[0]], better[lane[0]] = rewards[d], d
        if better:
            shown = env.look_batch(list(better.values()))
            afters.update({mi: shown[k].clone() for k, mi in enumerate(better)})
    strips = {}
    if drawn:
        from . import report
        trunk_of = {mi: (e, action) for e, mi, action in picked}
        items = []
        for mi in drawn:
            m, (e, action) = maps[mi], trunk_of[mi]
            t, flat = m["transform_index"], np.float32(flat_of[m["task"]])
            pix = report.transformed_pixels(action, [t] + m["chosen_pixel"], env.selector)
            items.append(dict(stack=stacks[e][t].to(env.device).float().contiguous(),
                              value_map=value_maps[e][action][t].float().contiguous(), predicted=m["predicted"],
                              measured=m["measured"] / flat, valid=m["valid"], range=None, origin=m["origin"], stride=stride,
                              chosen_cell=m["chosen_cell"], after=None if mi not in afters else afters[mi].contiguous(),
                              small=report.action_overlays(action, pix, thickness=1)))
        strips = dict(zip(drawn, report.compose_probe(items, panel=draw[0])))
    return maps, cells, strips


def run_episodes(policy, env, tasks, stride, steps=(0,), skip_off_cloth=True, max_steps=None, seed=None, fold=True, report=None):
    """evaluate.run_episodes, and at every episode step listed in `steps` the measured reward map of the map the policy
    chose from.  len(tasks) < env.sim.n_envs: task i runs in slot i, the remaining slots execute the cells.
    Before the trunks act at such a step: the policy's action (p*, t*, y*, z*) of every running episode (`select`'s), the
    lattice of stride `stride` through (y*, z*) on the interior of map (p*, t*) (`lattice_axis`), ONE ActionSelector.lattice
    call for all episodes, and every cell that is valid, confirmed by `_candidate` and -- unless skip_off_cloth is False --
    has at least one grasp point on cloth executed on a fork of its episode: a pass is ONE sim.fork plus ONE
    env.step_actions over as many cells of all episodes as there are free slots, further passes fork again from the untouched
    episodes.  The chosen cell is always executed.  Then `env.step` as ever.
    Returns every key of evaluate.run_episodes, equal to what it returns on the same tasks and seed (the simulation steps of
    the forks are counted apart, in probe["simulation_steps"]), plus "probe": dict(stride, steps_probed, maps, and
    summarize()'s means), maps = one entry per (task, probed step): task, step, primitive, transform_index, chosen_pixel,
    chosen_cell, origin, shape, predicted float32 [gy, gz], valid / on_cloth1 / on_cloth2 bool [gy, gz], measured float32
    [gy, gz] (the reward step_actions returned, NaN where not executed), terminated bool [gy, gz], n_executed, stats
    (`map_stats`).  An episode without a valid action has an empty map (shape [0, 0]).  With
    BatchedFlingEnv(record_experience=True) also "lane_records" in lookahead.run_episodes' format, one per executed cell, rank =
    the cell's order by predicted value descending, flat cell index ascending, among the executed cells of its map.
    report: None, or dict(panel=P, tasks=task indices or None, log=report.ActionLog or None): every probed map of those tasks
    is drawn (report.compose_probe: what the net saw with the chosen action | predicted map | measured map / flatten_area on its
    lattice, one colour range | the observation after the best-measured cell) and written through the log as
    <root>/episode{task:05d}/step{k:02d}_probe.png with one line in actions.jsonl (the lattice and `stats`); without a log the
    strips come back as "probe_panels" {(task, step): strip}.  Everything else the call returns is what it returns without."""
    if getattr(env, "dump_visualizations", False) or getattr(env, "action_report", False):
        raise ValueError("the probe neither films nor reports its lanes: dump_visualizations and action_report must be off")
    stride, wanted = int(stride), sorted({int(s) for s in steps})
    if stride < 1:
        raise ValueError(f"the probe stride must be at least 1, not {stride}")
    if fold:
        for net in policy.value_nets.values():
            if getattr(net, "_folded", None) is None:
                net.fold_batchnorm()
    randomized = getattr(env, "randomize_appearance", None) is not None
    first = int(getattr(policy, "first", 0))       # (run_waves: the tasks' indices in the whole set)
    if randomized:
        env.run_seed, env.appearance_task_offset = None if seed is None else int(seed), first
    obs = env.reset(tasks)
    envs = list(env.envs)
    free = [s for s in range(env.sim.n_envs) if s not in envs]
    flat = np.array([float(tasks[e]["flatten_area"]) for e in envs])
    cover = lambda: np.array(env.sim.coverage())[envs] / flat   # noqa: E731
    init = cover()
    trace = [init]
    recording = getattr(env, "record_experience", False)
    records = {e: dict(coverage=[float(c)], actions=[]) for e, c in zip(envs, np.array(env.sim.coverage())[envs])}
    lengths = np.zeros(len(envs), int)
    counts = {a: 0 for a in env.actions}
    probed, probed_cells, lane_sim_steps, panels = [], [], 0, {}
    draw = None
    if report is not None:
        draw = (int(report.get("panel", 200)), None if report.get("tasks") is None else {int(t) - first for t in report["tasks"]})
    steps_done = 0
    while obs and (max_steps is None or steps_done < max_steps):
        order = sorted(obs)
        looks = {e: env.last_appearance[e] for e in order} if randomized else {}
        with torch.no_grad():
            keys = None if seed is None else [(int(seed), envs.index(e), env.timestep[e]) for e in order]
            maps = policy.act([obs[e] for e in order], keep_on_device=True, keys=keys)
        value_maps = {e: {k: v.to(env.device) for k, v in m.items()} for e, m in zip(order, maps)}
        if steps_done in wanted:
            run = [e for e in order if not env.terminate[e]]
            counted = env.prim.sim_steps
            got, cells, strips = _probe_step(env, run, obs, value_maps, {e: envs.index(e) for e in run}, stride, skip_off_cloth,
                                             steps_done, free, recording, looks, flat, draw)
            lane_sim_steps += env.prim.sim_steps - counted
            env.prim.sim_steps = counted
            for m in got:
                m["stats"] = map_stats(m["predicted"], m["measured"], m.get("chosen_cell"), flat[m["task"]])
            for mi, strip in strips.items():
                _file_strip(got[mi], strip, first, None if report is None else report.get("log"), flat, panels)
            probed += got
            probed_cells += cells
        obs, rewards, terminate, actions = env.step(value_maps)
        for e, a in actions.items():
            lengths[envs.index(e)] += 1
            if a is not None:
                counts[a] += 1
            rec, (pre, post) = records[e], env.last_coverage[e]
            rec["coverage"].append(post)
            rec["actions"].append(a)
            rec.setdefault("rewards", []).append(rewards[e])
            rec.setdefault("preaction_coverage", []).append(pre)
            if recording:
                rec.setdefault("experience", []).append(env.last_experience[e])
            if randomized:
                rec.setdefault("appearance", []).append(looks[e])
        trace.append(cover())
        steps_done += 1
    trace = np.stack(trace)
    final = trace[-1]
    out = {
        "init_coverage": init, "final_coverage": final, "best_coverage": trace.max(axis=0),
        "episode_delta_coverage": final - init, "episode_length": lengths,
        "delta_coverage_steps": np.diff(trace, axis=0), "coverage_steps": trace, "action_primitive_counts": counts,
        "simulation_steps": int(env.prim.sim_steps), "visualization_dirs": {}, "records": [records[e] for e in envs],
        "mean": {"init_coverage": float(init.mean()), "final_coverage": float(final.mean()),
                 "best_coverage": float(trace.max(axis=0).mean()), "episode_delta_coverage": float((final - init).mean()),
                 "episode_length": float(lengths.mean())},
        "probe": dict(stride=stride, steps_probed=wanted, maps=probed, simulation_steps=int(lane_sim_steps), **summarize(probed)),
    }
    if recording:
        out["lane_records"] = lane_records(probed, probed_cells)
    if report is not None and report.get("log") is None:
        out["probe_panels"] = panels
    return out


def _file_strip(m, strip, first, log, flat, panels):
    """One probed map's strip: through the log to <root>/episode{first + task:05d}/step{k:02d}_probe.png and its line in
    actions.jsonl, or without one into panels[(task, step)]."""
    if log is None or log.root is None:
        panels[(m["task"], m["step"])] = strip
        return
    name = f"episode{first + m['task']:05d}"
    lists = lambda a: np.asarray(a).tolist()   # noqa: E731
    meta = dict(key=f"{name}_step{int(m['step']):02d}_probe", task=name, step=int(m["step"]), primitive=m["primitive"],
                probe=dict(transform_index=m["transform_index"], chosen_pixel=m["chosen_pixel"], chosen_cell=m["chosen_cell"],
                           origin=m["origin"], shape=m["shape"], n_executed=int(m["n_executed"]),
                           measured=[[None if np.isnan(v) else float(v) for v in row] for row in m["measured"]],
                           predicted=[[None if np.isnan(v) else float(v) for v in row] for row in m["predicted"]],
                           valid=lists(m["valid"])),
                stats=m["stats"], max_coverage=float(flat[m["task"]]))
    log.write(name, meta, strip, suffix="_probe")


def run_waves(policy, env, tasks, stride, steps=(0,), skip_off_cloth=True, max_steps=None, seed=None, report=None, trunks=None):
    """run_episodes over a task set of any length, in waves of `trunks` tasks (default: a quarter of the context's slots, at
    least one; the rest execute cells); the statistics of all tasks in task order, as lookahead.run_waves merges them, the
    maps' and records' task indices counted in the whole set.  The exploration key of task i stays (seed, i, step)."""
    from .lookahead import _ShiftedKeys
    n_envs = int(env.sim.n_envs)
    G = max(1, n_envs // 4) if trunks is None else int(trunks)
    if not 1 <= G < n_envs:
        raise ValueError(f"{G} episodes per wave leave no free slot of {n_envs} for the probe's lanes")
    parts = []
    for first in range(0, len(tasks), G):
        part = run_episodes(_ShiftedKeys(policy, first), env, tasks[first:first + G], stride, steps=steps, skip_off_cloth=skip_off_cloth,
                            max_steps=max_steps, seed=seed, report=report)
        for r in part.get("lane_records", ()):
            r["task"] += first
        for m in part["probe"]["maps"]:
            m["task"] += first
        parts.append(part)
    n = len(tasks)
    length = max(len(p["coverage_steps"]) for p in parts)
    trace = np.concatenate([np.concatenate([p["coverage_steps"], np.repeat(p["coverage_steps"][-1:], length - len(p["coverage_steps"]), 0)])
                            for p in parts], axis=1)
    init, final = trace[0], trace[-1]
    maps = [m for p in parts for m in p["probe"]["maps"]]
    out = {
        "init_coverage": init, "final_coverage": final, "best_coverage": trace.max(axis=0),
        "episode_delta_coverage": final - init, "episode_length": np.concatenate([p["episode_length"] for p in parts]),
        "delta_coverage_steps": np.diff(trace, axis=0), "coverage_steps": trace,
        "action_primitive_counts": {a: sum(p["action_primitive_counts"][a] for p in parts) for a in env.actions},
        "simulation_steps": int(sum(p["simulation_steps"] for p in parts)), "visualization_dirs": {},
        "records": [r for p in parts for r in p["records"]],
        "probe": dict(stride=int(stride), steps_probed=parts[0]["probe"]["steps_probed"], maps=maps,
                      simulation_steps=int(sum(p["probe"]["simulation_steps"] for p in parts)), **summarize(maps)),
    }
    out["mean"] = {"init_coverage": float(init.mean()), "final_coverage": float(final.mean()),
                   "best_coverage": float(trace.max(axis=0).mean()), "episode_delta_coverage": float((final - init).mean()),
                   "episode_length": float(out["episode_length"].mean())}
    if getattr(env, "randomize_appearance", None) is not None:
        env.appearance_task_offset = 0
    if all("lane_records" in p for p in parts):
        out["lane_records"] = [r for p in parts for r in p["lane_records"]]
    if all("probe_panels" in p for p in parts):
        out["probe_panels"] = {(first + t, k): strip for first, p in zip(range(0, n, G), parts) for (t, k), strip in p["probe_panels"].items()}
    return out


def save_maps(path, maps):
    """The arrays of a "probe" block's maps as one .npz: per map '<task:05d>_step<k:02d>/<name>' for predicted, measured, valid,
    on_cloth1, on_cloth2, terminated, plus 'lattice' = int64 [transform_index, y*, z*, y0, z0, gy, gz], and 'keys', 'stride'."""
    data, keys = {}, []
    for m in maps:
        key = f"{int(m['task']):05d}_step{int(m['step']):02d}"
        keys.append(key)
        for name in ("predicted", "measured", "valid", "on_cloth1", "on_cloth2", "terminated"):
            data[f"{key}/{name}"] = np.asarray(m[name])
        empty = m["primitive"] is None
        data[f"{key}/lattice"] = np.array([m["transform_index"]] + ([-1] * 4 if empty else m["chosen_pixel"] + m["origin"]) + m["shape"], np.int64)
    data["keys"] = np.array(keys)
    np.savez_compressed(path, **data)
    return len(keys)
