"""Look-ahead rollouts: at every step the K best DIFFERENT actions of one observation are executed side by side, each on a
copy of the episode, and the episode continues from whichever copy is chosen.

The reference runs one cloth per process and can execute exactly one action per state (`env.step` ->
get_max_value_valid_action's single winner -> one delta coverage).  Here the episodes are slots of one context, so a
state can branch: `FlingSim.fork` (fs_fork) copies an episode into other slots bit for bit, `ActionSelector.candidates`
(fs_transform_winners) names the best valid action of every rotation x scale map -- neighbouring pixels of one map would
be K copies of one action -- and one lock-step `env.step_actions` call executes all of them.  What comes out:

  * regret: how far the net's arg-max was from the best of its own K candidates, per step, and the "oracle-of-K" coverage
    curve (`follow="best"`) that bounds what better ranking could buy;
  * K labels per observation from ONE identical state (`lane_records`), written by `save_replay` through
    taskio.save_replay, so that replay.ExperienceSet and taskio.collect_stats read the file as it is -- and
    train.run(lookahead=K) trains on them;
  * with BatchedFlingEnv(action_report=True) a picture of every step (report.compose_lanes, fs_lane_panels): the observation
    with all executed candidates on it next to the observation after each lane.

Slots: G = n_envs // k groups; the trunk of group g starts in slot g, its lanes are the slots g + j G.  The followed slot
becomes the trunk; nothing is copied back.
"""
import numpy as np
import torch

from . import nets


def group_slots(n_envs, k):
    """[[slots of group 0], [slots of group 1], ...]: G = n_envs // k groups of k slots, group g = {g + j G}."""
    n_envs, k = int(n_envs), int(k)
    if k < 1 or n_envs < k:
        raise ValueError(f"look-ahead with k = {k} needs at least k slots, the context has {n_envs}")
    G = n_envs // k
    return [[g + j * G for j in range(k)] for g in range(G)]


def choose_followed(rewards, follow):
    """The rank that is followed: "policy" -> 0, "best" -> the highest reward, ties to the lowest rank."""
    if follow == "policy" or len(rewards) == 0:
        return 0
    if follow != "best":
        raise ValueError(f"follow must be 'policy' or 'best', not {follow!r}")
    return int(max(range(len(rewards)), key=lambda j: (rewards[j], -j)))


def summarize(steps, flatten_areas, k):
    """The means of a "lookahead" block.  steps[i] = the step entries of task i (each {'candidates': [...], 'followed_rank'}),
    flatten_areas[i] its normalisation.  Over the steps that executed at least one candidate: regret = (best reward -
    rank-0 reward) / flatten_area (>= 0 by construction), rank0_best_frac = how often rank 0 had the best reward (ties
    count for rank 0), mean_reward_per_rank[j] = mean normalised reward of rank j over the steps that executed it (None:
    never executed); n_steps / n_lane_steps: the steps and executed lane-steps counted."""
    regrets, best0 = [], []
    by_rank = [[] for _ in range(int(k))]
    for entries, flat in zip(steps, flatten_areas):
        for entry in entries:
            r = [c["reward"] / float(flat) for c in entry["candidates"]]
            if not r:
                continue
            regrets.append(max(r) - r[0])
            best0.append(1.0 if r[0] >= max(r) else 0.0)
            for j, v in enumerate(r):
                by_rank[j].append(v)
    mean = lambda v: float(np.mean(v)) if len(v) else None   # noqa: E731
    return dict(regret=mean(regrets), rank0_best_frac=mean(best0), mean_reward_per_rank=[mean(v) for v in by_rank],
                n_steps=len(regrets), n_lane_steps=int(sum(len(v) for v in by_rank)))


def pair_agreement(steps, min_gap=0.0):
    """How often the net ordered two executed candidates of one observation the way their rewards did.  steps: a "lookahead"
    block's `steps` (per task, per step {'candidates': [{'value', 'reward', ...}, ...]}).  Over every ordered pair (a, b) of one
    step with reward_a > reward_b + min_gap (rewards as recorded), returns (pairs, concordant): their number and how many of
    them have value_a > value_b.  The pairs of trainops' ranking loss, counted on lanes the net has not trained on yet."""
    pairs = concordant = 0
    for entries in steps:
        for entry in entries:
            cands = entry["candidates"]
            for a in cands:
                for b in cands:
                    if float(a["reward"]) > float(b["reward"]) + float(min_gap):
                        pairs += 1
                        concordant += int(float(a["value"]) > float(b["value"]))
    return pairs, concordant


LANES = ("winners", "sampled")


def sample_key(seed, task, step):
    """The key of the draw at step `step` of task `task` (its index in the whole set): two uint32 words that depend on
    (seed, task, step) and on nothing else in the batch."""
    return np.random.SeedSequence([int(seed), int(task), int(step), 0x5A]).generate_state(2, np.uint32)


def check_lanes(lanes, lane_temperature, lane_separation, seed):
    """ValueError for lane options run_episodes cannot run with."""
    if lanes not in LANES:
        raise ValueError(f"lanes must be 'winners' or 'sampled', not {lanes!r}")
    if lanes != "sampled":
        return
    if seed is None:
        raise ValueError("lanes='sampled' draws from keys (seed, task, step): pass a seed")
    if not float(lane_temperature) > 0:
        raise ValueError(f"lane_temperature must be positive (inf: uniform), not {lane_temperature}")
    if int(lane_separation) < 0:
        raise ValueError(f"lane_separation must not be negative, not {lane_separation}")


def run_episodes(policy, env, tasks, k, follow="policy", max_steps=None, seed=None, fold=True, lanes="winners",
                 lane_temperature=0.1, lane_separation=0, lane_on_cloth=True, sample_first=False):
    """evaluate.run_episodes with k lanes per episode.  Per step: observe the trunks, ONE batched forward,
    `candidates(..., k)`, ONE fs_fork of every trunk into as many lanes as it has further candidates, ONE `step_actions`
    over all trunks and lanes (lane j executes candidate j, the trunk candidate 0; rewards from its one coverage() before
    and one after), then the followed slot becomes the trunk (`choose_followed`).  An episode without a valid candidate
    ends the way env.step ends it (the trunk settles and the "cloth did not move" test terminates it); otherwise it
    terminates when the followed lane did or episode_length is reached.
    len(tasks) <= env.sim.n_envs // k.  seed: as in evaluate.run_episodes (the key of step s of task i is (seed, i, s)).
    Returns every key of evaluate.run_episodes for the FOLLOWED trajectories -- with follow="policy" equal to
    evaluate.run_episodes' own on the same tasks -- plus "lookahead": dict(k, follow, steps = per task and step
    {'candidates': [{rank, primitive, transform_index, pixel, value, flat_index, reward, terminated}, ...],
    'followed_rank'}, and summarize()'s means), and with BatchedFlingEnv(record_experience=True) "lane_records": one
    single-action record per executed lane-step (coverage = [pre, post], actions, rewards, preaction_coverage, experience
    from env.gather_experience, task, step, rank).
    With BatchedFlingEnv(action_report=True, report_root=DIR, report_panel=P, report=task indices or None) every step that
    executed a candidate is drawn (`_report_step`: one look_batch over the executed lane slots after step_actions, before the
    next step's appearance draw, and ONE report.compose_lanes for all groups) into DIR/episode{task index:05d}/
    step{k:02d}_lanes.png with one line in DIR/actions.jsonl; without a report_root the strips come back as "lane_panels"
    {task: [strip per drawn step]}.  Everything else the call returns is what it returns with the report off.  Films of
    lanes are refused.
    lanes: which k actions of an observation are executed.  "winners": the best winners of its rotation x scale maps
    (`candidates`).  "sampled": k different valid actions drawn with probability ~ exp(value / lane_temperature) over all
    primitives x transforms x pixels (`ActionSelector.sampled`, fs_sample_actions), with the key `sample_key(seed, task index in
    the whole set, step)` -- a seed is required --, their grasp points on cloth unless lane_on_cloth is False, two lanes of one
    primitive more than lane_separation pretransform pixels apart; candidate 0 is the net's arg-max (so follow="policy" still
    equals evaluate.run_episodes) unless sample_first, which draws it as well (k = 1: Boltzmann exploration).  The "lookahead"
    block then also holds lanes, lane_temperature ("inf" for a uniform draw) and refused (device picks the host's validation
    dropped), every candidate its 'sample_key' (the perturbed key it was drawn with) and 'grasp_cloth' (the two flags it was
    executed with)."""
    if follow not in ("policy", "best"):
        raise ValueError(f"follow must be 'policy' or 'best', not {follow!r}")
    check_lanes(lanes, lane_temperature, lane_separation, seed)
    sampling = lanes == "sampled"
    if getattr(env, "dump_visualizations", False):
        raise ValueError("look-ahead does not film its lanes: dump_visualizations must be off")
    refused_before = env.selector.sample_refused if sampling else 0
    sim, k = env.sim, int(k)
    reporting = bool(getattr(env, "action_report", False))
    if reporting and k > 8:
        raise ValueError(f"a lane strip shows at most 8 lanes (fs_lane_panels), k = {k}")
    groups = group_slots(sim.n_envs, k)
    if len(tasks) > len(groups):
        raise ValueError(f"{len(tasks)} tasks need {len(tasks) * k} slots for k = {k}, the context has {sim.n_envs}")
    if fold:
        for net in policy.value_nets.values():
            if getattr(net, "_folded", None) is None:
                net.fold_batchnorm()
    randomized = getattr(env, "randomize_appearance", None) is not None
    first = int(getattr(policy, "first", 0))       # (run_waves: the tasks' indices in the whole set)
    if randomized:   # a lane inherits its trunk's appearance through fs_fork and draws from the trunk's key next time
        env.run_seed, env.appearance_task_offset = None if seed is None else int(seed), first
    n = len(tasks)
    wanted, before, lane_panels = [], {}, {}
    if reporting:   # env.report names TASK indices here; the reset keeps the first observation of every slot it fills
        wanted = [i for i in range(n) if env.report is None or first + i in env.report]
        listed, env.report = env.report, None
    try:
        stacks = env.reset(tasks)                  # task i in slot i = the trunk of group i
    finally:
        if reporting:
            env.report = listed
    if reporting:   # from here on the observations a strip needs are kept below, per task
        before = {i: env._report_obs[i] for i in wanted}
        env._report_names, env._report_obs = {}, {}
        lane_panels = {i: [] for i in wanted}
    trunk = list(range(n))
    flat = np.array([float(tasks[i]["flatten_area"]) for i in range(n)])
    cover = lambda: np.array(sim.coverage())[trunk] / flat   # noqa: E731
    init = cover()
    trace = [init]
    recording = getattr(env, "record_experience", False)
    records = [dict(coverage=[float(c)], actions=[]) for c in np.array(sim.coverage())[trunk]]
    lane_records, look_steps = [], [[] for _ in range(n)]
    lengths = np.zeros(n, int)
    counts = {a: 0 for a in env.actions}
    done = [False] * n
    steps = 0
    while not all(done) and (max_steps is None or steps < max_steps):
        run = [i for i in range(n) if not done[i]]
        looks = {i: env.last_appearance[trunk[i]] for i in run} if randomized else {}   # what this step's observations show
        with torch.no_grad():
            keys = None if seed is None else [(int(seed), i, env.timestep[trunk[i]]) for i in run]
            maps = policy.act([stacks[trunk[i]] for i in run], keep_on_device=True, keys=keys)
        maps = [{a: v.to(env.device) for a, v in m.items()} for m in maps]
        where = ([env.adaptive_scale_factors[trunk[i]] for i in run], [env.pretransform_depth[trunk[i]] for i in run])
        on_device = [env.pretransform_depth_dev.get(trunk[i]) for i in run]
        if sampling:
            cands = env.selector.sampled(maps, *where, k, [sample_key(seed, first + i, steps) for i in run], lane_temperature,
                                         on_cloth=lane_on_cloth, separation=lane_separation, first_greedy=not sample_first,
                                         depth_device=on_device, radius=env.conservative_grasp_radius)
        else:
            cands = env.selector.candidates(maps, *where, k, depth_device=on_device)
        # lanes: candidate 0 stays in the trunk, candidate j goes to the j-th free slot of the group
        lanes, src, dst, chosen = {}, [], [], {}
        for i, found in zip(run, cands):
            free = [s for s in groups[i] if s != trunk[i]]
            lanes[i] = [trunk[i]] + free[:max(0, len(found) - 1)]
            src += [trunk[i]] * (len(lanes[i]) - 1)
            dst += lanes[i][1:]
            depth = env.pretransform_depth[trunk[i]]
            for slot, (action, params) in zip(lanes[i], found):
                pix = params["pretransform_pixels"]
                params["p1_grasp_cloth"] = env._on_cloth(depth, (pix[0][1], pix[0][0]))
                params["p2_grasp_cloth"] = env._on_cloth(depth, (pix[1][1], pix[1][0]))
                chosen[slot] = (action, params)
        if dst:
            sim.fork(src, dst)
            for s, d in zip(src, dst):   # what the host keeps per episode
                env.prim.grasp_states[d] = list(env.prim.grasp_states[s])
                env.prim.terminate[d] = env.prim.terminate[s]
                env.timestep[d], env.terminate[d] = env.timestep[s], env.terminate[s]
        slots = [s for i in run for s in lanes[i]]
        experience = {}
        if recording:   # before the action; every lane of a group shares its trunk's stack
            items = [(s, i) for i in run for s in lanes[i] if s in chosen]
            got = env.gather_experience([(stacks[trunk[i]], maps[run.index(i)][chosen[s][0]], chosen[s][1]) for s, i in items])
            experience = {s: g for (s, _), g in zip(items, got)}
        rewards, acted = env.step_actions(slots, chosen)
        for pos, i in enumerate(run):
            found = cands[pos]
            entries = []
            for rank, slot in enumerate(lanes[i][:max(1, len(found))]):
                if slot not in chosen:
                    break
                action, params = chosen[slot]
                pre, post = env.last_coverage[slot]
                entries.append(dict(rank=rank, primitive=action, transform_index=int(params["transform_index"]),
                                    pixel=[int(params["max_indices"][1]), int(params["max_indices"][2])],
                                    value=float(params["value"]), flat_index=int(params["flat_index"]),
                                    reward=float(rewards[slot]), terminated=bool(env.terminate[slot])))
                if sampling:
                    entries[-1].update(sample_key=float(params["sample_key"]),
                                       grasp_cloth=[bool(params["p1_grasp_cloth"]), bool(params["p2_grasp_cloth"])])
                if recording:
                    lane_records.append(dict(coverage=[pre, post], actions=[action], rewards=[float(rewards[slot])],
                                             preaction_coverage=[pre], experience=[experience[slot]], task=i, step=steps,
                                             rank=rank, **(dict(appearance=[looks[i]]) if randomized else {})))
            followed = choose_followed([c["reward"] for c in entries], follow)
            look_steps[i].append(dict(candidates=entries, followed_rank=followed))
            slot = lanes[i][followed]
            trunk[i] = slot
            action = acted[slot]
            lengths[i] += 1
            if action is not None:
                counts[action] += 1
            rec, (pre, post) = records[i], env.last_coverage[slot]
            rec["coverage"].append(post)
            rec["actions"].append(action)
            rec.setdefault("rewards", []).append(rewards[slot])
            rec.setdefault("preaction_coverage", []).append(pre)
            if recording:
                rec.setdefault("experience", []).append(experience.get(slot))
            if randomized:
                rec.setdefault("appearance", []).append(looks[i])
            done[i] = bool(env.terminate[slot])
        if reporting:   # before the next step's appearance draw: a lane shows the appearance its step's observation had
            shown = [i for i in run if i in before and look_steps[i][-1]["candidates"]]
            _report_step(env, k, first, steps, shown, {i: lanes[i][:len(look_steps[i][-1]["candidates"])] for i in shown},
                         chosen, {i: look_steps[i][-1] for i in shown}, before, flat, lane_panels)
        trace.append(cover())
        steps += 1
        live = [trunk[i] for i in range(n) if not done[i]]
        if live and (max_steps is None or steps < max_steps):
            if randomized:
                env.randomize({trunk[i]: first + i for i in range(n) if not done[i]})
            obs = env.get_obs_batch(live)
            stacks = {e: nets.prepare_image(obs[j], env.get_transformations(e), env.obs_dim) for j, e in enumerate(live)}
            if reporting:
                for j, e in enumerate(live):
                    if trunk.index(e) in before:
                        before[trunk.index(e)] = obs[j, :3].clone()   # (a view would keep the whole batch alive)
    trace = np.stack(trace)
    final = trace[-1]
    out = {
        "init_coverage": init, "final_coverage": final, "best_coverage": trace.max(axis=0),
        "episode_delta_coverage": final - init, "episode_length": lengths,
        "delta_coverage_steps": np.diff(trace, axis=0), "coverage_steps": trace, "action_primitive_counts": counts,
        "simulation_steps": int(env.prim.sim_steps), "visualization_dirs": {}, "records": records,
        "mean": {"init_coverage": float(init.mean()), "final_coverage": float(final.mean()),
                 "best_coverage": float(trace.max(axis=0).mean()), "episode_delta_coverage": float((final - init).mean()),
                 "episode_length": float(lengths.mean())},
        "lookahead": dict(k=k, follow=follow, steps=look_steps, **summarize(look_steps, flat, k)),
    }
    if sampling:
        out["lookahead"].update(lane_block("sampled", lane_temperature, env.selector.sample_refused - refused_before))
    if recording:
        out["lane_records"] = lane_records
    if reporting and getattr(env, "report_root", None) is None:   # (without a directory the caller keeps the strips)
        out["lane_panels"] = lane_panels
    return out


def lane_block(lanes, lane_temperature, refused):
    """What a "lookahead" block says about sampled lanes (JSON has no infinity: a uniform draw is "inf")."""
    t = float(lane_temperature)
    return dict(lanes=lanes, lane_temperature=t if np.isfinite(t) else "inf", refused=int(refused))


def _report_step(env, k, first, step, shown, slots, chosen, entries, before, flat, lane_panels):
    """The lane strips of one step for the tasks `shown` (indices within the call): ONE look_batch over their executed lane
    slots (slots[i], in rank order) -- the RGB planes and nothing else, so that the episodes' bookkeeping is what it is without
    a report --, ONE report.compose_lanes for all of them, then per task <root>/episode{first + i:05d}/step{step:02d}_lanes.png
    and its line in actions.jsonl, or without a root the strip into lane_panels[i]."""
    from . import report
    if not shown:
        return
    order = [s for i in shown for s in slots[i]]
    looks = env.look_batch(order)
    items = []
    for i in shown:
        lanes = [dict(after=looks[order.index(s)], prims=report.action_overlays(chosen[s][0], chosen[s][1]["pretransform_pixels"], thickness=3))
                 for s in slots[i]]
        items.append(dict(before=before[i], lanes=lanes, followed=entries[i]["followed_rank"]))
    strips = report.compose_lanes(items, k, panel=env.report_panel)
    log = getattr(env, "_report_log", None)
    for i, strip in zip(shown, strips):
        if log is None or log.root is None:
            lane_panels[i].append(strip)
            continue
        entry, name = entries[i], f"episode{first + i:05d}"
        pre = env.last_coverage[slots[i][0]][0]
        post = env.last_coverage[slots[i][entry["followed_rank"]]][1]
        keep = ("rank", "primitive", "transform_index", "pixel", "value", "reward", "terminated")
        meta = dict(key=f"{name}_step{int(step):02d}_lanes", task=name, step=int(step),
                    lanes=[{f: c[f] for f in keep} for c in entry["candidates"]], followed_rank=int(entry["followed_rank"]),
                    preaction_coverage=float(pre), postaction_coverage=float(post), max_coverage=float(flat[i]))
        log.write(name, meta, strip, suffix="_lanes")


def expand_tasks(lane_records, tasks):
    """The task of every lane record, in order: what taskio.save_replay wants next to a list of records."""
    return [tasks[int(r["task"])] for r in lane_records]


def save_replay(path, stats, tasks, first_record=0):
    """The lane records of run_episodes / run_waves (`stats["lane_records"]`; BatchedFlingEnv(record_experience=True)) as a
    replay file, through taskio.save_replay with the task list expanded per record: every executed lane-step is a one-action
    episode '<first_record + record number>_step00_last' whose pre / post coverage, reward and training arrays are its own,
    so replay.ExperienceSet and taskio.collect_stats read the file as it is.  Where a label came from travels with it as
    '<key>/lane_task', '/lane_step', '/lane_rank' and '/lane_followed' (1 for the lane the episode continued from).
    first_record: the records written before this file (train.run: the entries of the rounds before), so that keys stay unique
    over a run.  Returns the number of entries written."""
    from . import taskio
    if "lane_records" not in stats:
        raise ValueError("no lane records: run with BatchedFlingEnv(record_experience=True)")
    recs = stats["lane_records"]
    look = stats.get("lookahead", {}).get("steps")
    tagged = []
    for r in recs:
        extra = dict(lane_task=int(r["task"]), lane_step=int(r["step"]), lane_rank=int(r["rank"]))
        if look is not None:   # (records made by hand carry no statistics: where they came from is all that is known)
            extra["lane_followed"] = int(look[int(r["task"])][int(r["step"])]["followed_rank"] == int(r["rank"]))
        tagged.append(dict(r, extra=extra))
    return taskio.save_replay(path, tagged, expand_tasks(recs, tasks), first_episode=int(first_record))


def run_waves(policy, env, tasks, k, follow="policy", max_steps=None, seed=None, lanes="winners", lane_temperature=0.1,
              lane_separation=0, lane_on_cloth=True, sample_first=False):
    """run_episodes over a task set of any length, in waves of G = n_envs // k tasks; the statistics of all tasks in task
    order (a shorter episode's coverage is carried to the longest one's length, as evaluate.run_tasks does).  The exploration
    key of task i stays (seed, i, step), and so does its sample key (lanes="sampled": run_episodes' lane options)."""
    check_lanes(lanes, lane_temperature, lane_separation, seed)
    lane_options = dict(lanes=lanes, lane_temperature=lane_temperature, lane_separation=lane_separation,
                        lane_on_cloth=lane_on_cloth, sample_first=sample_first)
    G = len(group_slots(env.sim.n_envs, k))
    parts = []
    for first in range(0, len(tasks), G):
        wave = tasks[first:first + G]
        # (the keys count within the call: shift the seed's task index by running the wave with keys of its own)
        part = run_episodes(_ShiftedKeys(policy, first), env, wave, k, follow=follow, max_steps=max_steps, seed=seed,
                            **lane_options)
        for r in part.get("lane_records", ()):
            r["task"] += first
        parts.append(part)
    n = len(tasks)
    steps = max(len(p["coverage_steps"]) for p in parts)
    trace = np.concatenate([np.concatenate([p["coverage_steps"], np.repeat(p["coverage_steps"][-1:], steps - len(p["coverage_steps"]), 0)])
                            for p in parts], axis=1)
    init, final = trace[0], trace[-1]
    counts = {a: sum(p["action_primitive_counts"][a] for p in parts) for a in env.actions}
    look = [s for p in parts for s in p["lookahead"]["steps"]]
    flat = np.array([float(tasks[i]["flatten_area"]) for i in range(n)])
    out = {
        "init_coverage": init, "final_coverage": final, "best_coverage": trace.max(axis=0),
        "episode_delta_coverage": final - init, "episode_length": np.concatenate([p["episode_length"] for p in parts]),
        "delta_coverage_steps": np.diff(trace, axis=0), "coverage_steps": trace, "action_primitive_counts": counts,
        "simulation_steps": int(sum(p["simulation_steps"] for p in parts)), "visualization_dirs": {},
        "records": [r for p in parts for r in p["records"]],
        "lookahead": dict(k=int(k), follow=follow, steps=look, **summarize(look, flat, k)),
    }
    out["mean"] = {"init_coverage": float(init.mean()), "final_coverage": float(final.mean()),
                   "best_coverage": float(trace.max(axis=0).mean()), "episode_delta_coverage": float((final - init).mean()),
                   "episode_length": float(out["episode_length"].mean())}
    if lanes == "sampled":
        out["lookahead"].update(lane_block(lanes, lane_temperature, sum(p["lookahead"]["refused"] for p in parts)))
    if getattr(env, "randomize_appearance", None) is not None:
        env.appearance_task_offset = 0
    if all("lane_records" in p for p in parts):
        out["lane_records"] = [r for p in parts for r in p["lane_records"]]
    if all("lane_panels" in p for p in parts):
        out["lane_panels"] = {first + i: strips for first, p in zip(range(0, n, G), parts) for i, strips in p["lane_panels"].items()}
    return out


class _ShiftedKeys:
    """A policy whose exploration keys (seed, task index within the call, step) name the task by its index in the whole set."""

    def __init__(self, policy, first):
        self.policy, self.first = policy, int(first)
        self.value_nets = policy.value_nets

    def act(self, obs, keep_on_device=False, keys=None):
        if keys is not None:
            keys = [(s, i + self.first, t) for s, i, t in keys]
        return self.policy.act(obs, keep_on_device=keep_on_device, keys=keys)
