"""BatchedFlingEnv -- SimEnv.reset / step (environment/simEnv.py:477-515, 663-697) for many episodes on one GPU.

Composition of the device-side pieces of this package, one call per stage for ALL episodes where the stage allows it:
    tasks.load_tasks + FlingPrimitives.setup_pickers          SimEnv.reset           (simEnv.py:663-697)
    fs_render -> preprocess_obs -> fs_prepare_image           get_obs / prepare_image (simEnv.py:709-737, nets.py:177-193)
    ActionSelector.select (fs_select_action)                  get_max_value_valid_action (simEnv.py:560-661)
    FlingPrimitives.pick_and_fling / drag / place / stretchdrag   the action handlers  (simEnv.py:283-428)
    preaction / postaction, coverage                          SimEnv.step            (simEnv.py:464-515)
The observation stage (get_image's cv2.resize of the 720 x 720 render, the HSV cloth mask, its largest connected
component and the adaptive scale SimEnv.get_obs derives from it, simEnv.py:699-737) runs on the device in fs_observe
(csrc/fs_observe.hip); it follows OpenCV's / skimage's documented algorithms (oracle/observe.py) -- cv2 and skimage are
absent from this image, so that boundary is NOT pinned to the reference's own build.
The grasp-on-cloth flags (simEnv.py:235-255) test `depth != 2.0` on a Euclidean disc of conservative_grasp_radius, which
is pixel for pixel the filled cv2.circle (OpenCV's midpoint fill) for radii up to 6; the reference's default is 1.
Every other stage is pinned on its own in tests/ (see DESIGN.md section 2 and 4.3-4.8).
"""
import numpy as np
import torch

from . import nets
from .action import ActionSelector
from .primitives import FlingPrimitives
from .tasks import load_task_scene, load_task_state, load_tasks


class BatchedFlingEnv:
    def __init__(self, sim, action_primitives=("fling",), obs_dim=64, image_dim=400, num_rotations=12,
                 scale_factors=(1.0, 1.25, 1.5, 1.75, 2.0, 2.25, 2.5, 2.75), pix_grasp_dist=8, pix_drag_dist=8, pix_place_dist=5,
                 reach_distance_limit=1.2, conservative_grasp_radius=1, episode_length=10, grasp_height=0.02,
                 fling_speed=6e-3, stretchdrag_dist=0.3, device="cuda:0", render_dim=720, use_adaptive_scaling=True,
                 scheduled=True, dump_visualizations=False, visualize=None, frame_size=(720, 720), visualization_root=None,
                 record_experience=False, action_report=False, report_root=None, report_panel=200, report=None,
                 randomize_appearance=None, appearance_seed=None):
        """record_experience: keep, for every action that was actually chosen, what SimEnv.log_step_stats stores for the
        training set (simEnv.py:434-452, 597-608): entry x of the transformed stack the policy saw (float32 [4, D, D]), the
        one-pixel action mask (bool [D, D]), the chosen value map (float32 [D, D]), max_indices, rotation and scale --
        `gather_experience`; the lock-step driver leaves them in self.last_experience, episode_program in its record's
        'experience' list (one entry per action, None for a step without a valid action).
        dump_visualizations / visualize / frame_size: the reference's `--dump_visualizations` (FlingPrimitives has the
        details: slower default moves, three holds, frames taken on the device during movep).  visualize: the episodes
        (reset / attach) or task indices (evaluate.run_tasks) to film, None = all.  Frames are collected at the end of every
        action: written to <visualization_root>/<episode name>/ (taskio.FrameDump) when a root is given, else kept in
        self.frames[e] (a list of uint8 [F, H, W, 3] arrays, one per action: short test runs only).
        action_report / report_root / report_panel / report: the picture of every chosen action (flingbot_amd/report.py; the
        reference's visualize_action figure, simEnv.py:653-654): at selection time the chosen stack entry, the chosen value
        map, the value range over the chosen primitive's maps (fs_value_range), the observation's RGB planes and the action's
        overlay stay on the device; after the action the next observation -- for an action that ends the episode one extra,
        read-only observe_batch, the reference's unconditional get_obs() at simEnv.py:503 -- completes them, and ONE
        report.compose call (fs_action_panels) draws the strips of all episodes that just finished an action.  report: the
        episodes (reset / attach) or task indices (evaluate.run_tasks) to report, None = all.  With a report_root the strips go
        to <root>/<episode name>/step{k:02d}.png and one line per action to <root>/actions.jsonl (report.write_report makes
        index.html of them); without one they are kept in self.panels[e] (lock-step) or the record's 'panels' list
        (episode_program): short test runs only.  Off (the default): no launch, download or request is added.
        randomize_appearance / appearance_seed: domain randomisation of what the renderer draws (flingbot_amd/appearance.py;
        the reference's Blender configuration, render_rgbd.py:26-37).  "observation": before EVERY observation -- observe()
        and the ("observe",) request of episode_program -- the episode's appearance is set to
        appearance.draw((seed, task index, timestep)), as the reference draws at every render_cloth(); "episode": the
        timestep of the key is 0, one appearance per episode.  The after-image of a terminating action, the ("look",)
        request and the film frames use whatever was set last.  The seed is appearance_seed, else the run's (run_episodes' /
        run_tasks' `seed`), else 0.  The records gain 'appearance': one float32 row (appearance.as_row) per action, what its
        observation was rendered with.  None (the default): no call is added anywhere and the records are what they were."""
        self.sim = sim
        if randomize_appearance is not None:
            from . import appearance
            if randomize_appearance not in appearance.MODES:
                raise ValueError(f"randomize_appearance: {randomize_appearance!r} is none of {appearance.MODES}")
        self.randomize_appearance = randomize_appearance
        self.appearance_seed = None if appearance_seed is None else int(appearance_seed)
        self.run_seed = None              # the run's seed (run_episodes / run_tasks set it), used when appearance_seed is None
        self.last_appearance = {}         # {episode: the row its last observation was rendered with}
        self.appearance_task_offset = 0   # lock-step: the index of the tasks' first in its set (lookahead.run_waves)
        self.record_experience = bool(record_experience)
        self.action_report = bool(action_report)
        self.report_panel = int(report_panel)
        self.report = None if report is None else [int(v) for v in report]
        self.report_root = report_root
        self.panels, self._report_obs, self._report_names, self._report_max = {}, {}, {}, {}
        self._report_log = None
        if self.action_report:
            from .report import ActionLog
            self._report_log = ActionLog(report_root)
        self.last_experience, self.last_coverage, self._stacks = {}, {}, {}
        self.dump_visualizations = bool(dump_visualizations)
        self.visualize = None if visualize is None else [int(v) for v in visualize]
        self.frame_size = (int(frame_size[0]), int(frame_size[1]))
        self.visualization_root = visualization_root
        self.frames, self.frame_dumps = {}, {}
        self.visualization_dirs = {}   # lock-step driver: {episode: directory of its film}, filled when the episode ends
        # scheduled: every episode runs its action + postaction as its own program on shared launch sequences
        # (flingbot_amd/schedule.py); False: the lock-step phases of FlingPrimitives.  Identical results.
        self.scheduled = bool(scheduled)
        self.actions = list(action_primitives)
        self.obs_dim, self.image_dim = int(obs_dim), int(image_dim)
        self.render_dim = int(render_dim)  # pyflex renders 720 x 720 (get_image reshapes to it, flex_utils.py:421)
        self.use_adaptive_scaling = bool(use_adaptive_scaling)
        if "fling" in self.actions:  # nets.py:213-218
            self.rotations = [(2 * i / (num_rotations - 1) - 1) * 90 for i in range(num_rotations)]
        else:
            self.rotations = [(2 * i / num_rotations - 1) * 180 for i in range(num_rotations)]
        self.scale_factors = np.array(scale_factors, np.float64)
        self.transformations = [(r, s) for r in self.rotations for s in self.scale_factors]  # product(rotations, scales)
        self.conservative_grasp_radius = int(conservative_grasp_radius)
        self.episode_length = int(episode_length)
        self.device = torch.device(device)
        self.selector = ActionSelector(self.actions, self.rotations, obs_dim, pix_grasp_dist, pix_drag_dist, pix_place_dist,
                                       reach_distance_limit, stretchdrag_dist=stretchdrag_dist, grasp_height=grasp_height)
        self._prim_kwargs = dict(grasp_height=grasp_height, fling_speed=fling_speed, stretchdrag_dist=stretchdrag_dist)
        if self.dump_visualizations:
            self._prim_kwargs.update(dump_visualizations=True, frame_size=self.frame_size)
        self.envs, self.prim = [], None
        self.timestep, self.terminate = {}, {}
        self.pretransform_depth = {}
        self.pretransform_depth_dev = {}   # the same planes where fs_observe left them (views of the observation tensors)
        self.adaptive_scale_factors = {}

    # ---- SimEnv.reset for a batch of tasks (entry e of `tasks` becomes episode e)
    def reset(self, tasks):
        self.attach(load_tasks(self.sim, tasks))
        if getattr(self, "action_report", False):
            self._report_max = {e: float(tasks[k]["flatten_area"]) for k, e in enumerate(self.envs)}
        for e in self.envs:
            cp = self.sim.get_camera_params(e)
            self.sim.set_camera_params(e, [*cp[2:8], self.render_dim, self.render_dim])
        return self.observe()

    def attach(self, envs):
        """What SimEnv.reset does once the scene and state of the episodes are in place (simEnv.py:674-681): initial
        coverage, the two pickers at [0.2, 0.5, 0.0], reset_end_effectors, one simulation step, grasp off, counters."""
        self.envs = [int(e) for e in envs]
        self.init_coverage = np.array(self.sim.coverage())
        film = {}
        if getattr(self, "dump_visualizations", False):
            film = dict(visualize=self.envs if self.visualize is None else [e for e in self.envs if e in self.visualize])
        self.prim = FlingPrimitives(self.sim, self.envs, **self._prim_kwargs, **film)
        self.prim.setup_pickers()  # (capture starts at its end: what the reset itself moved is not part of the film)
        self.timestep = {e: 0 for e in self.envs}
        self.terminate = {e: False for e in self.envs}
        if getattr(self, "action_report", False):
            self._report_names = {e: f"episode{e:05d}" for e in self.envs if self.report is None or e in self.report}
            self.panels = {e: [] for e in self._report_names}
            self._report_max = {}
        for e in self.prim.visualize:
            self.frame_dumps.pop(e, None)  # (an episode of an earlier reset that never terminated: its film is abandoned)
            self._open_film(e, f"episode{e:05d}")

    # ---- the film: frames are handed over at the end of every action (host memory does not grow with the episode)
    def _open_film(self, e, name):
        import os

        from .taskio import FrameDump
        self.frames[e] = []
        if self.visualization_root is not None:
            self.frame_dumps[e] = FrameDump(os.path.join(str(self.visualization_root), str(name)))

    def _collect_frames(self, envs):
        for e in envs:
            if e not in self.frames:
                continue
            got = self.prim.take_frames(e)
            if got is None or not len(got):
                continue
            if e in self.frame_dumps:
                self.frame_dumps[e].append(got)
            else:
                self.frames[e].append(got)

    def close_film(self, e):
        """SimEnv.on_episode_end's video part (simEnv.py:782-803) for episode e: stop filming, write the file; returns the
        directory (`visualization_dir`) or None."""
        if e not in self.frames:
            return None
        self._collect_frames([e])
        self.prim.stop_capture([e])
        dump = self.frame_dumps.pop(e, None)
        if dump is None:
            return None
        del self.frames[e]
        return dump.finish()

    def _adaptive_factors(self, bbox):
        """simEnv.py:722-731: scale factors shrunk to the cloth's bounding box (with some breathing room)."""
        factors = self.scale_factors.copy()
        if self.use_adaptive_scaling and bbox[4] > 0:
            dim = self.image_dim  # dimx == dimy
            cropx = max(dim - 2 * int(bbox[0]), dim - 2 * (dim - int(bbox[1])))
            cropy = max(dim - 2 * int(bbox[2]), dim - 2 * (dim - int(bbox[3])))
            crop = int(max(cropx, cropy) * 1.5)  # some breathing room
            if crop < dim:
                factors *= crop / dim
        return factors

    def get_obs(self, e):
        """SimEnv.get_obs (simEnv.py:710-737): render, resize to image_dim, cloth mask -> adaptive scale factors,
        preprocess_obs -- all in fs_observe; returns float32 [4, S, S] on the device."""
        obs, bbox = self.sim.observe(e, self.image_dim)
        self.pretransform_depth[e] = obs[3].cpu().numpy()
        self.pretransform_depth_dev[e] = obs[3]
        if e in getattr(self, "_report_names", ()):
            self._report_obs[e] = obs[:3]
        self.adaptive_scale_factors[e] = self._adaptive_factors(bbox)
        return obs

    def get_obs_batch(self, envs):
        """get_obs for several episodes: one fs_observe_batch call (the labelling rounds of all episodes share their host
        round trips) and ONE download of the depth planes the host side of the action selection reads."""
        envs = [int(e) for e in envs]
        obs, bbox = self.sim.observe_batch(envs, self.image_dim)
        depth = obs[:, 3].cpu().numpy() if envs else None
        for k, e in enumerate(envs):
            self.pretransform_depth[e] = depth[k]
            self.pretransform_depth_dev[e] = obs[k, 3].clone()  # (a view would keep the whole batch tensor alive per slot)
            self.adaptive_scale_factors[e] = self._adaptive_factors(bbox[k])
            if e in getattr(self, "_report_names", ()):
                self._report_obs[e] = obs[k, :3].clone()
        return obs

    def particle_state(self, envs=None, **kwargs):
        """FlingSim.state_tensors for the episodes this environment drives (all of them, or the listed ones): the particle
        state as padded CUDA tensors, one launch."""
        envs = self.envs if envs is None else [int(e) for e in envs]
        stray = [e for e in envs if e not in self.envs]
        if stray:
            raise ValueError(f"particle_state: episodes {stray} are not driven by this environment")
        return self.sim.state_tensors(envs, **kwargs)

    def get_transformations(self, e):
        return [(r, s) for r in self.rotations for s in self.adaptive_scale_factors[e]]  # product(rotations, scales)

    def randomize(self, keys):
        """Before an observation: keys = {episode: task index}; ONE set_appearance call gives every listed episode the
        appearance of (seed, task index, timestep) -- a pure function of the key, whichever slot or batch it is served in."""
        from . import appearance
        seed = self.appearance_seed if self.appearance_seed is not None else (self.run_seed if self.run_seed is not None else 0)
        es = sorted(keys)
        drawn = [appearance.draw(appearance.key_of(self.randomize_appearance, seed, keys[e], self.timestep[e])) for e in es]
        self.sim.set_appearance(es, drawn)
        for e, a in zip(es, drawn):
            self.last_appearance[e] = appearance.as_row(a)

    def observe(self):
        """{episode: transformed observation [T, 4, D, D] (CUDA)} for the episodes that are still running."""
        run = [e for e in self.envs if not self.terminate[e]]
        if getattr(self, "randomize_appearance", None) is not None and run:
            first = getattr(self, "appearance_task_offset", 0)      # (reset: entry k of the tasks is episode envs[k])
            self.randomize({e: first + self.envs.index(e) for e in run})
        obs = self.get_obs_batch(run)
        stacks = {e: nets.prepare_image(obs[k], self.get_transformations(e), self.obs_dim) for k, e in enumerate(run)}
        if getattr(self, "record_experience", False) or getattr(self, "action_report", False):
            self._stacks = dict(stacks)   # (what the next step's actions were chosen from)
        return stacks

    # ---- the action report (flingbot_amd/report.py)
    def hold_action(self, e, stack, maps, action, params):
        """At selection time: what the strip of episode e's chosen action needs, kept on the device (clones: the stack and the
        maps are replaced by the next observation), plus the overlay lists and the line for actions.jsonl."""
        from . import report
        x = int(params["max_indices"][0])
        chosen = maps[action] if isinstance(maps, dict) else maps[self.actions.index(action)]
        chosen = chosen.to(self.device).contiguous().float()          # all maps of the chosen primitive, [T, D, D]
        pix = report.transformed_pixels(action, params["max_indices"], self.selector)
        return dict(stack=stack[x].to(self.device).float().clone(), value_map=chosen[x].clone(),
                    range=report.value_range([chosen])[0], before=self._report_obs[e], after=None,
                    small=report.action_overlays(action, pix, thickness=1),
                    large=report.action_overlays(action, params["pretransform_pixels"], thickness=3),
                    meta=dict(primitive=action, rotation=float(params["rotation"]), scale=float(params["scale"]),
                              max_indices=[int(v) for v in params["max_indices"]]))

    def look_batch(self, envs):
        """The observation's RGB planes of the listed episodes, [n, 3, S, S] on the device, and nothing else: the bookkeeping
        of get_obs_batch (depth, scale factors) is left as it is.  The after-image of an action that ended its episode."""
        obs, _ = self.sim.observe_batch([int(e) for e in envs], self.image_dim)
        return obs[:, :3]

    def compose_reports(self, held):
        """ONE report.compose call for the held actions (each with its 'after' in place) -> uint8 [n, panel, 5 panel, 3]."""
        from . import report
        return report.compose(held, panel=self.report_panel)

    def file_report(self, e, held, strip, step, pre, post, max_coverage=None, film_dir=None):
        """One finished strip: to the report directory when there is one; returns the png's path, or None."""
        if self._report_log is None or self._report_log.root is None:
            return None
        name = self._report_names[e]
        meta = dict(key=f"{name}_step{int(step):02d}", task=name, step=int(step), **held["meta"], preaction_coverage=float(pre),
                    postaction_coverage=float(post), max_coverage=None if max_coverage is None else float(max_coverage),
                    film_dir=None if film_dir is None else str(film_dir))
        return self._report_log.write(name, meta, strip)

    def gather_experience(self, items):
        """items: [(stack [T, 4, D, D], value map [T, D, D], action parameters of ActionSelector.select), ...] on the device.
        ONE gather (entry x of every stack and of every value map, concatenated) and ONE download for all of them; returns
        one dictionary per item: observations, actions, value_map, max_indices, rotation, scale."""
        if not items:
            return []
        xs = [int(p["max_indices"][0]) for _, _, p in items]
        planes = torch.cat([t for (stack, vmap, _), x in zip(items, xs)
                            for t in (stack[x].to(self.device), vmap[x].to(self.device).unsqueeze(0))]).cpu().numpy()
        planes = planes.reshape(len(items), 5, self.obs_dim, self.obs_dim)
        out = []
        for k, (_, _, p) in enumerate(items):
            x, y, z = (int(v) for v in p["max_indices"])
            mask = np.zeros((self.obs_dim, self.obs_dim), bool)
            mask[y, z] = True     # action_mask[y, z] = 1 (simEnv.py:590-591)
            out.append(dict(observations=np.ascontiguousarray(planes[k, :4], np.float32), actions=mask,
                            value_map=np.ascontiguousarray(planes[k, 4], np.float32),
                            max_indices=np.array([x, y, z], np.int64), rotation=float(p["rotation"]), scale=float(p["scale"])))
        return out

    def _on_cloth(self, depth, pix):
        yy, xx = np.ogrid[:depth.shape[0], :depth.shape[1]]
        r = self.conservative_grasp_radius
        if r <= 0:
            return True
        disc = (yy - pix[0]) ** 2 + (xx - pix[1]) ** 2 <= r * r
        return bool((depth != 2.0)[disc].all())

    # ---- SimEnv.step for every running episode: value_maps[e] = {primitive: CUDA tensor [T, D, D]}
    def step(self, value_maps):
        run = [e for e in self.envs if not self.terminate[e] and e in value_maps]
        if not run:
            return {}, {}, dict(self.terminate), {}
        # the reference takes the snapshot and the coverage BEFORE selecting (simEnv.py:477-485); selection reads neither
        chosen = {}
        for e in run:
            action, params = self.selector.select(value_maps[e], self.adaptive_scale_factors[e], self.pretransform_depth[e],
                                                  depth_device=self.pretransform_depth_dev.get(e))
            if action is not None:
                d, pix = self.pretransform_depth[e], params["pretransform_pixels"]
                params["p1_grasp_cloth"] = self._on_cloth(d, (pix[0][1], pix[0][0]))
                params["p2_grasp_cloth"] = self._on_cloth(d, (pix[1][1], pix[1][0]))
                chosen[e] = (action, params)
        if getattr(self, "record_experience", False):   # before the action: the stacks are replaced by the next observe()
            es = [e for e in run if e in chosen]
            vmap = lambda e: value_maps[e][chosen[e][0] if isinstance(value_maps[e], dict) else self.actions.index(chosen[e][0])]  # noqa: E731
            got = self.gather_experience([(self._stacks[e], vmap(e), chosen[e][1]) for e in es])
            self.last_experience = {e: None for e in run}
            self.last_experience.update(dict(zip(es, got)))
        held = {}
        if getattr(self, "action_report", False):   # before the action, for the same reason
            vmaps = lambda e: value_maps[e] if isinstance(value_maps[e], dict) else dict(zip(self.actions, value_maps[e]))  # noqa: E731
            held = {e: self.hold_action(e, self._stacks[e], vmaps(e), *chosen[e]) for e in run
                    if e in chosen and e in self._report_names}
            steps = {e: self.timestep[e] for e in held}
        rewards, acted = self.step_actions(run, chosen)
        stacks = self.observe()
        if getattr(self, "action_report", False) and self.report_root is None:
            for e in run:
                if e in self._report_names and e not in held:
                    self.panels[e].append(None)                 # (one entry per action, like last_experience)
        if held:
            ended = [e for e in held if self.terminate[e]]
            looks = self.look_batch(ended) if ended else None
            for e, item in held.items():
                item["after"] = looks[ended.index(e)].contiguous() if e in ended else self._report_obs[e]
            order = sorted(held)
            strips = self.compose_reports([held[e] for e in order])
            for k, e in enumerate(order):
                film = self.visualization_dirs.get(e) if e in ended else getattr(self.frame_dumps.get(e), "directory", None)
                pre, post = self.last_coverage[e]
                if self.file_report(e, held[e], strips[k], steps[e], pre, post, self._report_max.get(e), film) is None:
                    self.panels[e].append(strips[k])
        for e in run:
            if self.terminate[e]:
                self._report_obs.pop(e, None)        # (3 S^2 floats per episode: not kept past its end)
        return stacks, rewards, dict(self.terminate), acted

    def step_actions(self, run, chosen):
        """SimEnv.step (simEnv.py:477-515) for the episodes `run` once the actions are known: chosen[e] = (primitive,
        {'p1', 'p2', 'p1_grasp_cloth', 'p2_grasp_cloth'}); an episode missing from `chosen` found no valid action.
        preaction -> coverage -> one batched primitive call per action type -> postaction (reset_end_effectors,
        wait_until_stable, "the cloth did not move" -> terminate) -> coverage -> timestep / episode_length.
        Returns ({episode: reward}, {episode: primitive or None})."""
        run = [int(e) for e in run]
        self.prim.preaction(run)
        prev = np.array(self.sim.coverage())
        if getattr(self, "scheduled", False):
            acts = {e: (chosen[e][0], chosen[e][1]["p1"], chosen[e][1]["p2"], chosen[e][1]["p1_grasp_cloth"],
                        chosen[e][1]["p2_grasp_cloth"]) for e in run if e in chosen}
            self.prim.act_scheduled(acts, run)
            return self._finish_step(run, chosen, prev)
        for action in self.actions:  # one batched primitive call per action type
            es = [e for e in run if e in chosen and chosen[e][0] == action]
            if not es:
                continue
            film = dict(visualize=[e for e in es if self.prim.flagged(e)]) if getattr(self, "dump_visualizations", False) else {}
            sub = FlingPrimitives(self.sim, es, **self._prim_kwargs, **film)  # (capture state lives in the simulator)
            sub.grasp_states = {e: self.prim.grasp_states[e] for e in es}
            p1 = [chosen[e][1]["p1"] for e in es]
            p2 = [chosen[e][1]["p2"] for e in es]
            g1 = [chosen[e][1]["p1_grasp_cloth"] for e in es]
            g2 = [chosen[e][1]["p2_grasp_cloth"] for e in es]
            fn = {"fling": sub.pick_and_fling, "drag": sub.pick_and_drag, "place": sub.pick_and_place,
                  "stretchdrag": sub.pick_stretch_drag}[action]
            fn(p1, p2, g1, g2)
            self.prim.sim_steps += sub.sim_steps
            for e in es:
                self.prim.terminate[e] = self.prim.terminate[e] or sub.terminate[e]
                # SimEnv keeps grasp_states across the handler: an early return (cloth not grasped, simEnv.py:306-308) leaves
                # [p1_grasp, p2_grasp] set for postaction's reset_end_effectors / wait_until_stable
                self.prim.grasp_states[e] = list(sub.grasp_states[e])
        self.prim.postaction(run)
        return self._finish_step(run, chosen, prev)

    # ---- SimEnv.reset + SimEnv.step until the episode ends, for ONE slot, as a program (flingbot_amd/schedule.py)
    def open_slots(self, slots):
        """Bookkeeping for slots that episode_program will fill (instead of reset / attach)."""
        self.envs = [int(e) for e in slots]
        film = dict(visualize=[]) if getattr(self, "dump_visualizations", False) else {}  # (episode_program films per task)
        self.prim = FlingPrimitives(self.sim, self.envs, **self._prim_kwargs, **film)
        self.timestep = {e: 0 for e in self.envs}
        self.terminate = {e: True for e in self.envs}
        self.init_coverage = np.zeros(self.sim.n_envs)
        self.unpaid_steps = 0  # simulation steps the lock-step path does not count either (the step inside set_scene)
        self._report_names, self._report_obs = {}, {}   # (episode_program reports per task)

    def episode_program(self, e, task, max_actions=None, prebuilt=None, film=None, explore_key=None, report=None,
                        task_index=None):
        """One episode in slot e -- SimEnv.reset (simEnv.py:663-697: set_scene(config, state), initial coverage, pickers,
        reset_end_effectors, one step, grasp off) and then SimEnv.step (simEnv.py:477-515) until it terminates -- written as
        the reference's straight-line code with a request wherever it needs the simulator, the policy or a reduction (see
        schedule.run_programs; evaluate.run_tasks provides the services "observe", "act", "coverage", "snapshot",
        "max_disp").  max_actions: the episode also ends after that many actions (None: episode_length alone).
        prebuilt: the task's sim.PrebuiltScene when its host half was built ahead (tasks.ScenePrebuilder).
        film: a name -- the episode is filmed (dump_visualizations must be set), its frames go to
        <visualization_root>/<film>/ at the end of every action and the record gains 'visualization_dir'; None: not filmed.
        The flag's physics (default speed 1e-2, the three holds) applies to the filmed episodes only: the others run exactly
        as without the flag.
        explore_key: (seed, task index) -- the policy's exploration draws for action k come from the key (seed, task index, k)
        (nets.MaximumValuePolicy._explore); None: the global random streams.
        With record_experience the record gains 'experience' (service "record": gather_experience for all ready slots).
        report: a name -- the episode's chosen actions are reported (action_report must be set) under <report_root>/<report>/;
        after every action the program asks for ("panels", held action) -- report.compose for all ready slots -- and, for the
        action that ends the episode, first for ("look",): the after-image.  Without a report_root the record gains 'panels'.
        task_index: the task's index in its set -- with randomize_appearance the key of the episode's appearances (0 when
        None); the record gains 'appearance'.
        Returns {'coverage': [initial, after step 1, ...] (absolute areas), 'actions': [primitive or None, ...]}."""
        from . import schedule as sch

        e = int(e)
        sim, prim = self.sim, self.prim
        ep = sch.Episode(prim, e)
        load_task_scene(sim, e, task, prebuilt=prebuilt)
        yield ("step", 1)
        self.unpaid_steps += 1
        load_task_state(sim, e, task)
        cov = yield ("coverage",)
        self.init_coverage[e] = cov
        prim.grasp_states[e] = [False, False]
        prim.terminate[e] = False
        prim.place_pickers(e)
        yield from sch.reset_end_effectors(ep)
        yield ("step", 1)
        prim.set_grasp([e], False)
        cp = sim.get_camera_params(e)
        sim.set_camera_params(e, [*cp[2:8], self.render_dim, self.render_dim])
        self.timestep[e], self.terminate[e] = 0, False
        filmed = film is not None and self.dump_visualizations
        if filmed:  # env_video_frames = {} at the end of reset (simEnv.py:681)
            prim.visualize = sorted(set(prim.visualize) | {e})
            prim.start_capture([e])
            self._open_film(e, film)
        reported = report is not None and getattr(self, "action_report", False)
        self._report_names.pop(e, None)   # (the slot's previous episode)
        if reported:
            self._report_names[e] = str(report)
        cov = yield ("coverage",)  # what run_sim's statistics call the initial coverage: the state the first observation shows
        rec = dict(coverage=[float(cov)], actions=[])
        randomized = getattr(self, "randomize_appearance", None) is not None
        if randomized:
            self.randomize({e: 0 if task_index is None else int(task_index)})
        obs = yield ("observe",)
        while True:
            if randomized:
                rec.setdefault("appearance", []).append(self.last_appearance[e])
            if explore_key is None:
                maps = yield ("act", obs)
            else:
                maps = yield ("act", obs, tuple(explore_key) + (self.timestep[e],))
            action, params = self.selector.select(maps, self.adaptive_scale_factors[e], self.pretransform_depth[e],
                                                  depth_device=self.pretransform_depth_dev.get(e))
            body = None
            if action is not None:
                d, pix = self.pretransform_depth[e], params["pretransform_pixels"]
                g1 = self._on_cloth(d, (pix[0][1], pix[0][0]))
                g2 = self._on_cloth(d, (pix[1][1], pix[1][0]))
                body = sch.PROGRAMS[action](ep, params["p1"], params["p2"], g1, g2)
            if getattr(self, "record_experience", False):
                rec.setdefault("experience", []).append(
                    None if action is None else (yield ("record", obs, maps[action], params)))
            held = self.hold_action(e, obs, maps, action, params) if reported and action is not None else None
            yield ("snapshot",)                      # preaction
            prev = yield ("coverage",)
            yield from sch.action_then_settle(ep, body)
            moved = yield ("max_disp",)
            if filmed:   # (the action's chunks are closed: its wait's outcome is known)
                self._collect_frames([e])
            if moved < 5e-2:  # if didn't really move cloth then end early (simEnv.py:470-475)
                prim.terminate[e] = True
            curr = yield ("coverage",)
            self.timestep[e] += 1
            limit = self.episode_length if max_actions is None else min(self.episode_length, int(max_actions))
            self.terminate[e] = prim.terminate[e] or self.timestep[e] >= limit
            rec["coverage"].append(float(curr))
            rec["actions"].append(action)
            rec.setdefault("rewards", []).append(float(curr - prev))
            rec.setdefault("preaction_coverage", []).append(float(prev))
            if reported and held is None and self.report_root is None:
                rec.setdefault("panels", []).append(None)       # (one entry per action, like 'experience')
            if self.terminate[e]:
                if filmed:
                    vis_dir = self.close_film(e)
                    prim.visualize = [v for v in prim.visualize if v != e]
                    if vis_dir is not None:
                        rec["visualization_dir"] = vis_dir
                if held is not None:
                    held["after"] = yield ("look",)
                    strip = yield ("panels", held)
                    if self.file_report(e, held, strip, self.timestep[e] - 1, prev, curr, task["flatten_area"],
                                        rec.get("visualization_dir")) is None:
                        rec.setdefault("panels", []).append(strip)
                self._report_names.pop(e, None)
                self._report_obs.pop(e, None)        # (3 S^2 floats per slot: not kept past the episode)
                return rec
            if randomized:
                self.randomize({e: 0 if task_index is None else int(task_index)})
            obs = yield ("observe",)
            if held is not None:
                held["after"] = self._report_obs[e]
                strip = yield ("panels", held)
                film_dir = getattr(self.frame_dumps.get(e), "directory", None) if filmed else None
                if self.file_report(e, held, strip, self.timestep[e] - 1, prev, curr, task["flatten_area"], film_dir) is None:
                    rec.setdefault("panels", []).append(strip)

    def _finish_step(self, run, chosen, prev):
        filming = getattr(self, "dump_visualizations", False)
        if filming:
            self._collect_frames(run)
        curr = np.array(self.sim.coverage())
        rewards = {}
        for e in run:
            self.timestep[e] += 1
            self.terminate[e] = self.prim.terminate[e] or self.timestep[e] >= self.episode_length
            if filming and self.terminate[e] and self.prim.flagged(e):  # on_episode_end (simEnv.py:782-803)
                self.visualization_dirs[e] = self.close_film(e)
                self.prim.visualize = [v for v in self.prim.visualize if v != e]
            rewards[e] = float(curr[e] - prev[e])
            self.__dict__.setdefault("last_coverage", {})[e] = (float(prev[e]), float(curr[e]))   # (run_episodes' records)
        return rewards, {e: chosen.get(e, (None, None))[0] for e in run}
