"""The training half of learning/Memory.py + learning/utils.py GraspDataset: recorded experience as a dataset.

    stats = evaluate.run_tasks(policy, BatchedFlingEnv(sim, record_experience=True), tasks, seed=0)
    taskio.save_replay("replay.npz", stats["records"], tasks)
    data = ExperienceSet(["replay.npz"]).to_device("cuda:0")
    obs, mask, label = data.sample(128, np.random.default_rng(0))      # run_sim.optimize's loop body takes these three

The reference's loader opens one HDF5 group per sample and pushes the image through torchvision's
`ColorJitter(0.2, 0.3, 0.5, 0.5)` -- for PIL inputs a chain of Pillow's ImageEnhance.Brightness / Contrast / Color and an
RGB -> HSV -> RGB round trip -- on the host, 128 times per batch.  Here the set is resident on the device and ONE launch
per batch (fs_replay_sample, csrc/fs_replay.hip) gathers the drawn samples, selects the channels and runs the jitter.
`color_jitter_host` restates the Pillow chain in numpy; it is pinned to Pillow itself by tests/golden/jitter_golden.npz
and it is what the kernel is tested against, bit for bit.  Pillow is needed by neither.

`MapSet` reads the same files as a set of IMAGES: the entries that share one observation (the executed cells of a measured reward
map) are one stored image with a list of (pixel, label) pairs, drawn by `sample_maps` for train.optimize_maps.
"""
import numpy as np

from .sim import stream_call

REWARDS_MAX = 0.20572495126190674     # learning/utils.py:5-8
REWARDS_MIN = -0.11034914070874759
JITTER_RANGES = ((0.8, 1.2), (0.7, 1.3), (0.5, 1.5), (-0.5, 0.5))   # brightness, contrast, saturation, hue
BRIGHTNESS, CONTRAST, SATURATION, HUE = range(4)    # torchvision's fn_idx numbering (transforms.py ColorJitter.forward)
OBS_DIM = 64                                         # the size the hand-written value net and the sample kernel serve
ARRAY_FIELDS = ("observations", "actions", "value_map", "max_indices", "rotation", "scale")

_f32, _f64 = np.float32, np.float64


def draw_jitter(rng, n):
    """ColorJitter.get_params for n samples from a numpy Generator: a permutation of the four operations and one factor
    each, uniform in JITTER_RANGES.  Factors are float32 (torchvision draws them from a float32 tensor; Pillow's blend
    takes a C float).  Returns {'order': int32 [n, 4], 'factors': float32 [n, 4] (indexed by operation)}."""
    n = int(n)
    order = rng.permuted(np.tile(np.arange(4, dtype=np.int32), (n, 1)), axis=1)
    lo = np.array([r[0] for r in JITTER_RANGES])
    hi = np.array([r[1] for r in JITTER_RANGES])
    factors = rng.uniform(lo, hi, size=(n, 4)).astype(_f32)
    return {"order": np.ascontiguousarray(order, np.int32), "factors": np.ascontiguousarray(factors)}


def quantize(rgb):
    """float [0, 1] -> uint8 the way ToPILImage's `pic.mul(255).byte()` does inside [0, 255]: trunc(x * 255) in float32.
    Outside of it (prepare_image's cubic spline overshoots at edges) the reference's `.byte()` is a float -> uint8
    conversion of an out-of-range value, which C leaves undefined; here the product is clamped to [0, 255] first."""
    x = np.asarray(rgb, _f32) * _f32(255.0)
    return np.trunc(np.fmin(np.fmax(x, _f32(0.0)), _f32(255.0))).astype(np.uint8)


def luma(rgb):
    """Pillow's RGB -> L (Convert.c L24): (19595 R + 38470 G + 7471 B + 0x8000) >> 16; rgb: integer [..., 3]."""
    c = rgb.astype(np.int32)
    return (19595 * c[..., 0] + 38470 * c[..., 1] + 7471 * c[..., 2] + 0x8000) >> 16


def blend(degenerate, image, factor):
    """ImageEnhance._Enhance.enhance = Image.blend(degenerate, image, factor) (Blend.c): per channel
    trunc(clip(d + a * (x - d), 0, 255)), the product and the sum each rounded to float32."""
    d, x = degenerate.astype(np.int32), image.astype(np.int32)
    t = d.astype(_f32) + _f32(factor) * (x - d).astype(_f32)
    return np.trunc(np.clip(t, _f32(0.0), _f32(255.0))).astype(np.uint8)


def rgb_to_hsv(rgb):
    """Pillow's rgb2hsv_row (Convert.c): s and the per-channel ratios in float, the hue term and fmod(h / 6 + 1, 1) in
    double, every assignment to the C `float h` rounding to float32.  uint8 [..., 3] -> uint8 [..., 3]."""
    c = rgb.astype(np.int32)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    gray = maxc == minc
    cr = np.where(gray, 1, maxc - minc).astype(_f32)
    s = cr / np.maximum(maxc, 1).astype(_f32)
    rc, gc, bc = ((maxc - r).astype(_f32) / cr, (maxc - g).astype(_f32) / cr, (maxc - b).astype(_f32) / cr)
    h = np.where(r == maxc, bc - gc,
                 np.where(g == maxc, (2.0 + rc.astype(_f64) - bc.astype(_f64)).astype(_f32),
                          (4.0 + gc.astype(_f64) - rc.astype(_f64)).astype(_f32)))
    h = np.fmod(h.astype(_f64) / 6.0 + 1.0, 1.0).astype(_f32)
    uh = np.clip((h.astype(_f64) * 255.0).astype(np.int32), 0, 255)
    us = np.clip((s.astype(_f64) * 255.0).astype(np.int32), 0, 255)
    out = np.stack([np.where(gray, 0, uh), np.where(gray, 0, us), maxc], axis=-1)
    return out.astype(np.uint8)


def _round_half_away(x):
    """C round() for x >= 0 without the x + 0.5 rounding trap."""
    fl = np.floor(x)
    return (fl + (x - fl >= 0.5)).astype(np.int32)


def hsv_to_rgb(hsv):
    """Pillow's hsv2rgb (Convert.c): the sector and the remainder from h * 6 / 255 in double, `f` and `fs` stored as float,
    p / q / t = round(v * (1 - ...)) in double, rounded half away from zero.  uint8 [..., 3] -> uint8 [..., 3]."""
    c = hsv.astype(np.int32)
    h, s, v = c[..., 0], c[..., 1], c[..., 2]
    x6 = h.astype(_f64) * 6.0 / 255.0
    i = np.floor(x6)
    f = (x6 - i).astype(_f32).astype(_f64)
    fs = (s.astype(_f64) / 255.0).astype(_f32).astype(_f64)
    vd = v.astype(_f64)
    p = np.clip(_round_half_away(vd * (1.0 - fs)), 0, 255)
    q = np.clip(_round_half_away(vd * (1.0 - fs * f)), 0, 255)
    t = np.clip(_round_half_away(vd * (1.0 - fs * (1.0 - f))), 0, 255)
    sector = i.astype(np.int32) % 6
    r = np.choose(sector, [v, q, p, p, t, v])
    g = np.choose(sector, [t, v, v, q, p, p])
    b = np.choose(sector, [p, p, t, v, v, q])
    gray = s == 0
    out = np.stack([np.where(gray, v, r), np.where(gray, v, g), np.where(gray, v, b)], axis=-1)
    return out.astype(np.uint8)


def hue_shift(factor):
    """torchvision's `np_h += np.uint8(hue_factor * 255)`: the product in double, truncated toward zero, modulo 256."""
    return int(float(_f32(factor)) * 255.0) % 256


def jitter_uint8(img, order, factors):
    """The four operations on ONE uint8 [H, W, 3] image in the drawn order (torchvision's functional_pil adjust_* on a PIL
    image): brightness blends with black, saturation with the gray image L, contrast with the flat image
    int(mean(L) + 0.5) of the image as it stands at that stage, hue shifts the H plane of Pillow's HSV with wrap-around."""
    img = np.asarray(img, np.uint8)
    for op in order:
        op = int(op)
        if op == BRIGHTNESS:
            img = blend(np.zeros_like(img), img, factors[op])
        elif op == CONTRAST:
            mean = int(float(luma(img).sum(dtype=np.int64)) / float(img.shape[0] * img.shape[1]) + 0.5)
            img = blend(np.full_like(img, mean), img, factors[op])
        elif op == SATURATION:
            img = blend(np.repeat(luma(img)[..., None], 3, axis=-1), img, factors[op])
        elif op == HUE:
            hsv = rgb_to_hsv(img)
            hsv[..., 0] = (hsv[..., 0].astype(np.int32) + hue_shift(factors[op])) % 256
            img = hsv_to_rgb(hsv)
        else:
            raise ValueError(f"jitter operation {op}")
    return img


def color_jitter_host(rgb, params):
    """GraspDataset's `rgb_transform` (learning/utils.py:28-33: ToPILImage -> ColorJitter(0.2, 0.3, 0.5, 0.5) -> ToTensor)
    in numpy, for a batch: rgb float32 [B, 3, H, W] in [0, 1], params from draw_jitter.  Quantised with `quantize`
    (trunc(x * 255); the product is clamped to [0, 255] first, because the spline in prepare_image can overshoot and the
    reference's `.byte()` is undefined there), the four operations in each sample's own order, divided by 255 in float32
    at the end (ToTensor).  The CPU path, and the reference the kernel is tested against."""
    rgb = np.asarray(rgb, _f32)
    assert rgb.ndim == 4 and rgb.shape[1] == 3, rgb.shape
    order, factors = np.asarray(params["order"]), np.asarray(params["factors"], _f32)
    assert order.shape == (rgb.shape[0], 4) and factors.shape == (rgb.shape[0], 4)
    out = np.empty_like(rgb)
    for k in range(rgb.shape[0]):
        img = jitter_uint8(quantize(rgb[k]).transpose(1, 2, 0), order[k], factors[k])
        out[k] = img.transpose(2, 0, 1).astype(_f32) / _f32(255.0)
    return out


def read_entries(owner, paths):
    """The reading half of ExperienceSet and MapSet: the entries of `paths` that pass `owner`'s filters (its action_primitive,
    lane_ranks and the validity rule), one at a time, in file order and sorted key order within a file, as dicts {'file' (the
    path's number in this call), 'key', 'observation' float32 [4, D, D], 'mask' bool [D, D], 'label' (a Python float: float64
    arithmetic with owner.use_normalized_coverage's formula), 'lane' ((lane_task, lane_step) or None), 'primitive'}.
    owner.n_without_arrays / n_filtered / n_invalid grow by what is dropped.  Nothing but the entry being read is held."""
    from .taskio import REPLAY_FORMAT
    if isinstance(paths, (str, bytes)) or hasattr(paths, "__fspath__"):
        paths = [paths]
    action_primitive = owner.action_primitive
    for number, path in enumerate(paths):
        z = np.load(path, allow_pickle=False)
        if str(z["format"]) != REPLAY_FORMAT:
            raise ValueError(f"{path}: not a '{REPLAY_FORMAT}' file")
        names = set(z.files)
        for key in sorted(str(k) for k in z["keys"]):
            if f"{key}/observations" not in names or f"{key}/actions" not in names:
                owner.n_without_arrays += 1
                continue
            primitive = str(z[f"{key}/action_primitive"])
            if action_primitive is not None and primitive != action_primitive:
                owner.n_filtered += 1
                continue
            if owner.lane_ranks is not None:   # (an entry of an ordinary file is the policy's own action: rank 0)
                rank = int(z[f"{key}/lane_rank"]) if f"{key}/lane_rank" in names else 0
                if rank not in owner.lane_ranks:
                    owner.n_filtered += 1
                    continue
            o, m = z[f"{key}/observations"], z[f"{key}/actions"].astype(bool)
            if o.ndim != 3 or o.shape[0] != 4 or m.shape != o.shape[1:] or int(m.sum()) != 1:
                owner.n_invalid += 1
                continue
            delta = float(z[f"{key}/postaction_coverage"]) - float(z[f"{key}/preaction_coverage"])
            if owner.use_normalized_coverage:
                delta /= float(z[f"{key}/max_coverage"])
            else:
                delta = (delta - REWARDS_MIN) / (REWARDS_MAX - REWARDS_MIN)
            lane = None
            if f"{key}/lane_task" in names and f"{key}/lane_step" in names:
                lane = (int(z[f"{key}/lane_task"]), int(z[f"{key}/lane_step"]))
            yield dict(file=number, key=key, observation=np.asarray(o, _f32), mask=m, label=delta, lane=lane, primitive=primitive)


class ExperienceSet:
    """GraspDataset (learning/utils.py:12-100) over one or more files written by taskio.save_replay from a run with
    `record_experience`.

    Entries without arrays (evaluation files, steps without a valid action) are skipped; action_primitive keeps the
    entries of that primitive only (the reference's `filter_fn`); check_validity's rule -- exactly one true mask pixel,
    a [4, D, D] observation -- is applied at load and the dropped entries are counted in `n_invalid`.
    Label: (postaction - preaction coverage) / max_coverage, or with use_normalized_coverage=False the min-max form
    (delta - REWARDS_MIN) / (REWARDS_MAX - REWARDS_MIN) (utils.py:79-86); float64 arithmetic, stored as float32.
    Channels (utils.py:94-98): rgb_only -> [:3], depth_only -> [3:4], else all four.  The colour jitter applies ONLY in
    rgb_only mode -- the reference's own behaviour, kept.
    lane_ranks: a collection of look-ahead ranks -- only entries whose '<key>/lane_rank' (lookahead.save_replay) is in it are
    kept, entries of ordinary files counting as rank 0; None keeps all.  The dropped ones are counted in `n_filtered`.
    groups int64 [N]: entries that may be compared with each other share a value -- the lanes of one observation, i.e. the
    entries of ONE file with equal '<key>/lane_task' and '<key>/lane_step' (the same pair in another file is another group:
    rounds wrap around the task list); an entry without those fields is a group of its own.  The filters above apply first: a
    group is what survives them, possibly one entry.  `draw_groups` / `sample_groups` draw whole groups.
    Host arrays: observations float32 [N, 4, D, D], masks bool [N, D, D], labels float32 [N], groups int64 [N], keys."""

    def __init__(self, paths, action_primitive=None, rgb_only=True, depth_only=False, obs_color_jitter=True,
                 use_normalized_coverage=True, lane_ranks=None):
        assert not depth_only or not rgb_only
        self.lane_ranks = None if lane_ranks is None else frozenset(int(r) for r in lane_ranks)
        self.rgb_only, self.depth_only = bool(rgb_only), bool(depth_only)
        self.obs_color_jitter = bool(obs_color_jitter)
        self.use_normalized_coverage = bool(use_normalized_coverage)
        self.action_primitive = action_primitive
        self.n_invalid = self.n_without_arrays = self.n_filtered = 0
        self._next_group = 0       # group values are handed out in order of first appearance
        self._members = None       # draw_groups' table, built on demand
        obs, masks, labels, keys, groups = self._read(paths)
        self.keys = keys
        self.groups = np.array(groups, np.int64)
        dim = obs[0].shape[-1] if obs else OBS_DIM
        self.observations = np.stack(obs) if obs else np.zeros((0, 4, dim, dim), _f32)
        self.masks = np.stack(masks) if masks else np.zeros((0, dim, dim), bool)
        self.labels = np.array(labels, _f64).astype(_f32)
        self._dev = None

    def _read(self, paths):
        """The entries of `paths` that pass the set's filters, as lists (observations, masks, labels, keys, groups); the n_*
        counters grow by what was dropped and _next_group by the groups that appeared."""
        obs, masks, labels, keys, groups = [], [], [], [], []
        lanes = {}   # (file, lane_task, lane_step) -> group
        for e in read_entries(self, paths):
            obs.append(e["observation"])
            masks.append(e["mask"])
            labels.append(e["label"])
            keys.append(e["key"])
            where = None if e["lane"] is None else (e["file"],) + e["lane"]
            if where is None or where not in lanes:
                group = self._next_group
                self._next_group += 1
                if where is not None:
                    lanes[where] = group
            else:
                group = lanes[where]
            groups.append(group)
        return obs, masks, labels, keys, groups

    def extend(self, paths):
        """Add the entries of further files, through the constructor's filters; the result equals a set built from all
        files at once.  A set that is on a device uploads the new rows only.  Returns the number of entries added."""
        obs, masks, labels, keys, groups = self._read(paths)
        if not keys:
            return 0
        new_obs, new_masks = np.stack(obs), np.stack(masks)
        new_labels = np.array(labels, _f64).astype(_f32)
        if len(self.keys) and new_obs.shape[1:] != self.observations.shape[1:]:
            raise ValueError(f"ExperienceSet.extend: observations of {new_obs.shape[1:]} do not fit the set's {self.observations.shape[1:]}")
        if self._dev is not None and new_obs.shape[-2:] != (OBS_DIM, OBS_DIM):
            raise ValueError(f"fs_replay_sample serves {OBS_DIM} x {OBS_DIM} observations, got {new_obs.shape[-2:]}")
        if len(self.keys):
            self.observations = np.concatenate([self.observations, new_obs])
            self.masks = np.concatenate([self.masks, new_masks])
            self.labels = np.concatenate([self.labels, new_labels])
        else:
            self.observations, self.masks, self.labels = new_obs, new_masks, new_labels
        self.keys = list(self.keys) + keys
        self.groups = np.concatenate([self.groups, np.array(groups, np.int64)])
        self._members = None
        if self._dev is not None:
            import torch
            d = self._dev
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d["device"])   # noqa: E731
            d["obs"] = torch.cat([d["obs"], up(new_obs)])
            d["masks"] = torch.cat([d["masks"], up(new_masks.view(np.uint8))])
            d["labels"] = torch.cat([d["labels"], up(new_labels)])
        return len(keys)

    @classmethod
    def from_arrays(cls, observations, masks, labels, keys=None, groups=None, **kwargs):
        """A set over arrays that are already in memory (observations float32 [N, 4, D, D], masks bool [N, D, D], labels
        [N]); kwargs: the mode arguments of the constructor.  The validity rule is the caller's business here.
        groups: integers [N], equal for entries that may be compared (None: every entry a group of its own)."""
        self = cls([], **kwargs)
        self.observations = np.ascontiguousarray(observations, _f32)
        self.masks = np.ascontiguousarray(masks, bool)
        self.labels = np.ascontiguousarray(labels, _f32)
        n = len(self.observations)
        assert self.observations.shape[1:2] == (4,) and self.masks.shape == (n,) + self.observations.shape[2:] and self.labels.shape == (n,)
        self.keys = [f"{i:09d}" for i in range(n)] if keys is None else list(keys)
        self.groups = np.arange(n, dtype=np.int64) if groups is None else np.ascontiguousarray(groups, np.int64)
        if self.groups.shape != (n,):
            raise ValueError(f"ExperienceSet.from_arrays: groups of shape {self.groups.shape} for {n} entries")
        self._next_group = int(self.groups.max()) + 1 if n else 0
        self._members = None
        return self

    def __len__(self):
        return len(self.keys)

    @property
    def channels(self):
        """(first channel, channel count) of the recorded stack that a sample shows."""
        return (0, 3) if self.rgb_only else ((3, 1) if self.depth_only else (0, 4))

    @property
    def jitters(self):
        return self.rgb_only and self.obs_color_jitter

    def item_host(self, indices, params=None):
        """GraspDataset.__getitem__ for `indices` on the host: (obs [B, C, D, D], mask [B, D, D], label [B]) as numpy
        arrays; params (draw_jitter) are applied when the set jitters."""
        idx = np.asarray(indices, np.int64)
        off, cnt = self.channels
        obs = self.observations[idx, off:off + cnt]
        if self.jitters and params is not None:
            obs = color_jitter_host(obs, params)
        return np.ascontiguousarray(obs), self.masks[idx], self.labels[idx]

    def to_device(self, device):
        """Upload the set as recorded -- all four float32 channels, 64 KiB per sample at D = 64 -- so that the no-jitter
        path returns the recorded bits.  D = 64 only: the size the sample kernel serves."""
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("ExperienceSet.to_device: no GPU (the sample kernel is the only device path)")
        if self.observations.shape[-2:] != (OBS_DIM, OBS_DIM):
            raise ValueError(f"fs_replay_sample serves {OBS_DIM} x {OBS_DIM} observations, got {self.observations.shape[-2:]}")
        device = torch.device(device)
        self._dev = dict(device=device,
                         obs=torch.from_numpy(np.ascontiguousarray(self.observations)).to(device),
                         masks=torch.from_numpy(np.ascontiguousarray(self.masks).view(np.uint8)).to(device),
                         labels=torch.from_numpy(np.ascontiguousarray(self.labels)).to(device))
        return self

    def draw(self, batch_size, rng):
        """The host half of sample(): (indices int64 [B], jitter parameters or None) from `rng`."""
        if len(self) == 0:
            raise ValueError("ExperienceSet is empty")
        idx = rng.integers(0, len(self), size=int(batch_size))
        return idx, (draw_jitter(rng, batch_size) if self.jitters else None)

    def sample(self, batch_size, rng):
        """One training batch on the device: (obs [B, C, D, D] float32, mask [B, D, D] bool, label [B] float32), the
        arguments of run_sim.optimize's loop body.  Indices and jitter parameters are drawn on the host from `rng`
        (`draw`); gather, channel selection, quantisation, jitter, mask copy and label gather are ONE launch."""
        return self.gather(*self.draw(batch_size, rng))

    def group_members(self):
        """The groups in order of first appearance: a list of int64 index arrays, each in stored order."""
        if self._members is None:
            _, first, inverse = np.unique(self.groups, return_index=True, return_inverse=True)
            number = np.empty(len(first), np.int64)
            number[np.argsort(first, kind="stable")] = np.arange(len(first))
            numbered = number[inverse.ravel()]
            order = np.argsort(numbered, kind="stable").astype(np.int64)
            self._members = np.split(order, np.cumsum(np.bincount(numbered))[:-1]) if len(order) else []
        return self._members

    def draw_groups(self, batch_size, rng):
        """The host half of sample_groups(): (indices int64 [B], bounds int32 [B, 2], jitter parameters or None), a pure
        function of `rng`.  While room is left in the batch, g = rng.integers(0, number of groups) -- the groups numbered in
        order of first appearance -- and that group's members are appended in stored order, cut to the room that is left:
        one SEGMENT, also when a group comes twice.  bounds[i] = [begin, end) of sample i's segment in the batch.  Groups are
        drawn uniformly, so an entry's chance of being in a batch does not depend on the entry, as in draw(); only the last
        segment can be cut.  The jitter parameters are drawn after the indices, per sample, as draw() draws them."""
        if len(self) == 0:
            raise ValueError("ExperienceSet is empty")
        members = self.group_members()
        B = int(batch_size)
        idx, bounds, fill = np.empty(B, np.int64), np.empty((B, 2), np.int32), 0
        while fill < B:
            m = members[int(rng.integers(0, len(members)))][:B - fill]
            idx[fill:fill + len(m)] = m
            bounds[fill:fill + len(m)] = (fill, fill + len(m))
            fill += len(m)
        return idx, bounds, (draw_jitter(rng, B) if self.jitters else None)

    def sample_groups(self, batch_size, rng):
        """sample() over whole groups: (obs, mask, label, bounds int32 [B, 2] on the device) from draw_groups(), through the
        same gather -- one fs_replay_sample launch -- and one upload for the bounds.  The host copy stays with the device
        tensor as `bounds.host`: whoever validates the table (trainops.check_bounds) needs no download for it."""
        import torch

        idx, bounds, params = self.draw_groups(batch_size, rng)
        obs, mask, label = self.gather(idx, params)
        table = torch.from_numpy(bounds).to(self._dev["device"])
        table.host = bounds
        return obs, mask, label, table

    def gather(self, indices, params=None):
        """sample() for given indices and jitter parameters (None: the recorded floats unchanged)."""
        import torch

        if self._dev is None:
            raise RuntimeError("ExperienceSet.sample: call to_device() first (there is no host fallback; "
                               "item_host / color_jitter_host are the CPU path)")
        d = self._dev
        idx = np.asarray(indices, np.int64).ravel()
        if idx.size and (idx.min() < 0 or idx.max() >= len(self)):
            raise IndexError("ExperienceSet.gather: index out of range")
        B = int(idx.size)
        off, cnt = self.channels
        jitter = bool(self.jitters and params is not None)
        table = np.zeros((B, 9), np.int32)          # per sample: index, the order, the four factors' bits
        table[:, 0] = idx
        if jitter:
            order, factors = np.asarray(params["order"], np.int32), np.asarray(params["factors"], _f32)
            if order.shape != (B, 4) or factors.shape != (B, 4) or not (np.sort(order, axis=1) == np.arange(4)).all():
                raise ValueError("ExperienceSet.gather: params do not fit the batch (draw_jitter(rng, B))")
            table[:, 1:5] = order
            table[:, 5:9] = np.ascontiguousarray(factors).view(np.int32)
        dev = d["device"]
        obs = torch.empty((B, cnt, OBS_DIM, OBS_DIM), dtype=torch.float32, device=dev)
        mask = torch.empty((B, OBS_DIM, OBS_DIM), dtype=torch.bool, device=dev)
        label = torch.empty((B,), dtype=torch.float32, device=dev)
        if B == 0:
            return obs, mask, label
        stream_call("fs_replay_sample", dev, d["obs"], d["masks"], d["labels"], len(self), torch.from_numpy(table).to(dev), B,
                    off, cnt, int(jitter), OBS_DIM, obs, mask, label)
        return obs, mask, label


class MapSet:
    """The same files as a set of IMAGES: the entries that share one observation -- the executed cells of a measured reward map
    (probe.run_episodes with record_experience), the lanes of a look-ahead step that chose one transform -- become ONE stored
    image with a list of (pixel, label) pairs, for train.optimize_maps: one forward of the image, the last layer at its
    labelled pixels, one backward.  A 144-cell map is 64 KiB and 144 pairs here; in an ExperienceSet it is 144 copies.

    The files are read by ExperienceSet's own reader (read_entries) with the same arguments: the primitive, lane_ranks and
    validity filters, their counters and the label arithmetic are that code, so labels[l] is ExperienceSet's label of
    entry_keys[l] bit for bit.
    Two entries are one image when they are in one file, have equal '<key>/lane_task', '<key>/lane_step' and primitive, and their
    observations are byte-identical (the lanes of one step may have chosen different rotations or scales: those are different
    images).  An entry without lane fields is an image of its own.  A later entry of an image that names a pixel the image
    already lists is dropped and counted in `n_duplicate` (the kernels keep one gradient per pixel of an image).
    Host arrays: images float32 [M, 4, D, D] in order of first appearance, offsets int64 [M + 1] (image i owns list positions
    [offsets[i], offsets[i + 1])), pixels int32 [L] (flat y * D + x; within an image in stored -- key -- order), labels float32
    [L], entry_keys (the key of each list position).  len() is M.  Loading holds the unique images and the entry being read,
    never the copies."""

    def __init__(self, paths, action_primitive=None, rgb_only=True, depth_only=False, obs_color_jitter=True,
                 use_normalized_coverage=True, lane_ranks=None):
        assert not depth_only or not rgb_only
        self.lane_ranks = None if lane_ranks is None else frozenset(int(r) for r in lane_ranks)
        self.rgb_only, self.depth_only = bool(rgb_only), bool(depth_only)
        self.obs_color_jitter = bool(obs_color_jitter)
        self.use_normalized_coverage = bool(use_normalized_coverage)
        self.action_primitive = action_primitive
        self.n_invalid = self.n_without_arrays = self.n_filtered = self.n_duplicate = 0
        self.images = np.zeros((0, 4, OBS_DIM, OBS_DIM), _f32)
        self.offsets = np.zeros(1, np.int64)
        self.pixels = np.zeros(0, np.int32)
        self.labels = np.zeros(0, _f32)
        self.entry_keys = []
        self._dev = None
        self.extend(paths)

    channels = ExperienceSet.channels
    jitters = ExperienceSet.jitters

    def __len__(self):
        return int(self.images.shape[0])

    def _read(self, paths):
        """(images, per image: [(pixel, label, key), ...]) of `paths`, images in order of first appearance."""
        images, lists, seen = [], [], []       # seen[i]: the pixels image i lists
        candidates = {}                         # (file, lane_task, lane_step, primitive) -> the images found there so far
        for e in read_entries(self, paths):
            o = e["observation"]
            pixel = int(np.flatnonzero(e["mask"])[0])
            where = None if e["lane"] is None else (e["file"],) + e["lane"] + (e["primitive"],)
            index = None
            for i in candidates.get(where, ()) if where is not None else ():
                if images[i].shape == o.shape and images[i].tobytes() == o.tobytes():
                    index = i
                    break
            if index is None:
                index = len(images)
                images.append(o)
                lists.append([])
                seen.append(set())
                if where is not None:
                    candidates.setdefault(where, []).append(index)
            if pixel in seen[index]:
                self.n_duplicate += 1
                continue
            seen[index].add(pixel)
            lists[index].append((pixel, e["label"], e["key"]))
        return images, lists

    def extend(self, paths):
        """Add the images of further files, through the constructor's filters; the result equals a set built from all files at
        once (an image never spans two files).  A set that is on a device uploads the new images only.  Returns the number of
        images added."""
        images, lists = self._read(paths)
        if not images:
            return 0
        new = np.stack(images)
        del images
        if new.shape[1:] != self.images.shape[1:]:
            if len(self):
                raise ValueError(f"MapSet.extend: observations of {new.shape[1:]} do not fit the set's {self.images.shape[1:]}")
            if self._dev is not None and new.shape[-2:] != (OBS_DIM, OBS_DIM):
                raise ValueError(f"fs_replay_sample serves {OBS_DIM} x {OBS_DIM} observations, got {new.shape[-2:]}")
        flat = [row for rows in lists for row in rows]
        self.images = np.concatenate([self.images, new]) if len(self) else new
        self.offsets = np.concatenate([self.offsets, self.offsets[-1] + np.cumsum([len(rows) for rows in lists], dtype=np.int64)])
        self.pixels = np.concatenate([self.pixels, np.array([r[0] for r in flat], np.int32)])
        self.labels = np.concatenate([self.labels, np.array([r[1] for r in flat], _f64).astype(_f32)])
        self.entry_keys = list(self.entry_keys) + [r[2] for r in flat]
        if self._dev is not None:
            import torch
            d = self._dev
            d["obs"] = torch.cat([d["obs"], torch.from_numpy(np.ascontiguousarray(new)).to(d["device"])])
            self._dummies()
        return int(new.shape[0])

    @classmethod
    def from_arrays(cls, images, offsets, pixels, labels, entry_keys=None, **kwargs):
        """A set over arrays that are already in memory (the fields of the class docstring); kwargs: the mode arguments of the
        constructor.  The table is validated (trainops.check_pixel_table: distinct pixels per image)."""
        from .trainops import check_pixel_table

        self = cls([], **kwargs)
        self.images = np.ascontiguousarray(images, _f32)
        assert self.images.ndim == 4 and self.images.shape[1] == 4, self.images.shape
        self.offsets = check_pixel_table(offsets, pixels, len(self.images))
        self.pixels = np.ascontiguousarray(pixels, np.int32)
        self.labels = np.ascontiguousarray(labels, _f32)
        assert self.labels.shape == self.pixels.shape
        self.entry_keys = [f"{i:09d}" for i in range(len(self.pixels))] if entry_keys is None else list(entry_keys)
        return self

    def to_device(self, device):
        """Upload the images as recorded, once: all four float32 channels, 64 KiB per IMAGE at D = 64.  The pixel and label
        lists stay on the host; a batch's part of them travels with the batch (sample_maps)."""
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("MapSet.to_device: no GPU (the sample kernel is the only device path)")
        if self.images.shape[-2:] != (OBS_DIM, OBS_DIM):
            raise ValueError(f"fs_replay_sample serves {OBS_DIM} x {OBS_DIM} observations, got {self.images.shape[-2:]}")
        device = torch.device(device)
        self._dev = dict(device=device, obs=torch.from_numpy(np.ascontiguousarray(self.images)).to(device))
        self._dummies()
        return self

    def _dummies(self):
        """fs_replay_sample also copies a mask and a label per row; an image has neither, so it is given zeros to copy."""
        import torch
        d = self._dev
        d["masks"] = torch.zeros((len(self), OBS_DIM, OBS_DIM), dtype=torch.uint8, device=d["device"])
        d["labels"] = torch.zeros(len(self), dtype=torch.float32, device=d["device"])

    def resident_bytes(self):
        """Bytes the set holds on its device (0 before to_device)."""
        return 0 if self._dev is None else sum(int(t.numel()) * t.element_size() for k, t in self._dev.items() if k != "device")

    def draw_maps(self, n_images, rng, pixels_per_image=None):
        """The host half of sample_maps(): (image indices int64 [n], offsets int64 [n + 1], list positions int64 [L'], jitter
        parameters or None), a pure function of `rng`.  First the image indices, uniformly and with repetition (an image drawn
        twice is two images of the batch); then, per drawn image in order, all its list positions -- or, when it has more than
        `pixels_per_image`, those at sorted(rng.choice(count, pixels_per_image, replace=False)); then the jitter parameters, one
        per IMAGE, as draw_jitter draws them.  offsets is the batch's own CSR table over the positions."""
        if len(self) == 0:
            raise ValueError("MapSet is empty")
        n = int(n_images)
        if pixels_per_image is not None and int(pixels_per_image) < 1:
            raise ValueError("MapSet.draw_maps: pixels_per_image >= 1")
        idx = rng.integers(0, len(self), size=n)
        positions, offsets = [], np.zeros(n + 1, np.int64)
        for k, i in enumerate(idx):
            first, count = int(self.offsets[i]), int(self.offsets[i + 1] - self.offsets[i])
            if pixels_per_image is not None and count > int(pixels_per_image):
                take = first + np.sort(rng.choice(count, int(pixels_per_image), replace=False)).astype(np.int64)
            else:
                take = np.arange(first, first + count, dtype=np.int64)
            positions.append(take)
            offsets[k + 1] = offsets[k] + len(take)
        positions = np.concatenate(positions) if positions else np.zeros(0, np.int64)
        return idx, offsets, positions, (draw_jitter(rng, n) if self.jitters else None)

    def sample_maps(self, n_images, rng, pixels_per_image=None):
        """One training batch of images: (obs [n, C, D, D] float32, offsets int64 [n + 1] on the HOST, pix int32 [L'] with its
        host copy as `pix.host`, labels float32 [L']) from draw_maps().  On a set that is on a device the images go through
        ExperienceSet's gather launch (fs_replay_sample: one table row per image -- channel selection, quantisation and jitter as
        there; its mask and label outputs are not used) and the pixel and label lists go up in ONE upload.  A set that is not on
        a device returns host tensors through color_jitter_host: the CPU path."""
        return self._batch(*self.draw_maps(n_images, rng, pixels_per_image))

    def take_maps(self, indices):
        """sample_maps' deterministic sibling: the images `indices` in the given order, each with ALL its list positions and as
        recorded -- no jitter (ExperienceSet.gather(idx, None) on a device set, the recorded floats with the channel selection on
        the host), nothing drawn, `rng` not involved.  The same return shape: (obs, offsets, pix with `.host`, labels).  What
        train.score_maps walks a held-out set with."""
        idx = np.asarray(indices, np.int64).ravel()
        if idx.size and (idx.min() < 0 or idx.max() >= len(self)):
            raise IndexError("MapSet.take_maps: index out of range")
        counts = self.offsets[idx + 1] - self.offsets[idx]
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        positions = [np.arange(self.offsets[i], self.offsets[i + 1], dtype=np.int64) for i in idx]
        return self._batch(idx, offsets, np.concatenate(positions) if positions else np.zeros(0, np.int64), None)

    def _batch(self, idx, offsets, positions, params):
        """The batch of draw_maps' / take_maps' (indices, offsets, positions, jitter parameters or None)."""
        import torch

        count = len(positions)
        padded = (count + 3) // 4 * 4              # both halves of the upload start on a 16-byte boundary
        lists = np.zeros((2, padded), np.int32)
        lists[0, :count] = self.pixels[positions]
        lists[1, :count] = self.labels[positions].view(np.int32)
        off, cnt = self.channels
        jitter = bool(self.jitters and params is not None)
        if self._dev is None:
            obs = self.images[idx, off:off + cnt]
            if jitter:
                obs = color_jitter_host(obs, params)
            obs, both = torch.from_numpy(np.ascontiguousarray(obs)), torch.from_numpy(lists)
        else:
            obs, _, _ = ExperienceSet.gather(self, idx, params)   # (an image is a row of `_dev` like an entry is)
            both = torch.from_numpy(lists).to(self._dev["device"])
        pix, labels = both[0, :count], both[1, :count].view(torch.float32)
        pix.host = lists[0, :count]
        return obs, offsets, pix, labels
