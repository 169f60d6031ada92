"""The training half of run_sim.py: `optimize` (run_sim.py:16-34) and the collect / update loop (:53-109) on one GPU.

    policy = nets.MaximumValuePolicy(...); optimizer = make_optimizer(policy)
    run(policy, optimizer, env, tasks, log_dir, rounds=100, tasks_per_round=96, seed=0)

    python -m flingbot_amd.train --log runs/a --tasks train.npz --action_expl_prob 1 --value_expl_prob 1 --rounds 100

The reference interleaves single environment steps with updates: sixteen ray actors step on their own, and after every
`policy.act` the loop decays the exploration probabilities and runs `batches_per_update` updates per primitive.  Here
collection is evaluate.run_tasks -- every slot of a GPU context busy, one batched forward for all ready slots -- so the
loop runs in ROUNDS: collect `tasks_per_round` episodes with the exploration probabilities as they stand,
write them as one replay file, then run the reference's loop body once for each action the round recorded.  The number of
decays and updates per recorded action is the reference's; what differs is that the policy that collects a round is the
one the previous round left.

The update itself is stock PyTorch except for the sixteen 16 -> 16 convolutions, whose forward, data gradient and weight
gradient are HIP kernels (trainops.Conv16Function, csrc/fs_vntrain.hip) when the net is in train() mode on the GPU, and the 17
BatchNorm sites, whose batch statistics, activation and residual add are HIP kernels forward and backward
(trainops.BatchNormAct16Function, csrc/fs_bntrain.hip) when nets._TRAIN_BN_HIP is set.  With hip_step=True (--hip-step) the rest is
HIP too (csrc/fs_edgetrain.hip): the first layer, the last layer at the one pixel per sample the loss reads (trainops.ConvInFunction,
trainops.HeadPixelFunction), and Adam (HipAdam: one fs_adam_step launch per group).
Batches come from replay.ExperienceSet.sample: one launch per batch, colour jitter included.
With rank_weight > 0 (--rank-weight) the batches are whole groups of comparable entries (ExperienceSet.sample_groups: the lanes of
one observation side by side) and the loss gains a pairwise ranking term over each group, value and gradient in one launch
(trainops.GroupLossFunction, csrc/fs_grouploss.hip).
`optimize_maps` / `fit_maps` (--fit-maps) train on recorded reward maps as images with many labelled pixels each (replay.MapSet): one
forward of the image, the last layer at its labelled pixels (SpatialValueNet.forward_pixels, trainops.HeadPixelsFunction), one backward.
With map_loss=True (--map-loss) their loss is trainops.MapLossFunction (csrc/fs_maploss.hip): the ranking term over whole maps,
whatever images x labels comes to, normalised per label or per image (--per-image).
With list_weight > 0 (--list-weight) the loss gains a LISTWISE term, trainops.MapListFunction (csrc/fs_maplist.hip): per map -- in
`optimize`, per group of lanes -- the KL divergence between softmax(label / T) and softmax(prediction / T), O(K) where the pairwise
term is O(K^2), with its weight at the top of the list.
`score_maps` (--score-maps; inside fit_maps with --holdout-maps) scores recorded maps the weights were NOT trained on: the eval
forward of the stored images, then every per-map rank statistic -- regret, chosen rank, Spearman, pair accuracy -- in one launch
(trainops.map_score, csrc/fs_mapscore.hip), and a dozen means on the host.
"""
import contextlib
import glob
import json
import os

import numpy as np
import torch

TRAIN_LOG = "train_log.jsonl"
LATEST = "latest_ckpt.pth"


class HipAdam(torch.optim.Adam):
    """torch.optim.Adam whose step() is ONE launch for all parameters of a group (libflingsim fs_adam_step,
    csrc/fs_edgetrain.hip) instead of PyTorch's multi-tensor path.  The state is stock Adam's -- per parameter `step` (a float32
    scalar on the host), `exp_avg`, `exp_avg_sq` -- and so are the param_groups, so state_dicts load in both directions.  A
    parameter whose grad is None is skipped, as stock Adam skips it.  Parameters and gradients are CUDA fp32 (ValueError
    otherwise); amsgrad, maximize, capturable, differentiable, fused and decoupled_weight_decay are refused."""
    n_launches = 0   # fs_adam_step calls so far (the tests count them)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, **kwargs):
        for name in ("amsgrad", "maximize", "capturable", "differentiable", "fused", "decoupled_weight_decay"):
            if kwargs.get(name):
                raise ValueError(f"HipAdam does not support {name}")
        if torch.is_tensor(lr) or any(torch.is_tensor(b) for b in betas):
            raise ValueError("HipAdam takes lr and betas as floats")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **kwargs)

    def load_state_dict(self, state_dict):
        """torch.optim.Adam's, then `step` back to the host: a checkpoint read with map_location=<device> (load_checkpoint)
        arrives with every tensor on the device, and stock Adam leaves a non-capturable `step` where it finds it."""
        super().load_state_dict(state_dict)
        for state in self.state.values():
            if torch.is_tensor(state.get("step")) and state["step"].is_cuda:
                state["step"] = state["step"].cpu()

    @torch.no_grad()
    def step(self, closure=None):
        from torch.optim.optimizer import _get_scalar_dtype
        from . import sim as fsim

        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            for name in ("amsgrad", "maximize", "capturable", "differentiable", "fused", "decoupled_weight_decay"):
                if group.get(name):   # a loaded state_dict can bring them
                    raise ValueError(f"HipAdam does not support {name}")
            beta1, beta2 = group["betas"]
            launches = {}   # (device index, step count) -> segments; the tensors are kept alive until the launch is queued
            for p in group["params"]:
                grad = p.grad
                if grad is None:
                    continue
                if not (p.is_cuda and p.dtype == torch.float32 and grad.is_cuda and grad.dtype == torch.float32
                        and not grad.is_sparse and grad.device == p.device and grad.shape == p.shape):
                    raise ValueError(f"HipAdam serves CUDA fp32 parameters and gradients, got {p.dtype} on {p.device} with a "
                                     f"{grad.dtype} gradient on {grad.device}")
                if not p.is_contiguous():
                    raise ValueError("HipAdam: parameters are contiguous")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=_get_scalar_dtype())
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                m, v = state["exp_avg"], state["exp_avg_sq"]
                if not (m.is_cuda and v.is_cuda and m.device == v.device == p.device and m.dtype == v.dtype == torch.float32
                        and m.is_contiguous() and v.is_contiguous() and m.shape == v.shape == p.shape):
                    raise ValueError("HipAdam: exp_avg and exp_avg_sq are contiguous CUDA fp32 tensors of the parameter's shape")
                if p.numel() == 0:
                    continue
                if torch.is_tensor(state["step"]) and state["step"].is_cuda:
                    raise ValueError("HipAdam: `step` lives on the host (a capturable or fused optimizer's state was loaded)")
                state["step"] += 1
                grad = grad.contiguous()
                launches.setdefault((p.device.index, int(state["step"])), []).append((p, grad, m, v))
            for (device, t), members in launches.items():
                table = (fsim.AdamSegment * len(members))()
                for seg, (p, grad, m, v) in zip(table, members):
                    seg.param, seg.grad, seg.exp_avg, seg.exp_avg_sq, seg.count = p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
                fsim.stream_call("fs_adam_step", device, table, len(members), float(group["lr"]), float(beta1), float(beta2),
                                 float(group["eps"]), float(group["weight_decay"]), 1.0 - float(beta1) ** t, 1.0 - float(beta2) ** t)
                HipAdam.n_launches += 1
        return loss


def make_optimizer(policy, lr=1e-3, weight_decay=1e-6, hip=False):
    """utils.setup_network's optimizer (utils.py:102-104): Adam over ALL of the policy's parameters -- the exploration
    scalars and step counters included, which never get a gradient -- so that its state_dict is indexed like the
    reference's.  hip: a HipAdam, whose step is one launch (same state_dict)."""
    if hip:
        return HipAdam(policy.parameters(), lr=lr, weight_decay=weight_decay)
    return torch.optim.Adam(policy.parameters(), lr=lr, weight_decay=weight_decay)


def _list_arguments(name, list_weight, list_temperature, label_temperature):
    """True when the listwise term is on (list_weight > 0).  ValueError for a negative or non-finite list_weight and for a
    temperature that is not positive and finite (label_temperature None: equal to list_temperature), and for
    list_temperature='fit', which optimize_maps and fit_maps resolve before they come here."""
    if isinstance(list_temperature, str):
        raise ValueError(f"{name}: list_temperature={list_temperature!r} -- a fitted temperature ('fit') is served by optimize_maps "
                         f"and fit_maps only")
    values = [float(list_weight), float(list_temperature), float(list_temperature if label_temperature is None else label_temperature)]
    if not (np.isfinite(values).all() and values[0] >= 0.0 and values[1] > 0.0 and values[2] > 0.0):
        raise ValueError(f"{name}: list_weight >= 0, list_temperature > 0 and label_temperature > 0 (or None), all finite")
    return values[0] > 0.0


def group_offsets(bounds, batch):
    """The segment table of a grouped batch (ExperienceSet.sample_groups; validated by trainops.check_bounds) as CSR offsets, int64
    numpy [groups + 1]: the groups are the contiguous distinct rows of `bounds`, in order -- group k owns samples [offsets[k],
    offsets[k + 1]).  ValueError when the table does not tile [0, batch) that way."""
    from .trainops import check_bounds

    table = check_bounds(bounds, batch)
    starts = np.flatnonzero(np.concatenate([[True], (table[1:] != table[:-1]).any(axis=1)]))
    offsets = np.concatenate([starts, [int(batch)]]).astype(np.int64)
    if not (np.array_equal(table[starts, 0], offsets[:-1]) and np.array_equal(table[starts, 1], offsets[1:])):
        raise ValueError("group offsets: the groups must be the contiguous distinct rows of bounds, in order")
    return offsets


def optimize(key, value_net, optimizer, data, num_updates, batch_size, rng, hip_step=False, rank_weight=0.0,
             rank_temperature=0.1, rank_min_gap=0.0, stats=None, list_weight=0.0, list_temperature=0.1, label_temperature=None):
    """run_sim.optimize (run_sim.py:16-34) with `data.sample(batch_size, rng)` in place of the DataLoader: `num_updates`
    times dense prediction -> the one pixel per sample the action mask names -> mse_loss -> zero_grad / backward / step ->
    `value_net.steps += 1`.  Nothing happens when the set is smaller than a batch (utils.get_loader returns None then) or
    there is no optimizer.  The caller puts the policy into train() before and eval() after.  `key` names the primitive
    (the reference uses it for its TensorBoard tag).  Returns the losses as floats.
    hip_step: the prediction comes from value_net.forward_selected inside nets.train_edge_hip() -- first layer and last layer
    in libflingsim, the last one at the mask's pixel only -- instead of the dense map and masked_select.
    rank_weight > 0: the batch is `data.sample_groups(batch_size, rng)` -- whole groups of comparable entries, the lanes of one
    observation side by side -- and the loss is trainops.GroupLossFunction: mse + rank_weight * the mean over the pairs (i, j) of
    one group with label_i > label_j + rank_min_gap of softplus(-(pred_i - pred_j) / rank_temperature), value and gradient in one
    fs_group_loss launch on the GPU.  The default temperature of 0.1 is a guess at the scale of the label differences within a
    group; nobody has measured it.  Every such update appends {'loss', 'mse', 'rank', 'pairs', 'concordant'} to the list `stats`
    when one is given: the kernel's statistics row, fetched in the one download that fetches the loss.  A set without groups
    is no error: every segment is one sample, there is no pair and the update is the regression's.  With rank_weight = 0 (the
    default) nothing of this is touched: data.sample and torch's mse_loss, as before.  ValueError for a negative or non-finite
    rank_weight or rank_min_gap and for a rank_temperature that is not positive and finite.
    list_weight > 0: the batch is `data.sample_groups` too, also with rank_weight = 0, and whatever loss the path above uses gains
    trainops.MapListFunction over the groups (group_offsets turns `bounds` into CSR offsets; ValueError when the groups are not
    its contiguous distinct rows, in order): list_weight * the mean over the labels of groups of at least two of the group's KL
    divergence between softmax(label / label_temperature) and softmax(pred / list_temperature); label_temperature=None means
    equal to list_temperature.  Both defaults are guesses, as the rank temperature is; nobody has measured them.  A batch whose
    groups are all single samples has no listed group: the term is absent and the update is the regression's.  Every such update
    appends a row to `stats` that also carries 'list' (the unweighted term), 'listed_images', 'top1_hits', 'chosen_mass' and
    'best_mass' (0 / 0 / 0 / None / None when the term is absent) and, without rank_weight, 'mse'; 'loss' is the sum the update
    used.  With list_weight = 0 (the default) nothing of this runs.  list_temperature='fit' is a ValueError here: the fitted
    temperature is optimize_maps' and fit_maps', over recorded maps."""
    rank_weight, rank_temperature, rank_min_gap = float(rank_weight), float(rank_temperature), float(rank_min_gap)
    if not (np.isfinite([rank_weight, rank_temperature, rank_min_gap]).all() and rank_weight >= 0.0 and rank_temperature > 0.0
            and rank_min_gap >= 0.0):
        raise ValueError("optimize: rank_weight >= 0, rank_temperature > 0 and rank_min_gap >= 0, all finite")
    ranked = rank_weight > 0.0
    listed = _list_arguments("optimize", list_weight, list_temperature, label_temperature)
    losses = []
    if data is None or optimizer is None or len(data) < batch_size:
        return losses
    device = next(value_net.parameters()).device
    for _ in range(int(num_updates)):
        if ranked or listed:
            obs, action_mask, label, bounds = data.sample_groups(batch_size, rng)
        else:
            obs, action_mask, label = data.sample(batch_size, rng)
        if hip_step:
            from . import nets
            with nets.train_edge_hip():
                value_pred = value_net.forward_selected(obs.to(device, non_blocking=True), action_mask.to(device, non_blocking=True))
        else:
            value_pred_dense = value_net(obs.to(device, non_blocking=True))
            value_pred = torch.masked_select(value_pred_dense.squeeze(), action_mask.to(device, non_blocking=True))
        if ranked:
            from .trainops import GroupLossFunction
            loss, row = GroupLossFunction.apply(value_pred, label.to(device, non_blocking=True), bounds, rank_weight,
                                                rank_temperature, rank_min_gap)
        else:
            loss = torch.nn.functional.mse_loss(value_pred, label.to(device, non_blocking=True))
        list_row = None
        if listed:
            offsets = group_offsets(bounds, value_pred.shape[0])
            base = loss.detach()
            if (np.diff(offsets) >= 2).any():   # (otherwise no group is listed: the term is absent)
                from .trainops import MapListFunction
                term, list_row, _ = MapListFunction.apply(value_pred, label.to(device, non_blocking=True), offsets, float(list_weight),
                                                          float(list_temperature), label_temperature, False)
                loss = loss + term
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        value_net.steps += 1
        if listed:
            # one download: the total, the path's own row (or its mse alone) and the list statistics
            head = row.double() if ranked else base.double().reshape(1)
            tail = list_row.double() if list_row is not None else torch.zeros(0, dtype=torch.float64, device=head.device)
            got = torch.cat([loss.detach().double().reshape(1), head, tail]).cpu().tolist()
            losses.append(got[0])
            if stats is not None:
                own = got[1:1 + len(head)]
                line = {"loss": got[0], "mse": own[1] if ranked else own[0]}
                if ranked:
                    line.update(rank=own[2], pairs=int(own[3]), concordant=int(own[4]))
                ls = got[1 + len(head):]
                if ls:
                    line.update(list=ls[1], listed_images=int(ls[2]), top1_hits=int(ls[4]), chosen_mass=ls[5], best_mass=ls[6])
                else:
                    line.update(list=0.0, listed_images=0, top1_hits=0, chosen_mass=None, best_mass=None)
                stats.append(line)
        elif ranked:
            row = row.cpu().tolist()   # loss, mse, rank, P, C: the loss comes with its statistics
            losses.append(row[0])
            if stats is not None:
                stats.append({"loss": row[0], "mse": row[1], "rank": row[2], "pairs": int(row[3]), "concordant": int(row[4])})
        else:
            losses.append(loss.cpu().item())
    return losses


def optimize_maps(key, value_net, optimizer, data, num_updates, images_per_batch, rng, pixels_per_image=None, hip_step=False,
                  rank_weight=0.0, rank_temperature=0.1, rank_min_gap=0.0, stats=None, map_loss=False, per_image=False,
                  list_weight=0.0, list_temperature=0.1, label_temperature=None, refit_every=100, temperature_range=(1e-3, 1e2),
                  refits=None, fit_state=None):
    """optimize's loop body over IMAGES with many labelled pixels each (replay.MapSet: the executed cells of a measured reward
    map share one observation): `num_updates` times `data.sample_maps(images_per_batch, rng, pixels_per_image)` -> ONE forward of
    the images -> the prediction at every labelled pixel (value_net.forward_pixels) -> loss -> zero_grad / backward / step ->
    `value_net.steps += 1`.  The loss is mse_loss over the [L'] vector of all labels of the batch: a mean over LABELS, not over
    images, so an image with many labels weighs more than one with few (map_loss=True, per_image=True weighs images alike).
    pixels_per_image: an image with more labels than this contributes a random subset of that size (MapSet.draw_maps).
    hip_step: the forward runs inside nets.train_edge_hip() -- first layer in libflingsim, last layer at the listed pixels only
    (trainops.HeadPixelsFunction: fs_head_forward_pixels / fs_head_backward_pixels).
    rank_weight > 0: the loss is trainops.GroupLossFunction with one segment per image, bounds[l] = [offsets[b], offsets[b + 1])
    for the labels l of image b: pairs are compared within one image only.  fs_group_loss serves at most 4096 predictions, so
    this needs pixels_per_image with images_per_batch * pixels_per_image <= 4096: ValueError up front otherwise.
    Every update appends {'loss', 'images', 'labels'} -- the batch's image and label counts -- to the list `stats` when one is
    given, and with rank_weight > 0 also 'mse', 'rank', 'pairs' and 'concordant', as optimize does.
    map_loss=True: the loss of every update is trainops.MapLossFunction (fs_map_loss: every image's pairs found by workgroups of
    its own, any number of images and labels, at most 4096 labels in one image) -- also with rank_weight = 0, which is then the
    regression under the chosen normalisation.  The 4096 refusal does not apply and pixels_per_image is optional.  per_image=True
    (ValueError without map_loss): mse is the mean over the images of the image's mean squared error and rank the mean over the
    images with pairs of the image's mean over its pairs, so a 170-cell map weighs what a 30-cell map does; False: the means over
    labels and over pairs, as above.  Every row of `stats` then carries 'loss', 'images', 'labels', 'mse', 'rank', 'pairs',
    'concordant', 'images_with_pairs' and 'map_pair_accuracy': the mean of C_b / P_b over the images with pairs (None without any).
    With map_loss=False nothing of this is touched.
    list_weight > 0 (ValueError without map_loss): the loss gains trainops.MapListFunction (fs_map_list_loss, O(K) per image):
    list_weight * the KL divergence, per image with at least two labels, between softmax(label / label_temperature) and
    softmax(pred / list_temperature), normalised as per_image says; label_temperature=None means equal to list_temperature, where
    the term is 0 exactly when pred - label is constant over each image, so it does not pull against the regression.  The defaults
    (0.1, equal temperatures) are guesses at the scale of the label differences within a map; the label temperature defines the
    target and stays a choice, the prediction temperature can be fitted (below).  Every
    row of `stats` then also carries 'list' (the unweighted term), 'listed_images', 'top1_hits' (the listed images whose arg-max
    of the prediction is the arg-max of the label), 'chosen_mass' and 'best_mass' (the mean target mass at the net's choice, and
    its ceiling), fetched in the download that fetches the row, and 'loss' is the sum the update used.  With list_weight = 0
    (the default) none of this runs.  ValueError for a negative or non-finite list_weight and for temperatures that are not
    positive and finite.
    list_temperature='fit' (needs list_weight > 0 and an explicit label_temperature -- with None the target would move with the
    fit -- ValueError otherwise): the prediction temperature is FITTED to the training maps.  Before the first update, and then
    every `refit_every` updates, all images of `data` go through the eval forward as recorded (MapSet.take_maps, no jitter: the
    path score_maps walks) and trainops.fit_temperature (fs_map_list_sweep: a few sweeps over all labels, not one per batch)
    finds the temperature in `temperature_range` = (lo, hi) at which the term over them, normalised as per_image says, is
    smallest; the following updates use it.  When the fit sits at an end of the range or no image has two labels, the previous
    value is kept; the first such fallback is the default 0.1.  The refit sees eval-mode BatchNorm (running statistics), while the
    updates' predictions are made with batch statistics: the fitted value is the one the checkpoint will be scored at, not
    exactly the one the next batch sees.  Each refit appends {'step', 'list_temperature', 'previous', 'list_kl', 'at_bound',
    'sweeps'} to the list `refits` when one is given.  `fit_state`: a dict that carries {'temperature', 'updates'} from one
    call to the next, so that calls on one rng count as one run (fit_maps' segments); None: this call is a run of its own.
    Nothing happens (and [] is returned) when the set holds fewer than `images_per_batch` images or there is no optimizer.  The
    caller puts the policy into train() before and eval() after.  ValueError for the rank arguments as in optimize."""
    rank_weight, rank_temperature, rank_min_gap = float(rank_weight), float(rank_temperature), float(rank_min_gap)
    if not (np.isfinite([rank_weight, rank_temperature, rank_min_gap]).all() and rank_weight >= 0.0 and rank_temperature > 0.0
            and rank_min_gap >= 0.0):
        raise ValueError("optimize_maps: rank_weight >= 0, rank_temperature > 0 and rank_min_gap >= 0, all finite")
    ranked = rank_weight > 0.0
    if pixels_per_image is not None and int(pixels_per_image) < 1:
        raise ValueError("optimize_maps: pixels_per_image >= 1")
    if per_image and not map_loss:
        raise ValueError("optimize_maps: per_image=True needs map_loss=True")
    fitted = isinstance(list_temperature, str) and list_temperature == "fit"
    if fitted:
        _fit_arguments("optimize_maps", list_weight, label_temperature, refit_every, temperature_range)
        fit_state = {} if fit_state is None else fit_state
        fit_state.setdefault("temperature", 0.1)
        fit_state.setdefault("updates", 0)
        list_temperature = fit_state["temperature"]
    listed = _list_arguments("optimize_maps", list_weight, list_temperature, label_temperature)
    if listed and not map_loss:
        raise ValueError("optimize_maps: list_weight > 0 needs map_loss=True")
    if ranked and not map_loss and (pixels_per_image is None or int(images_per_batch) * int(pixels_per_image) > 4096):
        raise ValueError("optimize_maps: rank_weight > 0 needs pixels_per_image with images_per_batch * pixels_per_image <= 4096 "
                         "(fs_group_loss serves at most 4096 predictions)")
    losses = []
    if data is None or optimizer is None or len(data) < images_per_batch:
        return losses
    from . import nets
    device = next(value_net.parameters()).device
    for _ in range(int(num_updates)):
        if fitted:
            if fit_state["updates"] % int(refit_every) == 0:
                fit = _fit_recorded_maps(value_net, data, label_temperature, per_image, temperature_range)
                previous = fit_state["temperature"]
                if fit["temperature"] is not None and fit["at_bound"] is None:
                    fit_state["temperature"] = fit["temperature"]
                if refits is not None:
                    refits.append({"step": int(value_net.steps), "list_temperature": fit_state["temperature"], "previous": previous,
                                   "list_kl": fit["list"], "at_bound": fit["at_bound"], "sweeps": fit["sweeps"]})
            list_temperature = fit_state["temperature"]
            fit_state["updates"] += 1
        obs, offsets, pix, label = data.sample_maps(images_per_batch, rng, pixels_per_image)
        host = getattr(pix, "host", None)
        obs, pix, label = obs.to(device, non_blocking=True), pix.to(device, non_blocking=True), label.to(device, non_blocking=True)
        if host is not None:
            pix.host = host   # (.to() of a tensor that is already there returns it; of a host tensor, a new one)
        with nets.train_edge_hip() if hip_step else contextlib.nullcontext():
            value_pred = value_net.forward_pixels(obs, offsets, pix)
        if map_loss:
            from .trainops import MapLossFunction
            loss, row, rows = MapLossFunction.apply(value_pred, label, offsets, rank_weight, rank_temperature, rank_min_gap,
                                                    bool(per_image))
            if listed:
                from .trainops import MapListFunction
                list_term, list_row, _ = MapListFunction.apply(value_pred, label, offsets, float(list_weight), float(list_temperature),
                                                               label_temperature, bool(per_image))
                loss = loss + list_term
                row = torch.cat([row, list_row.to(row.dtype), loss.detach().to(row.dtype).reshape(1)])   # one download below
        elif ranked:
            from .trainops import GroupLossFunction
            bounds = np.repeat(np.stack([offsets[:-1], offsets[1:]], axis=1), np.diff(offsets), axis=0).astype(np.int32)
            table = torch.from_numpy(bounds).to(device)
            table.host = bounds
            loss, row = GroupLossFunction.apply(value_pred, label, table, rank_weight, rank_temperature, rank_min_gap)
        else:
            loss = torch.nn.functional.mse_loss(value_pred, label)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        value_net.steps += 1
        sizes = {"images": int(len(offsets) - 1), "labels": int(offsets[-1])}
        if map_loss:
            row, rows = row.cpu().tolist(), rows.cpu().numpy()   # loss, mse, rank, P, C, G', G''; per image .., P_b, C_b
            if listed:
                losses.append(row[16])                                                            # (the sum the update used)
            else:
                losses.append(float(np.float32(row[0])) if loss.dtype == torch.float32 else row[0])   # (the loss the update used)
            with_pairs = rows[:, 2] > 0
            sizes.update(loss=losses[-1], mse=row[1], rank=row[2], pairs=int(row[3]), concordant=int(row[4]),
                         images_with_pairs=int(row[6]),
                         map_pair_accuracy=float(np.mean(rows[with_pairs, 3].astype(np.float64) / rows[with_pairs, 2]))
                         if with_pairs.any() else None)
            if listed:
                sizes.update(list=row[9], listed_images=int(row[10]), top1_hits=int(row[12]), chosen_mass=row[13], best_mass=row[14])
        elif ranked:
            row = row.cpu().tolist()   # loss, mse, rank, P, C: the loss comes with its statistics
            losses.append(row[0])
            sizes.update(loss=row[0], mse=row[1], rank=row[2], pairs=int(row[3]), concordant=int(row[4]))
        else:
            losses.append(loss.cpu().item())
            sizes["loss"] = losses[-1]
        if stats is not None:
            stats.append(sizes)
    return losses


def _fit_arguments(name, list_weight, label_temperature, refit_every, temperature_range):
    """What list_temperature='fit' needs: ValueError unless list_weight > 0, label_temperature is given, refit_every >= 1 and
    temperature_range is (lo, hi) with 0 < lo < hi, finite."""
    if not float(list_weight) > 0.0:
        raise ValueError(f"{name}: list_temperature='fit' needs list_weight > 0")
    if label_temperature is None:
        raise ValueError(f"{name}: list_temperature='fit' needs an explicit label_temperature (with None the target would move "
                         f"with the fit)")
    if int(refit_every) < 1:
        raise ValueError(f"{name}: refit_every >= 1")
    _temperature_range(name, temperature_range)


def _temperature_range(name, temperature_range):
    try:
        lo, hi = (float(v) for v in temperature_range)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: temperature_range is (lo, hi)") from None
    if not (0.0 < lo < hi < float("inf")):
        raise ValueError(f"{name}: temperature_range is (lo, hi) with 0 < lo < hi, finite")
    return lo, hi


def _labelled_predictions(value, offsets, pix):
    """The dense maps' values at the labelled pixels, [L] float32: position l of image b reads value[b] at flat pixel pix[l]."""
    images = len(offsets) - 1
    image = torch.repeat_interleave(torch.arange(images, device=value.device), torch.as_tensor(np.diff(offsets), device=value.device))
    return value.reshape(images, -1)[image, pix.long()].float()


def _join_maps(preds, labels, counts):
    """The batches of a set as one (pred [L], label [L], offsets [G + 1]); None for a set without a label."""
    if not preds:
        return None
    return torch.cat(preds), torch.cat(labels), np.concatenate([[0], np.cumsum(np.concatenate(counts))]).astype(np.int64)


def _fit_recorded_maps(net, data, label_temperature, per_image, temperature_range, images_per_batch=64):
    """trainops.fit_temperature over ALL images of `data` as recorded, under the net's current weights: the eval-mode forward of
    score_maps (folded HIP forward on a GPU; every module's `training` flag and the generators are put back), the predictions at
    the labelled pixels kept on the device, one fit over the whole set."""
    from . import trainops

    lo, hi = _temperature_range("fit", temperature_range)
    device = next(net.parameters()).device
    flags = [(m, m.training) for m in net.modules()]
    preds, labels, counts = [], [], []
    try:
        net.eval()
        with torch.no_grad(), torch.random.fork_rng(devices=[]):
            if device.type == "cuda" and net._hip is None:
                net.fold_batchnorm(hip=True)
            for first in range(0, len(data), int(images_per_batch)):
                obs, offsets, pix, label = data.take_maps(np.arange(first, min(first + int(images_per_batch), len(data))))
                counts.append(np.diff(offsets))
                if int(offsets[-1]) == 0:
                    continue
                preds.append(_labelled_predictions(net(obs.to(device)), offsets, pix.to(device)))
                labels.append(label.to(device).float())
    finally:
        for m, flag in flags:
            m.train(flag)
    joined = _join_maps(preds, labels, counts)
    if joined is None:
        return dict(temperature=None, list=None, slope=None, at_bound=None, sweeps=0, chosen=[], first_curve=[])
    return trainops.fit_temperature(*joined, label_temperature, per_image, lo=lo, hi=hi)


def _map_sets(policy, paths):
    """{primitive: replay.MapSet} of `paths` for the policy's value nets, on the policy's device when that is a GPU: one set per
    primitive, in the nets' channel mode.  A dict {primitive: MapSet} of ready sets is taken as it is."""
    from . import replay

    if isinstance(paths, dict):
        return {key: paths[key] for key in policy.value_nets if key in paths}
    device = torch.device(policy.device)
    first = policy.value_nets[next(iter(policy.value_nets))]
    mode = dict(rgb_only=bool(first.rgb_only), depth_only=bool(first.depth_only))
    sets = {}
    for key in policy.value_nets:
        sets[key] = replay.MapSet(paths, action_primitive=key, **mode)
        if device.type == "cuda":
            sets[key].to_device(device)
    return sets


def score_maps(policy, paths, images_per_batch=64, min_gap=0.0, list_temperature=None, label_temperature=None,
               fit_temperature=False, temperature_range=(1e-3, 1e2)):
    """Recorded reward maps scored under the policy's CURRENT weights, without a simulator: {primitive: summary} over the images
    of `paths` (the files fit_maps takes; or {primitive: replay.MapSet} of ready sets), one replay.MapSet per primitive.  Per
    primitive, in stored image order and `images_per_batch` at a time: MapSet.take_maps (the recorded floats, no jitter) -> the
    dense value maps of the eval-mode forward -> trainops.map_score (fs_map_score: every per-map statistic in one launch) -> the
    rows of all batches, read back once -> trainops.summarize_scores.  On a GPU the forward is the folded HIP one
    (fs_value_net_forward): a net that has not folded is folded here, a stale fold is renewed by the forward itself.
    "chosen" is the arg-max of the scored weights over the recorded cells, regret is in label units.  Runs under policy.eval() and
    torch.no_grad(), restores every module's `training` flag, and touches neither parameters, optimizer state nor any generator
    (folding builds layers, whose initialisation draws: the generator's state is put back).
    list_temperature (None: not asked for, and nothing below runs): every summary gains 'list_kl', 'chosen_mass' and 'best_mass',
    the listwise figures of trainops.MapListFunction at that temperature (label_temperature None: the same one) -- per map with
    at least two labels the KL divergence between softmax(label / T) and softmax(prediction / T), the target mass at the
    arg-max of the prediction and the largest target mass -- as means over those maps, None without any.  The predictions at the
    labelled pixels are gathered from the dense maps and go through the term's entry once per batch, with weight 1 and its
    gradient discarded (per_image=True: every map weighs the same); the batches' means are read back once and combined on the
    host, each weighted by its number of such maps.
    fit_temperature=True (label_temperature must be given: ValueError otherwise; list_temperature is not needed): the predictions
    and labels at the recorded pixels of ALL batches are kept on the device and trainops.fit_temperature runs ONCE over the whole
    set, with per_image=True as list_kl is formed: the prediction temperature in `temperature_range` = (lo, hi) at which list_kl
    is smallest.  Every summary gains 'list_fit': {'temperature', 'list_kl' (there), 'at_bound' (None, 'low' or 'high': the
    minimum lies outside the range), 'slope', 'sweeps', 'curve'}, the curve being the first sweep's 33 temperatures over the
    range, each {'temperature', 'list_kl', 'expected_regret' (label units, like regret), 'best_draw', 'greedy_draw'}: what drawing
    a recorded cell with probability softmax(prediction / T) loses against the best cell, how often it draws the best cell, and
    how often the arg-max -- the trade-off a --lane-temperature sets.  A set without a map of two labels has temperature None."""
    from . import trainops

    if int(images_per_batch) < 1:
        raise ValueError("score_maps: images_per_batch >= 1")
    if list_temperature is not None:
        _list_arguments("score_maps", 1.0, list_temperature, label_temperature)
    if fit_temperature:
        if label_temperature is None:
            raise ValueError("score_maps: fit_temperature=True needs label_temperature")
        _list_arguments("score_maps", 1.0, label_temperature, label_temperature)
        lo, hi = _temperature_range("score_maps", temperature_range)
    sets = _map_sets(policy, paths)
    flags = [(m, m.training) for m in policy.modules()]
    out = {}
    try:
        policy.eval()
        with torch.no_grad(), torch.random.fork_rng(devices=[]):
            for key, data in sets.items():
                net = policy.value_nets[key]
                device = next(net.parameters()).device
                if device.type == "cuda" and net._hip is None:
                    net.fold_batchnorm(hip=True)
                rows, listwise = [], []
                preds, labels, counts = [], [], []
                for first in range(0, len(data), int(images_per_batch)):
                    obs, offsets, pix, label = data.take_maps(np.arange(first, min(first + int(images_per_batch), len(data))))
                    counts.append(np.diff(offsets))
                    if int(offsets[-1]) == 0:   # a batch without a label: nothing to launch
                        rows.append(torch.from_numpy(trainops.empty_score_rows(len(offsets) - 1)).to(device))
                        continue
                    host = pix.host
                    obs, pix, label = obs.to(device), pix.to(device), label.to(device)
                    pix.host = host
                    value = net(obs)
                    rows.append(trainops.map_score(value, offsets, pix, label, min_gap))
                    if fit_temperature:
                        preds.append(_labelled_predictions(value, offsets, pix))
                        labels.append(label.float())
                    if list_temperature is not None:
                        image = torch.repeat_interleave(torch.arange(len(offsets) - 1, device=device),
                                                        torch.as_tensor(np.diff(offsets), device=device))
                        pred = value.reshape(len(offsets) - 1, -1)[image, pix.long()]
                        listwise.append(trainops.MapListFunction.apply(pred.float(), label.float(), offsets, 1.0, list_temperature,
                                                                       label_temperature, True)[1].double())
                out[key] = trainops.summarize_scores(torch.cat(rows).cpu().numpy() if rows else trainops.empty_score_rows(0))
                if list_temperature is not None:
                    got = torch.stack(listwise).cpu().numpy() if listwise else np.zeros((0, 8))
                    maps = got[:, 2].sum()
                    mean = lambda k: float((got[:, k] * got[:, 2]).sum() / maps) if maps else None   # noqa: E731
                    out[key].update(list_kl=mean(1), chosen_mass=mean(5), best_mass=mean(6))
                if fit_temperature:
                    joined = _join_maps(preds, labels, counts)
                    fit = (trainops.fit_temperature(*joined, label_temperature, True, lo=lo, hi=hi) if joined is not None
                           else dict(temperature=None, list=None, slope=None, at_bound=None, sweeps=0, first_curve=[]))
                    out[key]["list_fit"] = dict(
                        temperature=fit["temperature"], list_kl=fit["list"], at_bound=fit["at_bound"], slope=fit["slope"],
                        sweeps=fit["sweeps"],
                        curve=[dict(temperature=c["temperature"], list_kl=c["list"], expected_regret=c["expected_regret"],
                                    best_draw=c["best_draw"], greedy_draw=c["greedy_draw"]) for c in fit["first_curve"]])
    finally:
        for m, flag in flags:   # parents before children: every module ends on its own flag, and a net that was training
            m.train(flag)       # marks the fold made here stale, as any train() phase does
    return out


def _image_hashes(data):
    import hashlib

    return [hashlib.sha1(np.ascontiguousarray(image).tobytes()).digest() for image in data.images]


def fit_maps(policy, optimizer, paths, log_dir, updates, images_per_batch=32, pixels_per_image=None, seed=0, hip_step=False,
             rank_weight=0.0, rank_temperature=0.1, rank_min_gap=0.0, load_latest=True, map_loss=False, per_image=False,
             holdout=None, validate_every=0, list_weight=0.0, list_temperature=0.1, label_temperature=None, refit_every=100,
             temperature_range=(1e-3, 1e2)):
    """Train on recorded files without a simulator: `updates` optimize_maps updates per primitive on the images of `paths`
    (replay files of `evaluate --probe-stride N --record-experience`, of look-ahead rounds, or ordinary ones: replay.MapSet, one
    per primitive, on the policy's device).
    Resume: with load_latest a latest_ckpt.pth in log_dir is loaded into policy and optimizer first, as train.run does.  The
    batches are drawn from np.random.default_rng([seed, 2]).  One JSON line per update goes to log_dir/train_log.jsonl: {'fit':
    true, 'primitive', 'step', 'loss', 'images', 'labels'} and, with rank_weight > 0, 'mse', 'rank', 'pairs' and 'pair_accuracy'
    (concordant / pairs of the batch, or null without pairs).  map_loss / per_image as in optimize_maps (trainops.MapLossFunction:
    whole maps, no cap on the batch; per_image=True without map_loss is a ValueError): every line then carries 'mse', 'rank',
    'pairs', 'pair_accuracy', 'images_with_pairs' and 'map_pair_accuracy' (the mean over the images with pairs of the image's
    own concordant / pairs, or null), whatever rank_weight is.  latest_ckpt.pth and ckpt_{steps:06d}.pth are written at the end.
    A primitive whose set holds fewer than images_per_batch images gets no update.  hip_step as in optimize_maps: such updates
    run outside deterministic_library_convs(), the others inside it.
    Returns {'primitives': {key: {'images', 'labels', 'duplicates', 'updates', 'mean_loss'}}, 'steps'}.
    holdout: files (or ready sets, as score_maps takes them) the fit does NOT train on.  They are scored with score_maps under
    rank_min_gap before the first update, after every `validate_every` updates (0: not in between) and after the last one; each
    score is a line {'validate': true, 'primitive', 'step', **summary} in train_log.jsonl, and the result gains 'validation':
    {primitive: {'before', 'after'}} and 'holdout_overlap': the held-out images whose bytes equal a training image's of the same
    primitive (by a hash of the image bytes; reported, not refused).  The updates then run as optimize_maps calls of validate_every
    updates on the same rng: the batches drawn, and so the parameters, are those of one uninterrupted call.  Without holdout
    neither the log nor the result changes.
    list_weight, list_temperature, label_temperature as in optimize_maps (trainops.MapListFunction; list_weight > 0 without
    map_loss is a ValueError; the default label temperature is a guess, not measured, and stays a choice): every update's line
    then also carries 'list', 'listed_images', 'top1_hits', 'chosen_mass' and 'best_mass', and every 'validate' line and the
    `validation` block 'list_kl', 'chosen_mass' and 'best_mass' of the held-out maps at those temperatures (score_maps).  With
    list_weight = 0 every file the fit writes is what it was without these arguments.
    list_temperature='fit' with refit_every and temperature_range as in optimize_maps (list_weight > 0 and an explicit
    label_temperature: ValueError otherwise): per primitive the prediction temperature is fitted to ALL training maps
    (trainops.fit_temperature over the eval forward of the images as recorded) before the first update and then every
    refit_every updates, counted over the whole fit whatever validate_every is; a fit at an end of the range keeps the previous
    value, the first fallback being 0.1.  Each refit is one line {'refit': true, 'primitive', 'step' (the net's at the refit),
    'list_temperature' (in force from here on), 'previous', 'list_kl' (the training maps' term at the fitted value), 'at_bound',
    'sweeps'} in train_log.jsonl, written before the lines of the updates that follow it; 'validate' lines and the result are
    scored at the temperature in force, and the primitive's summary gains 'list_temperature'.  The refit sees eval-mode
    BatchNorm, while the updates' predictions are made with batch statistics.  Nothing is added to the checkpoints: a resumed run
    refits before its first update.  With a numeric list_temperature every file is what it was without these arguments."""
    from . import replay

    if per_image and not map_loss:
        raise ValueError("fit_maps: per_image=True needs map_loss=True")
    fitted = isinstance(list_temperature, str) and list_temperature == "fit"
    if fitted:
        _fit_arguments("fit_maps", list_weight, label_temperature, refit_every, temperature_range)
    listed = _list_arguments("fit_maps", list_weight, 0.1 if fitted else list_temperature, label_temperature)
    if listed and not map_loss:
        raise ValueError("fit_maps: list_weight > 0 needs map_loss=True")
    list_options = dict(list_weight=list_weight, list_temperature=list_temperature, label_temperature=label_temperature) if listed else {}
    score_options = dict(list_temperature=list_temperature, label_temperature=label_temperature) if listed else {}
    refits, fit_state = [], {}
    if fitted:
        list_options.update(refit_every=refit_every, temperature_range=temperature_range, refits=refits)
    if int(validate_every) < 0:
        raise ValueError("fit_maps: validate_every >= 0")
    os.makedirs(log_dir, exist_ok=True)
    latest = os.path.join(log_dir, LATEST)
    if load_latest and os.path.exists(latest):
        load_checkpoint(latest, policy, optimizer)
    device = torch.device(policy.device)
    first = policy.value_nets[next(iter(policy.value_nets))]
    mode = dict(rgb_only=bool(first.rgb_only), depth_only=bool(first.depth_only))
    ranked = float(rank_weight) > 0.0
    rng = np.random.default_rng([int(seed), 2])
    summary = {}
    held = None if holdout is None else _map_sets(policy, holdout)
    validation, overlap = {}, 0
    with open(os.path.join(log_dir, TRAIN_LOG), "a") as log:
        def validate(key, net):
            """One score of the primitive's held-out set under the weights as they stand, logged; the summary."""
            if fitted:
                score_options["list_temperature"] = fit_state.get("temperature", 0.1)   # the one in force
            score = score_maps(policy, {key: held[key]}, min_gap=rank_min_gap, **score_options)[key]
            log.write(json.dumps({"validate": True, "primitive": key, "step": int(net.steps), **score}) + "\n")
            return score

        for key, net in policy.value_nets.items():
            data = replay.MapSet(paths, action_primitive=key, **mode)
            if device.type == "cuda":
                data.to_device(device)
            validated = held is not None and key in held
            if fitted:
                fit_state = {}   # (per primitive; validate reads it)
                list_options["fit_state"] = fit_state
            if validated:
                trained = set(_image_hashes(data))
                overlap += sum(h in trained for h in _image_hashes(held[key]))
                validation[key] = {"before": validate(key, net)}
            # one call of `updates` updates -- or, between two scores, calls of validate_every updates on the same rng
            segment = int(validate_every) if validated and int(validate_every) > 0 else int(updates)
            losses, done = [], 0
            while True:
                rows = []
                policy.train()
                with contextlib.nullcontext() if hip_step else deterministic_library_convs():
                    before = int(net.steps)
                    losses += optimize_maps(key, net, optimizer, data, min(segment, int(updates) - done), images_per_batch, rng,
                                            pixels_per_image=pixels_per_image, hip_step=hip_step, rank_weight=rank_weight,
                                            rank_temperature=rank_temperature, rank_min_gap=rank_min_gap, stats=rows,
                                            map_loss=map_loss, per_image=per_image, **list_options)
                policy.eval()
                for u, row in enumerate(rows):
                    while refits and refits[0]["step"] <= before + u:
                        log.write(json.dumps({"refit": True, "primitive": key, **refits.pop(0)}) + "\n")
                    line = {"fit": True, "primitive": key, "step": before + u + 1, "loss": row["loss"], "images": row["images"],
                            "labels": row["labels"]}
                    if ranked or map_loss:
                        line.update(mse=row["mse"], rank=row["rank"], pairs=row["pairs"],
                                    pair_accuracy=row["concordant"] / row["pairs"] if row["pairs"] else None)
                    if map_loss:
                        line.update(images_with_pairs=row["images_with_pairs"], map_pair_accuracy=row["map_pair_accuracy"])
                    if listed:
                        line.update({name: row[name] for name in ("list", "listed_images", "top1_hits", "chosen_mass", "best_mass")})
                    log.write(json.dumps(line) + "\n")
                done += segment
                if done >= int(updates) or not rows:   # (no rows: the set is too small for a batch, and stays so)
                    break
                validate(key, net)
            if validated:
                validation[key]["after"] = validate(key, net)
            summary[key] = {"images": len(data), "labels": int(data.offsets[-1]), "duplicates": int(data.n_duplicate),
                            "updates": len(losses), "mean_loss": float(np.mean(losses)) if losses else None}
            if fitted:
                summary[key]["list_temperature"] = fit_state.get("temperature", 0.1)
    save_checkpoint(latest, policy, optimizer)
    save_checkpoint(os.path.join(log_dir, f"ckpt_{int(policy.steps()):06d}.pth"), policy, optimizer)
    out = {"primitives": summary, "steps": int(policy.steps())}
    if held is not None:
        out.update(validation=validation, holdout_overlap=int(overlap))
    return out


def save_checkpoint(path, policy, optimizer):
    """The reference's checkpoint (run_sim.py:87-88): {'net': policy.state_dict(), 'optimizer': optimizer.state_dict()}."""
    torch.save({"net": policy.state_dict(), "optimizer": optimizer.state_dict()}, path)


def load_checkpoint(path, policy, optimizer=None, map_location=None):
    """utils.setup_network's load (utils.py:114-118); the optimizer state is optional (an evaluation needs the net only)."""
    ckpt = torch.load(path, map_location=policy.device if map_location is None else map_location)
    policy.load_state_dict(ckpt["net"])
    if optimizer is not None:
        optimizer.load_state_dict(ckpt["optimizer"])
    return ckpt


def replay_files(log_dir):
    """The rounds' replay files already in log_dir, in round order."""
    return sorted(glob.glob(os.path.join(log_dir, "replay_[0-9][0-9][0-9][0-9][0-9].npz")))


def _entries(path):
    return int(len(np.load(path, allow_pickle=False)["keys"]))


def round_seed(seed, r):
    """The exploration seed of round r: a non-negative integer that is a function of (seed, r) alone."""
    return int(np.random.SeedSequence([int(seed), int(r)]).generate_state(1)[0])


@contextlib.contextmanager
def deterministic_library_convs(on=True):
    """The library convolutions that remain in a step (first and last layer) may pick weight-gradient kernels that add with
    atomics; inside this context they are asked for their deterministic forms, so that a run is a function of its seed.
    Only that switch is touched: `torch.backends.cudnn.flags(deterministic=True)` would also switch the library off."""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = bool(on)
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = before


def plan_round(entries_before, ranks, warmup, update_frequency, save_ckpt):
    """What the loop does for each entry a round recorded: one (decay, update, checkpoint) triple per entry, a pure function.
    ranks[t]: the look-ahead rank of entry t (all 0 without lanes).  With i = entries_before + t counting from the data-set
    size before the round (run_sim.py:52) and size = entries_before + len(ranks) the size after it:
      decay       i > warmup and ranks[t] == 0: the exploration probabilities decay once per OBSERVATION, as the reference
                  decays them once per policy decision -- the K lanes of a step are one decision;
      update      size > warmup and i % update_frequency == 0: per stored label, the reference's ratio of updates to entries;
      checkpoint  size > warmup and i % save_ckpt == 0."""
    entries_before, size = int(entries_before), int(entries_before) + len(ranks)
    plan = []
    for t, rank in enumerate(ranks):
        i = entries_before + t
        plan.append((i > warmup and int(rank) == 0, size > warmup and i % update_frequency == 0,
                     size > warmup and i % save_ckpt == 0))
    return plan


def run(policy, optimizer, env, tasks, log_dir, rounds, tasks_per_round, seed, batch_size=128, warmup=128,
        update_frequency=1, batches_per_update=1, save_ckpt=512, load_latest=True, hip_step=False, lookahead=None,
        follow="policy", rank_weight=0.0, rank_temperature=0.1, rank_min_gap=0.0, lanes="winners", lane_temperature=0.1,
        lane_separation=0, lane_on_cloth=True, sample_first=False, list_weight=0.0, list_temperature=0.1,
        label_temperature=None):
    """`rounds` rounds of collect -> record -> update (the module docstring has the correspondence with run_sim.py).

    policy / optimizer: nets.MaximumValuePolicy and make_optimizer(policy); env: BatchedFlingEnv(record_experience=True);
    tasks: a list of tasks, walked in order and wrapped around like TaskLoader(repeat=True).
    Resume: the replay files already in log_dir are read back, the round counter continues from their number, and with
    load_latest a latest_ckpt.pth in log_dir is loaded into policy and optimizer first.
    Per round r: s_r = round_seed(seed, r) seeds the exploration draws (key (s_r, task index in the round, action number));
    log_dir/replay_{r:05d}.npz; then for each recorded action, with i counting from the data-set size (run_sim.py:52):
    decay_exploration() when i > warmup; when the set holds more than `warmup` entries and i % update_frequency == 0,
    optimize(..., batches_per_update) for every primitive, and ckpt_{steps:06d}.pth when i % save_ckpt == 0.
    latest_ckpt.pth is written once per round; one JSON line per update goes to log_dir/train_log.jsonl.
    hip_step: the updates are optimize(..., hip_step=True) and run OUTSIDE deterministic_library_convs(): no library
    convolution is left in such a step, so it is a function of its seed as it is.
    lookahead = K: a round collects through lookahead.run_waves(policy, env, chosen, K, follow=follow, seed=s_r) -- at every
    step the K best different actions of the observation, each on a copy of the episode -- and the round's file holds one
    entry per executed lane-step (lookahead.save_replay; keys count on from the entries already recorded), K labels per
    observation.  plan_round says what each entry triggers: decays per observation, updates and checkpoints per label.  The
    round's summary row gains 'lookahead' (k, follow, regret, rank0_best_frac, mean_reward_per_rank, n_steps, n_lane_steps), which
    is also written as one line of train_log.jsonl; 'final_coverage' is that of the followed trajectories.  A log directory
    may mix rounds collected with and without lanes.  ValueError for K < 1, more lanes than the context has slots, or an
    unknown `follow`.
    lanes, lane_temperature, lane_separation, lane_on_cloth, sample_first: lookahead.run_waves' own (lanes="sampled": the K
    actions are drawn with probability ~ exp(value / lane_temperature), keyed by (s_r, task, step); lookahead=1 with
    sample_first is Boltzmann exploration); the round's 'lookahead' row then also holds lanes, lane_temperature and refused.
    ValueError for lanes other than "winners" without lookahead.
    rank_weight > 0: the updates are optimize(..., rank_weight, rank_temperature, rank_min_gap) -- grouped batches and the
    pairwise ranking term (trainops.GroupLossFunction).  Each update's line of train_log.jsonl then also carries 'mse', 'rank',
    'pairs' and 'pair_accuracy' (concordant / pairs of the batch, or null without pairs), and the round's summary row -- and its
    look-ahead line in the log -- a top-level 'collected_pair_accuracy': lookahead.pair_agreement over the lanes the round has
    just collected, the net's recorded values against the rewards with the same rank_min_gap.  The net has not trained on those
    lanes yet, so it is a held-out figure; null without look-ahead or without pairs.  With rank_weight = 0 every file the run
    leaves is what it was without these arguments.
    list_weight > 0: the updates are optimize(..., list_weight, list_temperature, label_temperature) -- grouped batches, also with
    rank_weight = 0, and the listwise term over each group (trainops.MapListFunction).  Each update's line of train_log.jsonl
    then also carries 'list', 'listed_images', 'top1_hits', 'chosen_mass' and 'best_mass' (and 'mse').  With list_weight = 0
    every file the run leaves is what it was without these arguments.  list_temperature='fit' is a ValueError: the fitted
    temperature belongs to fit_maps, over recorded maps.
    Returns {'first_round', 'rounds': [per round: round, entries, updates, mean loss, steps, the probabilities]}."""
    from . import evaluate, replay, taskio

    if not getattr(env, "record_experience", False):
        raise ValueError("train.run: the environment must be made with record_experience=True")
    if not len(tasks):
        raise ValueError("train.run: no tasks")
    ranked = float(rank_weight) > 0.0
    listed = _list_arguments("train.run", list_weight, list_temperature, label_temperature)
    list_options = dict(list_weight=list_weight, list_temperature=list_temperature, label_temperature=label_temperature) if listed else {}
    if lookahead is not None:
        from . import lookahead as flook
        if follow not in ("policy", "best"):
            raise ValueError(f"train.run: follow must be 'policy' or 'best', not {follow!r}")
        if int(lookahead) < 1 or int(lookahead) > env.sim.n_envs:
            raise ValueError(f"train.run: lookahead = {lookahead} needs 1 <= K <= the context's {env.sim.n_envs} slots")
        lookahead = int(lookahead)
        flook.check_lanes(lanes, lane_temperature, lane_separation, seed)
    elif lanes != "winners":
        raise ValueError(f"train.run: lanes = {lanes!r} needs lookahead = K")
    lane_options = dict(lanes=lanes, lane_temperature=lane_temperature, lane_separation=lane_separation,
                        lane_on_cloth=lane_on_cloth, sample_first=sample_first)
    os.makedirs(log_dir, exist_ok=True)
    latest = os.path.join(log_dir, LATEST)
    if load_latest and os.path.exists(latest):
        load_checkpoint(latest, policy, optimizer)
    device = torch.device(policy.device)
    first = policy.value_nets[next(iter(policy.value_nets))]
    mode = dict(rgb_only=bool(first.rgb_only), depth_only=bool(first.depth_only))
    done = replay_files(log_dir)
    sets = {}
    for key in policy.value_nets:
        sets[key] = replay.ExperienceSet(done, action_primitive=key, **mode)
        if device.type == "cuda":
            sets[key].to_device(device)
    size = sum(_entries(p) for p in done)
    first_round = len(done)
    summary = []
    with open(os.path.join(log_dir, TRAIN_LOG), "a") as log:
        for r in range(first_round, first_round + int(rounds)):
            chosen = [tasks[(r * tasks_per_round + j) % len(tasks)] for j in range(tasks_per_round)]
            policy.eval()
            path = os.path.join(log_dir, f"replay_{r:05d}.npz")
            if lookahead is None:
                stats = evaluate.run_tasks(policy, env, chosen, seed=round_seed(seed, r))
                n = taskio.save_replay(path, stats["records"], chosen, first_episode=r * tasks_per_round)
                ranks = [0] * n
            else:
                stats = flook.run_waves(policy, env, chosen, lookahead, follow=follow, seed=round_seed(seed, r), **lane_options)
                n = flook.save_replay(path, stats, chosen, first_record=size)
                ranks = [int(rec["rank"]) for rec in stats["lane_records"]]   # step-major, then task, then rank ascending
            for data in sets.values():
                data.extend([path])
            plan = plan_round(size, ranks, warmup, update_frequency, save_ckpt)
            size += n
            rng = np.random.default_rng([int(seed), int(r), 1])
            losses = []
            for decay, update, checkpoint in plan:
                if decay:
                    policy.decay_exploration()
                if update:
                    policy.train()
                    with contextlib.nullcontext() if hip_step else deterministic_library_convs():
                        for key, net in policy.value_nets.items():
                            rows = []
                            got = optimize(key, net, optimizer, sets[key], batches_per_update, batch_size, rng,
                                           hip_step=hip_step, rank_weight=rank_weight, rank_temperature=rank_temperature,
                                           rank_min_gap=rank_min_gap, stats=rows, **list_options)
                            for u, loss in enumerate(got):
                                losses.append(loss)
                                line = {"round": r, "primitive": key, "step": int(net.steps), "loss": loss}
                                if ranked:
                                    row = rows[u]
                                    line.update(mse=row["mse"], rank=row["rank"], pairs=row["pairs"],
                                                pair_accuracy=row["concordant"] / row["pairs"] if row["pairs"] else None)
                                if listed:
                                    line.update({name: rows[u][name] for name in
                                                 ("mse", "list", "listed_images", "top1_hits", "chosen_mass", "best_mass")})
                                log.write(json.dumps(line) + "\n")
                    policy.eval()
                if checkpoint:
                    save_checkpoint(os.path.join(log_dir, f"ckpt_{int(policy.steps()):06d}.pth"), policy, optimizer)
            save_checkpoint(latest, policy, optimizer)
            summary.append({"round": r, "entries": size, "new_entries": n, "updates": len(losses),
                            "mean_loss": float(np.mean(losses)) if losses else None, "steps": int(policy.steps()),
                            "action_expl_prob": float(policy.action_expl_prob), "value_expl_prob": float(policy.value_expl_prob),
                            "final_coverage": stats["mean"]["final_coverage"]})
            if ranked:
                pairs, concordant = flook.pair_agreement(stats["lookahead"]["steps"], rank_min_gap) if lookahead is not None else (0, 0)
                summary[-1]["collected_pair_accuracy"] = concordant / pairs if pairs else None
            if lookahead is not None:
                summary[-1]["lookahead"] = {name: stats["lookahead"][name] for name in
                                            ("k", "follow", "regret", "rank0_best_frac", "mean_reward_per_rank", "n_steps", "n_lane_steps")
                                            + (("lanes", "lane_temperature", "refused") if lanes == "sampled" else ())}
                line = {"round": r, "entries": size, "new_entries": n, "lookahead": summary[-1]["lookahead"]}
                if ranked:
                    line["collected_pair_accuracy"] = summary[-1]["collected_pair_accuracy"]
                log.write(json.dumps(line) + "\n")
            log.flush()
    return {"first_round": first_round, "rounds": summary}


def _temperature_or_fit(text):
    """--list-temperature: a number, or the word 'fit'."""
    return "fit" if text == "fit" else float(text)


def build_parser():
    """The reference's flag names (utils.config_parser, utils.py:17-87) for what this loop has, plus --slots, --rounds and
    --tasks-per-round."""
    import argparse

    class Parser(argparse.ArgumentParser):
        def parse_known_args(self, args=None, namespace=None):
            a, rest = super().parse_known_args(args, namespace)
            if a.score_maps is not None:
                if a.fit_maps is not None or a.tasks is not None:
                    self.error("--score-maps runs no updates: not together with --fit-maps or --tasks")
            elif a.tasks is None and a.fit_maps is None:   # --tasks is required, except by --fit-maps and --score-maps
                self.error("the following arguments are required: --tasks")
            if a.fit_maps is None and (a.holdout_maps is not None or a.validate_every):
                self.error("--holdout-maps and --validate-every go with --fit-maps")
            if a.validate_every and a.holdout_maps is None:
                self.error("--validate-every needs --holdout-maps")
            return a, rest

    ap = Parser(description=main.__doc__)
    ap.add_argument("--log", type=str, required=True, help="run directory: replay files, checkpoints, train_log.jsonl")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--load", type=str, default=None, help="checkpoint to start from (default: <log>/latest_ckpt.pth if it exists)")
    ap.add_argument("--tasks", type=str, default=None, help=".npz task set (flingbot_amd/taskio.py); required unless --fit-maps")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--batch_size", type=int, default=128)
    ap.add_argument("--weight_decay", type=float, default=1e-6)
    ap.add_argument("--batches_per_update", type=int, default=1)
    ap.add_argument("--update_frequency", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=128)
    ap.add_argument("--save_ckpt", type=int, default=512)
    ap.add_argument("--action_expl_prob", type=float, default=0.0)
    ap.add_argument("--action_expl_decay", type=float, default=0.9995)
    ap.add_argument("--value_expl_prob", type=float, default=0.0)
    ap.add_argument("--value_expl_decay", type=float, default=0.995)
    ap.add_argument("--action_primitives", choices=["fling", "stretchdrag", "drag", "place"], default=["fling"], nargs="+")
    ap.add_argument("--slots", type=int, default=96, help="episodes resident on the GPU at a time")
    ap.add_argument("--rounds", type=int, default=1, help="rounds of collect + update in this call")
    ap.add_argument("--tasks-per-round", type=int, default=96, help="episodes collected per round")
    ap.add_argument("--episode-length", type=int, default=10)
    ap.add_argument("--device", type=int, default=0, help="HIP device")
    ap.add_argument("--hip-step", action="store_true", help="every pass of an update in libflingsim: first layer, last layer at the "
                    "action's pixel and Adam too (HipAdam), outside the deterministic-library context")
    ap.add_argument("--lookahead", type=int, default=None, metavar="K",
                    help="collect with look-ahead rollouts (flingbot_amd/lookahead.py): the K best different actions of every "
                         "observation run side by side on copies of the episode, and every executed lane-step becomes a replay "
                         "entry -- K labels per observation; K <= --slots")
    ap.add_argument("--follow", choices=("policy", "best"), default="policy",
                    help="--lookahead: continue an episode from the net's own arg-max (policy) or from the lane with the highest reward (best)")
    from .evaluate import add_lane_arguments
    add_lane_arguments(ap)
    ap.add_argument("--rank-weight", type=float, default=0.0, metavar="W",
                    help="weight of the pairwise ranking term over the labels of one observation (grouped batches, "
                         "trainops.GroupLossFunction: one fs_group_loss launch); 0: the regression alone, as before")
    ap.add_argument("--rank-temperature", type=float, default=0.1, metavar="T",
                    help="--rank-weight: the prediction difference that counts as a clear margin (a guess, not measured)")
    ap.add_argument("--rank-min-gap", type=float, default=0.0, metavar="G",
                    help="--rank-weight: two labels form a pair only when they differ by more than this; also the pairs that "
                         "--holdout-maps and --score-maps count")
    ap.add_argument("--fit-maps", type=str, nargs="+", default=None, metavar="FILE",
                    help="no collection: train on these recorded replay files as IMAGES with many labelled pixels each "
                         "(replay.MapSet, train.fit_maps) -- the files of `evaluate --probe-stride N --record-experience`; "
                         "takes --updates, --images-per-batch, --pixels-per-image, --hip-step and the --rank-* options")
    ap.add_argument("--updates", type=int, default=500, help="--fit-maps: updates per primitive")
    ap.add_argument("--images-per-batch", type=int, default=32, help="--fit-maps: images per update")
    ap.add_argument("--pixels-per-image", type=int, default=None, metavar="K",
                    help="--fit-maps: an image with more labels contributes a random K of them per update (needed with "
                         "--rank-weight: images x K <= 4096, unless --map-loss)")
    ap.add_argument("--map-loss", action="store_true",
                    help="--fit-maps: the loss is trainops.MapLossFunction (fs_map_loss) -- whole maps in the ranking term, no "
                         "cap on images x labels; also with --rank-weight 0")
    ap.add_argument("--per-image", action="store_true",
                    help="--map-loss: average per image first, so that every image weighs the same whatever its label count")
    ap.add_argument("--list-weight", type=float, default=0.0, metavar="W",
                    help="weight of the listwise term (trainops.MapListFunction, fs_map_list_loss): per map, or per group of lanes, "
                         "the KL divergence between softmax(label / T) and softmax(prediction / T); with --fit-maps it needs "
                         "--map-loss; 0: absent, as before")
    ap.add_argument("--list-temperature", type=_temperature_or_fit, default=None, metavar="T",
                    help="--list-weight: the temperature of the prediction's softmax (default 0.1), or 'fit' (with --fit-maps and "
                         "--label-temperature): fitted to the training maps before the first update and every --refit-every "
                         "updates (trainops.fit_temperature, fs_map_list_sweep); given as a number with --score-maps, the printed "
                         "summary gains list_kl, chosen_mass and best_mass at that temperature")
    ap.add_argument("--label-temperature", type=float, default=None, metavar="T",
                    help="--list-weight: the temperature of the label's softmax (default: --list-temperature; a guess, not "
                         "measured -- it defines the target and stays a choice)")
    ap.add_argument("--refit-every", type=int, default=100, metavar="N",
                    help="--list-temperature fit: fit again after every N updates")
    ap.add_argument("--temperature-range", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                    help="--list-temperature fit / --fit-temperature: the range searched (default 0.001 100)")
    ap.add_argument("--fit-temperature", action="store_true",
                    help="--score-maps with --label-temperature: the summary gains list_fit -- the prediction temperature at which "
                         "list_kl over the scored maps is smallest, and over 33 temperatures of the range list_kl and what a draw "
                         "with probability softmax(prediction / T) earns (expected_regret, best_draw, greedy_draw): the figures to "
                         "choose a --lane-temperature by")
    ap.add_argument("--holdout-maps", type=str, nargs="+", default=None, metavar="FILE",
                    help="--fit-maps: recorded files the fit does not train on, scored under the weights (train.score_maps, "
                         "fs_map_score) before the first and after the last update; one 'validate' line each in train_log.jsonl")
    ap.add_argument("--validate-every", type=int, default=0, metavar="N",
                    help="--holdout-maps: also score after every N updates (0: only before and after)")
    ap.add_argument("--score-maps", type=str, nargs="+", default=None, metavar="FILE",
                    help="no updates, no checkpoint: score the checkpoint (--load CKPT, or <log>/latest_ckpt.pth) on these recorded "
                         "files -- regret, chosen rank, Spearman and pair accuracy per primitive as one JSON line; takes "
                         "--images-per-batch and --rank-min-gap; not together with --fit-maps or --tasks")
    from .evaluate import add_appearance_option
    add_appearance_option(ap)   # (drawn from round_seed(seed, r), like the round's exploration)
    return ap


def _file_policy(a):
    """A policy of the run's shape on the device, for the modes that read recorded files only."""
    import inspect

    from . import nets
    from .env import BatchedFlingEnv

    scales = inspect.signature(BatchedFlingEnv.__init__).parameters["scale_factors"].default   # what main's environment has
    dev = f"cuda:{a.device}"
    torch.cuda.set_device(a.device)
    return nets.MaximumValuePolicy(action_primitives=list(a.action_primitives), num_rotations=12,
                                   scale_factors=list(scales), obs_dim=64, pix_grasp_dist=8, pix_drag_dist=8,
                                   pix_place_dist=5, rgb_only=True, depth_only=False,
                                   action_expl_prob=a.action_expl_prob, action_expl_decay=a.action_expl_decay,
                                   value_expl_prob=a.value_expl_prob, value_expl_decay=a.value_expl_decay, device=dev)


def _main_score_maps(a, ap):
    """--score-maps: the checkpoint's weights in a policy of the run's shape, score_maps over the given files, one JSON line."""
    ckpt = a.load or os.path.join(a.log, LATEST)
    if not os.path.exists(ckpt):
        ap.error(f"--score-maps needs a checkpoint: --load CKPT or {os.path.join(a.log, LATEST)}")
    policy = _file_policy(a)
    load_checkpoint(ckpt, policy)
    fit = dict(fit_temperature=True, **_range_kwargs(a)) if a.fit_temperature else {}
    print(json.dumps(score_maps(policy, a.score_maps, images_per_batch=a.images_per_batch, min_gap=a.rank_min_gap,
                                list_temperature=a.list_temperature, label_temperature=a.label_temperature, **fit)))


def _list_kwargs(a):
    """The listwise arguments of fit_maps / run from the parsed flags: none when --list-weight is 0, so the call is the old one."""
    if not a.list_weight > 0.0:
        return {}
    out = dict(list_weight=a.list_weight, list_temperature=0.1 if a.list_temperature is None else a.list_temperature,
               label_temperature=a.label_temperature)
    if a.list_temperature == "fit":
        out.update(refit_every=a.refit_every, **_range_kwargs(a))
    return out


def _range_kwargs(a):
    return {} if a.temperature_range is None else dict(temperature_range=tuple(a.temperature_range))


def _main_fit_maps(a):
    """--fit-maps: a policy of the run's shape on the device, fit_maps over the given files, the summary as one JSON line."""
    policy = _file_policy(a)
    optimizer = make_optimizer(policy, lr=a.lr, weight_decay=a.weight_decay, hip=a.hip_step)
    if a.load:
        load_checkpoint(a.load, policy, optimizer)
    out = fit_maps(policy, optimizer, a.fit_maps, a.log, a.updates, images_per_batch=a.images_per_batch,
                   pixels_per_image=a.pixels_per_image, seed=a.seed, hip_step=a.hip_step, rank_weight=a.rank_weight,
                   rank_temperature=a.rank_temperature, rank_min_gap=a.rank_min_gap, load_latest=a.load is None,
                   map_loss=a.map_loss, per_image=a.per_image, holdout=a.holdout_maps, validate_every=a.validate_every,
                   **_list_kwargs(a))
    print(json.dumps(out))


def main(argv=None):
    """python -m flingbot_amd.train --log DIR --tasks set.npz [--rounds N] [--tasks-per-round M] [reference flags]
    python -m flingbot_amd.train --log DIR --fit-maps probes.npz [more.npz ...] --updates N [--images-per-batch M]
                                 [--rank-weight W --map-loss [--per-image]] [--list-weight W [--list-temperature T]]
                                 [--list-weight W --label-temperature T --list-temperature fit [--refit-every N]]
                                 [--holdout-maps other.npz --validate-every N]
    python -m flingbot_amd.train --log DIR --score-maps other.npz [--load CKPT] [--list-temperature T]
                                 [--fit-temperature --label-temperature T [--temperature-range LO HI]]

    run_sim.py's training run on one GPU: collect with exploration, record, update, checkpoint; resumes from DIR.  With
    --fit-maps: no collection, dense updates on recorded reward maps (fit_maps), with --holdout-maps scored on maps it does not
    train on.  With --score-maps: no updates at all, a checkpoint scored on recorded maps (score_maps)."""
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.seed < 0:
        ap.error("--seed >= 0")
    if min(a.rounds, a.tasks_per_round, a.slots, a.batch_size, a.update_frequency, a.save_ckpt) < 1 or a.batches_per_update < 0:
        ap.error("--rounds, --tasks-per-round, --slots, --batch_size, --update_frequency, --save_ckpt >= 1")
    if not all(0.0 <= p <= 1.0 for p in (a.action_expl_prob, a.value_expl_prob, a.action_expl_decay, a.value_expl_decay)):
        ap.error("exploration probabilities and decays lie in [0, 1]")
    if not (np.isfinite([a.rank_weight, a.rank_temperature, a.rank_min_gap]).all() and a.rank_weight >= 0.0
            and a.rank_temperature > 0.0 and a.rank_min_gap >= 0.0):
        ap.error("--rank-weight >= 0, --rank-temperature > 0, --rank-min-gap >= 0, all finite")
    fitted = a.list_temperature == "fit"
    given = [t for t in (None if fitted else a.list_temperature, a.label_temperature) if t is not None]
    if not (np.isfinite([a.list_weight] + given).all() and a.list_weight >= 0.0 and all(t > 0.0 for t in given)):
        ap.error("--list-weight >= 0, --list-temperature > 0 (or 'fit'), --label-temperature > 0, all finite")
    if a.label_temperature is not None and a.list_temperature is None and not a.list_weight > 0.0 and not a.fit_temperature:
        ap.error("--label-temperature goes with --list-weight, --list-temperature or --fit-temperature")
    if fitted and (a.fit_maps is None or a.score_maps is not None):
        ap.error("--list-temperature fit belongs to --fit-maps (not to --tasks or --score-maps)")
    if fitted and not (a.list_weight > 0.0 and a.label_temperature is not None):
        ap.error("--list-temperature fit needs --list-weight > 0 and --label-temperature (the target must not move with the fit)")
    if a.fit_temperature and a.score_maps is None:
        ap.error("--fit-temperature goes with --score-maps")
    if a.fit_temperature and a.label_temperature is None:
        ap.error("--fit-temperature needs --label-temperature")
    if a.refit_every < 1:
        ap.error("--refit-every >= 1")
    if a.temperature_range is not None and not (fitted or a.fit_temperature):
        ap.error("--temperature-range goes with --list-temperature fit or --fit-temperature")
    if a.temperature_range is not None and not (np.isfinite(a.temperature_range).all() and 0.0 < a.temperature_range[0] < a.temperature_range[1]):
        ap.error("--temperature-range LO HI with 0 < LO < HI, finite")
    if a.score_maps is not None and a.list_weight > 0.0:
        ap.error("--score-maps runs no updates: --list-weight does not apply (give --list-temperature for the listwise figures)")
    if a.lookahead is not None and a.lookahead < 1:
        ap.error("--lookahead takes K >= 1")
    if a.lookahead is not None and a.lookahead > a.slots:
        ap.error(f"--lookahead {a.lookahead} needs at least that many --slots (a lane is a slot)")
    from .evaluate import lane_flags_given, lane_kwargs
    if a.lookahead is None and lane_flags_given(a):
        ap.error("--lanes, --lane-temperature, --lane-separation, --lanes-off-cloth and --sample-first belong to --lookahead K")
    if a.lanes != "sampled" and lane_flags_given(a):
        ap.error("--lane-temperature, --lane-separation, --lanes-off-cloth and --sample-first belong to --lanes sampled")
    if a.lanes == "sampled" and not (a.lane_temperature > 0 and a.lane_separation >= 0):
        ap.error("--lane-temperature > 0 (inf: a uniform draw), --lane-separation >= 0")

    if a.score_maps is not None:
        if a.images_per_batch < 1:
            ap.error("--images-per-batch >= 1")
        return _main_score_maps(a, ap)
    if a.fit_maps is not None:
        if a.validate_every < 0:
            ap.error("--validate-every >= 0")
        if min(a.updates, a.images_per_batch) < 1 or (a.pixels_per_image is not None and a.pixels_per_image < 1):
            ap.error("--updates, --images-per-batch, --pixels-per-image >= 1")
        if a.per_image and not a.map_loss:
            ap.error("--per-image needs --map-loss")
        if a.list_weight > 0.0 and not a.map_loss:
            ap.error("--list-weight with --fit-maps needs --map-loss")
        if a.rank_weight > 0.0 and not a.map_loss and (a.pixels_per_image is None or a.images_per_batch * a.pixels_per_image > 4096):
            ap.error("--rank-weight with --fit-maps needs --pixels-per-image with images x pixels <= 4096")
        return _main_fit_maps(a)

    from . import nets, sim as fsim, taskio
    from .env import BatchedFlingEnv
    from .evaluate import appearance_env_kwargs

    tasks = taskio.TaskLoader(a.tasks, repeat=True).all_tasks()
    dev = f"cuda:{a.device}"
    torch.cuda.set_device(a.device)
    n_slots = min(a.slots, a.tasks_per_round) if a.lookahead is None else max(a.lookahead, min(a.slots, a.tasks_per_round * a.lookahead))
    ctx = fsim.FlingSim(n_envs=max(1, n_slots), device=a.device, solver=0)
    try:
        env = BatchedFlingEnv(ctx, action_primitives=tuple(a.action_primitives), episode_length=a.episode_length, device=dev,
                              record_experience=True, **appearance_env_kwargs(a))
        policy = nets.MaximumValuePolicy(action_primitives=list(a.action_primitives), num_rotations=12,
                                         scale_factors=list(env.scale_factors), obs_dim=64, pix_grasp_dist=8, pix_drag_dist=8,
                                         pix_place_dist=5, rgb_only=True, depth_only=False,
                                         action_expl_prob=a.action_expl_prob, action_expl_decay=a.action_expl_decay,
                                         value_expl_prob=a.value_expl_prob, value_expl_decay=a.value_expl_decay, device=dev)
        optimizer = make_optimizer(policy, lr=a.lr, weight_decay=a.weight_decay, hip=a.hip_step)
        if a.load:
            load_checkpoint(a.load, policy, optimizer)
        out = run(policy, optimizer, env, tasks, a.log, a.rounds, a.tasks_per_round, a.seed, batch_size=a.batch_size,
                  warmup=a.warmup, update_frequency=a.update_frequency, batches_per_update=a.batches_per_update,
                  save_ckpt=a.save_ckpt, load_latest=a.load is None, hip_step=a.hip_step, lookahead=a.lookahead, follow=a.follow,
                  rank_weight=a.rank_weight, rank_temperature=a.rank_temperature, rank_min_gap=a.rank_min_gap, **lane_kwargs(a),
                  **_list_kwargs(a))
    finally:
        ctx.close()
    for row in out["rounds"]:
        print(json.dumps(row))


if __name__ == "__main__":
    from flingbot_amd.train import main as _package_main

    _package_main()
