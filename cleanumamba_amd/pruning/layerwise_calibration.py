"""Layer-wise pruning calibration: public interface of the reference's src/pruning/layerwise_calibration.py.

    cal = calibrator(ema_factor=0.5)
    cal.gather(model, groups, loss_fn, "taylor_squared_individual", batches, batch_size, loss_samples, seed)
    chosen, n_params, minima = get_prune_channels(groups, metric, None, 0.005, 8, calibrator_container=cal)

``get_calibration`` runs a baseline forward + backward over the calibration batches (its gradients give the
importances), then, per group and prune percentage, prunes the group's cheapest channels in a trial and measures the
loss change over the same batches.  The reference does each trial on a ``copy.deepcopy`` of the model that it prunes
physically.  Here, for every group but ``d_model``, the trial zeroes in place exactly the elements the prune would
remove (``device.TrialMask``, one HIP launch), runs the forward on the model itself (its packed operands and buffers,
no copy and no new pack plan) and writes the saved values back bit-exact.  That is the same function as the pruned
model's (DESIGN 7c lists the argument per group).  ``d_model`` is not: the LayerNorms normalise over the d_model
channels, so that group is pruned physically on a scratch model built from the state dict.

Data.  This project has no dataset loader: ``root`` is a sequence of ``(clean, noisy)`` batches, or a zero-argument
callable returning a fresh iterable of them (called once per pass, with numpy and torch seeded by ``random_seed`` as
the reference reseeds numpy before each pass).  Every pass reads the same batches; a pass stops after the batch that
brings it to ``loss_samples`` clips, or at the end of the data.  Two reference quirks are deliberately not copied:
its ``run_forward`` tests the break after a batch (``floor(n / bs) + 2`` batches), and its baseline call omits
``root`` (it reads the default dataset path).  A string path raises ``NotImplementedError``.
"""
import os

import numpy as np
import torch
import torch.nn as nn

from . import device
from .importance import select_prune_channels
from .pruninggroup import CleanUMambaPrunableChannels

DEFAULT_SCALE = 36          # reference: calibrator.scale of a group it has no scale for


def normalize_scales(scales):
    """Divide every scale by the largest, in place; returns (scales, largest)."""
    max_scale = max(scales.values())
    for key in scales:
        scales[key] /= max_scale
    return scales, max_scale


class calibrator:  # noqa: N801 - the reference's name
    """Per-group importance scales gathered by layer-wise pruning, mixed by an EMA and floored at ``min_scale``;
    ``get_prune_channels(..., calibrator_container=cal)`` multiplies each group's importances by its scale."""

    def __init__(self, ema_factor=1, min_scale=0.0000001):
        self.scales = {}
        self.ema_factor = ema_factor
        self.min_scale = min_scale

    def gather(self, model, prune_groups, loss_fn, importance_metric, root, batch_size, loss_samples, random_seed):
        """One-point calibration on the metric ``n_parameters*<importance_metric>``; zeroes the model's gradients at the
        end (the reference expects them zero before).  A flat-managed model (TrainStep / FlatAdam) keeps its
        parameters bitwise, its Adam moments, step count and loss scale, and its captured train-step graph."""
        scales, offsets, results = get_calibration(model, prune_groups, loss_fn, f"n_parameters*{importance_metric}",
                                                   root, False, batch_size, loss_samples, random_seed)
        for group, scale in scales.items():
            if group in self.scales:
                self.scales[group] = max(self.scales[group] * (1 - self.ema_factor) + scale * self.ema_factor,
                                         self.min_scale)
            else:
                self.scales[group] = max(scales[group], self.min_scale)
        _zero_grads(model)

    def scale(self, importances, group):
        return importances * self.scales.get(group.name, DEFAULT_SCALE)

    def log(self, log_file):
        """Write the scales, normalised by the largest, into ``log_file``.  As in the reference this normalises
        ``self.scales`` in place, which changes later EMA mixing and the scale of absolute importance caps."""
        normalized_scales, max_scale = normalize_scales(self.scales)
        log_file["Prune/calibration_scales/max_scale"] = max_scale
        for group, scale in normalized_scales.items():
            log_file[f"Prune/calibration_scales/{group}"] = scale
        return log_file


def scales_from_results(layer_wise_results, two_point=False):
    """(scales, offsets) from calibrate_prune_groups' rows, as the reference's get_calibration computes them: one point
    scale = loss_change / total_importance; two points (~10 % and ~40 %) fit a line through both."""
    low_point = layer_wise_results[0] if layer_wise_results else None
    scales, offsets = {}, {}
    for r in layer_wise_results:
        if two_point:
            if r["prune_percentage"] < 0.15:
                low_point = r
                continue
            if r["prune_percentage"] < 0.35 or r["prune_percentage"] > 0.45:
                continue
            dx = r["total_importance"] - low_point["total_importance"]
            dy = r["loss_change"] - low_point["loss_change"]
            offsets[r["group"]] = low_point["total_importance"] - low_point["loss_change"] * dx / dy
            scales[r["group"]] = r["loss_change"] / (r["total_importance"] - offsets[r["group"]])
        else:
            offsets[r["group"]] = 0
            scales[r["group"]] = r["loss_change"] / r["total_importance"]
    return scales, offsets


def get_calibration(model, prune_groups, loss_fn, importance_metric, root, two_point=False, batch_size=2,
                    loss_samples=16, random_seed=42):
    """(scales, offsets, layer_wise_results): trial prunes of 20 % of every group (``two_point``: 10 % and 40 %)."""
    prune_group_percentages = [0.1, 0.4] if two_point else [0.2]
    results = calibrate_prune_groups(model, prune_groups, prune_group_percentages, loss_fn, importance_metric, root,
                                     loss_samples, random_seed, batch_size)
    scales, offsets = scales_from_results(results, two_point)
    return scales, offsets, results


def calibrate_prune_groups(model, prune_groups, prune_group_percentages, loss_fn, importance_metric, root,
                           loss_samples=16, random_seed=42, batch_size=2, physical=False, timings=None):
    """One row per (group, percentage) with a non-empty selection: group, prune_percentage, prune_parameters,
    prune_groups (channels), mean_importance, total_importance, loss_change, as the reference's; and index (the
    channels the trial pruned, which the reference does not return).  The baseline's gradients stay in the
    model (the reference leaves them for its caller).  ``physical``: every trial on a pruned scratch model, as the
    reference does it (for comparisons and the benchmark).  ``timings``: a dict that receives host wall times."""
    models = _models_of(model, prune_groups)
    _check_state(models, model)
    clock = _Clock(timings)
    np_state, torch_state = np.random.get_state(), torch.random.get_rng_state()
    adam = _flat_adam(model)
    slot = adam.grads_scale_slot if adam is not None else None
    try:
        if _flat_of_model(model) is not None:
            _zero_grads(model)          # a TrainStep leaves its last step's gradients in the flat buffer
        # ---- baseline: forward + backward over every batch; gradients accumulate
        loss_sum, n = _run_pass(model, loss_fn, root, loss_samples, random_seed, backward=True, adam=adam)
        clock.lap("baseline")
        rows, trials = [], []
        if prune_groups:
            imps = device.group_importances(prune_groups, to_host=True)
            for i, (group, imp) in enumerate(zip(prune_groups, imps)):
                for pct in prune_group_percentages:
                    chosen, params_pruned, _ = select_prune_channels([group], [imp], importance_metric, None, pct, 8)
                    importances = [p["importance"].item() for p in chosen]
                    if not importances:
                        continue
                    idxs = [int(p["index"]) for p in chosen]
                    total = sum(importances)
                    rows.append({"group": group.name,
                                 "prune_percentage": len(idxs) / group.n_channels,
                                 "prune_parameters": params_pruned,
                                 "prune_groups": len(importances),
                                 "mean_importance": total / len(importances),
                                 "total_importance": total,
                                 "loss_change": None,
                                 "index": idxs})
                    trials.append((i, group, idxs))
            clock.lap("select")
        trial_sums = []
        if trials:
            _drop_stream_caches(models)
            for i, group, idxs in trials:
                if physical or _is_d_model(group):
                    trial_sums.append(_physical_trial(model, prune_groups, i, idxs, loss_fn, root, loss_samples,
                                                      random_seed))
                    clock.lap("physical_trials")
                    continue
                mask = device.TrialMask(group, idxs)
                mask.mask()
                clock.lap("mask")
                try:
                    trial_sums.append(_run_pass(model, loss_fn, root, loss_samples, random_seed, backward=False))
                    clock.lap("masked_trials")
                finally:
                    mask.restore()
                    clock.lap("mask")
            _drop_stream_caches(models)
        # ---- one host read for the baseline and every trial
        sums = torch.stack([loss_sum] + [s for s, _ in trial_sums]).cpu().tolist()
        baseline = sums[0] / n
        for row, s, (_, cnt) in zip(rows, sums[1:], trial_sums):
            row["loss_change"] = s / cnt - baseline
        clock.lap("read")
        if timings is not None:
            timings["baseline_loss"] = baseline
        return rows
    finally:
        if adam is not None:
            adam.grads_scale_slot = slot
        np.random.set_state(np_state)
        torch.random.set_rng_state(torch_state)


def remove_forward_hooks(model):
    """Drop every forward (pre-)hook of ``model``'s modules; returns the model (reference helper)."""
    from collections import OrderedDict
    for module in model.modules():
        module._forward_pre_hooks = OrderedDict()
        module._forward_hooks = OrderedDict()
    return model


# ------------------------------------------------------------------------------------------------------------- helpers
class _Clock:
    def __init__(self, timings):
        self.timings = timings
        if timings is not None:
            import time
            sync = torch.cuda.synchronize if torch.cuda.is_available() else (lambda: None)
            self._now = lambda: (sync(), time.perf_counter())[1]
            self.t = self._now()

    def lap(self, key):
        if self.timings is None:
            return
        t = self._now()
        self.timings[key] = self.timings.get(key, 0.0) + (t - self.t)
        self.t = t


def _batches(root, random_seed):
    if isinstance(root, (str, bytes, os.PathLike)):
        raise NotImplementedError("calibration reads no dataset from a path: pass a sequence of (clean, noisy) batches "
                                  "or a zero-argument callable that returns an iterable of them")
    if callable(root):
        np.random.seed(random_seed)
        torch.manual_seed(random_seed)
        return root()
    if root is None:
        raise ValueError("calibration needs data: a sequence of (clean, noisy) batches or a callable returning one")
    return root


def _run_pass(model, loss_fn, root, loss_samples, random_seed, backward, adam=None):
    """(device f64 sum of the per-batch losses, number of batches).  Nothing is read to the host."""
    dev = _device_of(model)
    total = torch.zeros((), dtype=torch.float64, device=dev)
    n, clips = 0, 0
    for clean, noisy in _batches(root, random_seed):
        clean, noisy = clean.to(dev), noisy.to(dev)
        if backward:
            loss, _ = loss_fn(model, (clean, noisy))
            (adam.scale_loss(loss) if adam is not None else loss).backward()
        else:
            with torch.no_grad():
                loss, _ = loss_fn(model, (clean, noisy))
        total = total + loss.detach().double()
        n += 1
        clips += clean.shape[0]
        if clips >= loss_samples:
            break
    if n == 0:
        raise ValueError("calibration: the data yielded no batch")
    return total, n


def _device_of(model):
    return next(model.parameters()).device


def _is_d_model(group):
    return group.name == "d_model"


def _models_of(model, prune_groups):
    out = [model]
    for g in prune_groups:
        m = getattr(g, "model", None)
        if m is not None and all(m is not x for x in out):
            out.append(m)
    return out


def _flat_of_model(model):
    from ..training.flat_optim import sink_of
    for p in model.parameters():
        return sink_of(p)
    return None


def _flat_adam(model):
    """The FlatAdam of a flat-managed model that scales its loss (its importances divide by that scale), else None."""
    flat = _flat_of_model(model)
    adam = flat.optimizer() if flat is not None and getattr(flat, "optimizer", None) is not None else None
    return adam if adam is not None and adam.loss_scaling else None


def _check_state(models, model):
    """Refuse, as prune() does, where a trial would run on state that does not follow the weights."""
    device.refuse_live_streams(models, "calibration", "calibrating")
    flat = _flat_of_model(model)
    if flat is not None:
        buckets = flat.buckets() if getattr(flat, "buckets", None) is not None else None
        if buckets is not None and buckets.exchanging:
            raise NotImplementedError("calibration under a gradient exchange (several ranks) is not supported: every "
                                      "rank would have to measure the same trials")
        flat.require_intact()


def _drop_stream_caches(models):
    """Caches the version counters do not reach: the hop plan / graph and the stream pools' weight blobs (no stream is
    live: checked first).  Pack plans and -exp(A_log) follow the counters TrialMask bumps."""
    for m in models:
        if getattr(m, "stream", None) is not None:
            m.stream.drop_caches(m)


def _zero_grads(model):
    flat = _flat_of_model(model)
    if flat is not None:
        flat.zero_grad()            # lazily: the views stay attached; settle() reads zeros
    else:
        model.zero_grad()


def _network_config(model):
    """Constructor arguments of a CleanUMamba from its modules (the shapes come from the state dict afterwards)."""
    acts = {nn.SiLU: "SiLU", nn.ReLU: "ReLU", nn.GELU: "GELU", nn.Sigmoid: "Sigmoid"}
    enc = model.encoder
    return dict(channels_input=model.channels_input, channels_output=model.channels_output,
                channels_H=model.channels_H, max_H=model.max_H, encoder_n_layers=len(enc),
                kernel_size=model.kernel_size, stride=model.stride,
                encoder_groups=[e[0].groups for e in enc], bypass_channels=[e[3].bypass_channels for e in enc],
                glu_activation=acts[type(enc[0][3].activation)], tsfm_n_layers=len(model.tsfm_Mamba_layers),
                tsfm_n_head=model.tsfm_n_head, tsfm_d_model=model.tsfm_d_model, tsfm_d_inner=model.tsfm_d_inner,
                norm_epsilon=model.norm_f.eps, normalize_input=model.normalize_input)


def scratch_copy(model):
    """A stand-alone copy of ``model`` (same class, weights, mode and path switches) built from its state dict: the
    reference's ``remove_forward_hooks(copy.deepcopy(model))`` without the flat buffers, caches and hooks."""
    dev = _device_of(model)
    copy = type(model)(**_network_config(model), device=dev)
    copy.load_pruned_state_dict({k: v.detach() for k, v in model.state_dict().items()})
    for key in ("use_fused_convs", "use_stack_backward", "use_fused_stream", "use_hop_graph", "use_hop_kernel"):
        if key in model.__dict__:
            setattr(copy, key, model.__dict__[key])
    return copy.train(model.training)


def _physical_trial(model, prune_groups, i, idxs, loss_fn, root, loss_samples, random_seed):
    group = prune_groups[i]
    scratch = scratch_copy(model)
    groups = CleanUMambaPrunableChannels(scratch)
    twin = [g for g in groups if g.name == group.name]
    if len(twin) != 1 or twin[0].n_channels != group.n_channels:
        raise ValueError(f"calibration: group {group.name} is not a group of CleanUMambaPrunableChannels(model)")
    device.prune(groups, {twin[0]: idxs})
    try:
        return _run_pass(scratch, loss_fn, root, loss_samples, random_seed, backward=False)
    finally:
        del scratch, groups
