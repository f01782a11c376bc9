"""Importance metrics and channel selection: public interface of the reference's src/pruning/importance.py.

``get_prune_channels`` computes the importances of ALL groups in one HIP launch (device.group_importances), reads them
to the host once, and runs the reference's selection on them (``select_prune_channels``): the cheapest channels under
``n_prune_channels`` / ``perc_prune_channels_per_iter``, trimmed to the importance cap, d_inner counts rounded down to
multiples of 8.
"""
import torch


def calc_importance(importances, importance_metric):
    """Evaluate ``importance_metric`` over the dict ``importances``: names, numbers, + - / ** * (in that order of
    splitting, left to right within an operator, as the reference parses it)."""
    if "+" in importance_metric:
        return sum(calc_importance(importances, part) for part in importance_metric.split("+"))
    for op in ("-", "/"):
        if op in importance_metric:
            first, *rest = importance_metric.split(op)
            value = calc_importance(importances, first)
            for part in rest:
                other = calc_importance(importances, part)
                value = value - other if op == "-" else value / other
            return value
    if "**" in importance_metric:
        parts = importance_metric.split("**")
        if len(parts) != 2:
            raise ValueError(f"** takes two operands, got {parts}")
        return calc_importance(importances, parts[0]) ** calc_importance(importances, parts[1])
    if "*" in importance_metric:
        first, *rest = importance_metric.split("*")
        value = calc_importance(importances, first)
        for part in rest:
            value = value * calc_importance(importances, part)
        return value
    try:
        return float(importance_metric)
    except ValueError:
        return importances[importance_metric]


def select_prune_channels(prune_groups, group_importances, importance_metric, n_prune_channels,
                          perc_prune_channels_per_iter, min_channels_per_group, max_prune_importance_per_iter=None,
                          calibrator_container=None, min_prune_channels=4):
    """The selection of get_prune_channels on importance dicts already in hand (one per group, in order)."""
    if n_prune_channels is None:
        n_prune_channels = max(4, int(sum(g.n_channels for g in prune_groups) * perc_prune_channels_per_iter))
    prunable, prunable_params, minima = [], 0, {}
    for group, raw in zip(prune_groups, group_importances):
        scores = calc_importance(raw, importance_metric)
        if calibrator_container:
            scores = calibrator_container.scale(scores, group)
        minima[group.name] = scores.min()
        n_parameters = raw["n_parameters"]
        cap = min(n_prune_channels, group.n_channels - min_channels_per_group)
        if cap < 1:
            continue
        # merge this group's cheapest channels into the list (kept sorted by importance; at most `cap` of them, and once
        # the list is that long only channels cheaper than an entry at or after the last insertion point get in)
        start = 0
        order = torch.sort(scores, descending=False)
        for j, (value, index) in enumerate(zip(order.values, order.indices)):
            if j >= cap:
                break
            entry = {"group": group, "index": index, "importance": value, "n_parameters": n_parameters}
            if len(prunable) < cap:
                prunable.append(entry)
                prunable_params += n_parameters
                continue
            for k in range(start, len(prunable)):
                if prunable[k]["importance"] > value:
                    prunable.insert(k, entry)
                    prunable_params += n_parameters
                    break
                start += 1

    slack = 8 * 3              # room for the d_inner channels dropped by the multiple-of-8 rule below
    while len(prunable) > n_prune_channels + slack and len(prunable) > min_prune_channels + slack:
        prunable_params -= prunable.pop()["n_parameters"]

    if max_prune_importance_per_iter is not None:
        total = sum(e["importance"] for e in prunable)
        while total > max_prune_importance_per_iter and len(prunable) > min_prune_channels + slack:
            gone = prunable.pop()
            total -= gone["importance"]
            prunable_params -= gone["n_parameters"]

    # a d_inner group loses a multiple of 8 channels: drop its most important picks until it does
    counts = {}
    for e in prunable:
        if e["group"].name.startswith("d_inner"):
            counts[e["group"].name] = counts.get(e["group"].name, 0) + 1
    for name in counts:
        if counts[name] % 8 == 0:
            continue
        for i in reversed(range(len(prunable))):
            if prunable[i]["group"].name == name:
                prunable_params -= prunable.pop(i)["n_parameters"]
                counts[name] -= 1
                if counts[name] % 8 == 0:
                    break

    # back to the channel budget and the importance cap, passing over d_inner picks
    total = sum(e["importance"] for e in prunable)
    skips = 0
    while ((len(prunable) > n_prune_channels
            or (max_prune_importance_per_iter is not None and total > max_prune_importance_per_iter))
           and skips < len(prunable) - 1 and len(prunable) > min_prune_channels):
        if "d_inner" in prunable[-1 - skips]["group"].name:
            skips += 1
            continue
        gone = prunable.pop(-1 - skips)
        total -= gone["importance"]
        prunable_params -= gone["n_parameters"]
    return prunable, prunable_params, minima


def get_prune_channels(prune_groups, importance_metric, n_prune_channels, perc_prune_channels_per_iter,
                       min_channels_per_group, max_prune_importance_per_iter=None, calibrator_container=None,
                       min_prune_channels=4):
    """(prunable, prunable_params, importance_min_dict) as the reference returns them: ``prunable`` a list of
    {"group", "index", "importance", "n_parameters"} sorted by importance.  All groups' importances come from one HIP
    launch; ``calibrator_container`` is duck-typed (only ``.scale(importances, group)`` is called)."""
    from . import device
    imps = device.group_importances(prune_groups, to_host=True)
    return select_prune_channels(prune_groups, imps, importance_metric, n_prune_channels, perc_prune_channels_per_iter,
                                 min_channels_per_group, max_prune_importance_per_iter, calibrator_container,
                                 min_prune_channels)
