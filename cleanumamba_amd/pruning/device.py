"""Device side of channel pruning: importances in one HIP launch (csrc/prune.hip cum_prune_importance) and the prune
itself, which keeps a flat-managed model flat (cum_prune_gather).

Pruning a model whose parameters are views of a FlatParams (TrainStep with the flat optimizer) cannot re-point
``p.data`` at sliced copies: the flat views would be orphaned (FlatParams.require_intact raises on purpose).  Here the
four flat buffers (parameters, gradients, exp_avg, exp_avg_sq) are rebuilt in the new layout by one gather launch and
every ``p.data`` / ``p.grad`` is re-pointed at its view of the new buffers; the Adam step count and the loss-scale state
stay where they are (FlatAdam.state_vec).  Parameters that are not flat-managed are sliced per tensor, as the reference
does (src/pruning/util.py:328-349), together with the moments of a torch.optim.Adam.
"""
import ctypes

import torch
import torch.nn as nn

from .. import hip

IMP_KEYS = ("weight", "grad", "taylor_individual", "taylor_squared_individual", "taylor_group")
_LANES_ON_CHANNELS_MAX = 16      # a channel of at most this many elements is reduced by one lane, not a whole wave


# ---------------------------------------------------------------------------------------------------------- importances
def _flat_of(param):
    from ..training.flat_optim import sink_of
    return sink_of(param)


def _settle_and_scale(params):
    """Settle lazily zeroed gradient views of every FlatParams among ``params`` (a stale view holds the previous cycle's
    values and counts as zero), and return the device loss-scale pointer their gradients carry (None: unscaled)."""
    scales = set()
    seen = set()
    scale_t = None
    for p in params:
        flat = _flat_of(p)
        if flat is None:
            scales.add(None)
            continue
        if id(flat) not in seen:
            seen.add(id(flat))
            flat.settle()
        adam = flat.optimizer() if getattr(flat, "optimizer", None) is not None else None
        if adam is not None and adam.loss_scaling:
            # the scale the gradients carry: the current one while they accumulate, the one the last step used after it
            slot = adam.grads_scale_slot
            scale_t = adam.state_vec[slot:slot + 1]
            scales.add(scale_t.data_ptr())
        else:
            scales.add(None)
    if len(scales) > 1:
        raise ValueError("pruning importances: the parameters carry different loss scales (several optimizers)")
    return scale_t


def _descriptor(pm, n_channels, out_row):
    p = pm.param()
    w = p.data
    g = p.grad
    if not w.is_contiguous() or (g is not None and (not g.is_contiguous() or g.shape != w.shape)):
        raise ValueError(f"pruning importances: {pm} needs a contiguous parameter and gradient")
    rows = w.shape[pm.dim]
    heads = pm.n_heads
    if pm.channel_offset + n_channels * heads + pm._next_start(rows) > rows:
        raise ValueError(f"pruning importances: {pm} has fewer rows than its group's channels")
    d = hip.PruneImpDesc()
    d.w = w.data_ptr()
    d.g = g.data_ptr() if g is not None else None
    d.numel = w.numel()
    rs = w.stride(pm.dim) if w.dim() > 1 else 1
    d.off = pm.channel_offset * rs
    d.ch_stride = heads * rs
    d.head_stride = rs
    if w.dim() == 1:
        n0, s0, n1, s1 = 1, 0, 1, 0
    elif pm.dim == 0:
        n0, s0, n1, s1 = w[0].numel(), 1, 1, 0
    elif w.dim() == 2:
        n0, s0, n1, s1 = w.shape[0], w.stride(0), 1, 0
    else:
        n0, s0, n1, s1 = w.shape[0], w.stride(0), w[0, 0].numel(), 1
    d.n0, d.s0, d.n1, d.s1 = n0, s0, n1, s1
    d.channels, d.heads = n_channels, heads
    d.out = out_row
    d.lanes_on_channels = int(pm.dim != 0 or heads * n0 * n1 <= _LANES_ON_CHANNELS_MAX)
    return d, heads * n0 * n1, g is not None


def _launch(items):
    """items: [(PruningModule, n_channels)] -> (out (rows, 5) f32 on the device, [(first row, n_parameters, has_grad)])."""
    params = [pm.param() for pm, _ in items]
    dev = hip.require_gpu(*[p.data for p in params])
    for p in params:
        if p.grad is not None:
            hip.require_gpu(p.grad)
    scale = _settle_and_scale(params)
    descs = (hip.PruneImpDesc * len(items))()
    meta, row = [], 0
    for i, (pm, n) in enumerate(items):
        d, n_par, has_grad = _descriptor(pm, n, row)
        descs[i] = d
        meta.append((row, n_par, has_grad))
        row += n
    lib = hip.lib()
    wsb = lib.cum_prune_importance_workspace_bytes(descs, len(items))
    ws = torch.empty(max(int(wsb), 1), dtype=torch.uint8, device=dev)
    out = torch.empty(row, 5, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        hip.check(lib.cum_prune_importance(descs, len(items), hip.ptr(scale), hip.ptr(out), row, hip.ptr(ws), int(wsb),
                                           hip.stream_ptr()))
    return out, meta


def _empty_group_dict():
    return {"weight": None, "grad": None, "taylor_individual": None, "taylor_squared_individual": None,
            "taylor_group": None, "act_var": None, "n_parameters": 0, "n_filters": 0}


def _module_dict(out, row, n, n_par, has_grad):
    d = {k: None for k in IMP_KEYS}
    d["act_var"], d["n_parameters"] = None, n_par
    d["weight"] = out[row:row + n, 0]
    if has_grad:
        for j, k in enumerate(IMP_KEYS[1:], start=1):
            d[k] = out[row:row + n, j]
    return d


def _check_finite(names, out, spans):
    """One host read: the name of every group whose sums are not finite (a non-finite gradient: pruning on it would
    remove arbitrary channels)."""
    ok = torch.stack([torch.isfinite(out[a:b]).all() for a, b in spans]).cpu().tolist()
    bad = [nm for nm, good in zip(names, ok) if not good]
    if bad:
        raise FloatingPointError(f"pruning importances: non-finite gradient (or weight) in group(s) {', '.join(bad)}; "
                                 "nothing was selected")


def module_importances(modules):
    """Importance dicts of single PruningModules (their groups give the channel counts), one launch."""
    out, meta = _launch([(pm, pm.group.n_channels) for pm in modules])
    _check_finite([str(pm) for pm in modules], out, [(r, r + pm.group.n_channels) for pm, (r, _, _) in zip(modules, meta)])
    return [_module_dict(out, r, pm.group.n_channels, n_par, hg) for pm, (r, n_par, hg) in zip(modules, meta)]


def group_importances(groups, to_host=False):
    """Importance dicts of ``groups`` (reference PruningGroup.channel_importances), all from ONE launch.  Per metric the
    module values are averaged in the reference's running form ((acc * count + new) / (count + 1), f32).  ``to_host``:
    the dicts hold CPU tensors (one device-to-host copy for all groups)."""
    items = [(pm, g.n_channels) for g in groups for pm in g.modules]
    out, meta = _launch(items)
    spans, k = [], 0
    for g in groups:
        spans.append((meta[k][0], meta[k + len(g.modules) - 1][0] + g.n_channels))
        k += len(g.modules)
    _check_finite([g.name for g in groups], out, spans)
    if to_host:
        out = out.cpu()
    result, k = [], 0
    for g in groups:
        acc = _empty_group_dict()
        counts = dict.fromkeys(IMP_KEYS, 0)
        for pm in g.modules:
            row, n_par, has_grad = meta[k]
            k += 1
            md = _module_dict(out, row, g.n_channels, n_par, has_grad)
            for m in IMP_KEYS:
                if md[m] is None:
                    continue
                acc[m] = md[m].clone() if acc[m] is None else (acc[m] * counts[m] + md[m]) / (counts[m] + 1)
                counts[m] += 1
            acc["n_parameters"] += n_par
            acc["n_filters"] += 1
        result.append(acc)
    return result


# --------------------------------------------------------------------------------------------------------------- prune
def _normalise(selection):
    """{group: [indices]} from a mapping or from get_prune_channels' list of {"group", "index", ...}."""
    from .pruninggroup import _as_index_list
    if isinstance(selection, dict):
        return {g: _as_index_list(v) for g, v in selection.items()}
    out = {}
    for e in selection:
        out.setdefault(e["group"], []).extend(_as_index_list([e["index"]]))
    return out


def prune(prune_groups, prune_channels, optimizer=None):
    """Prune the selection of get_prune_channels (``prune_channels``: its list, or {group: indices}) from
    ``prune_groups`` in one pass: one compaction of the flat buffers for all groups.  Equivalent to the reference's loop
    ``for group in prune_groups: group.prune([indices of group], optimizer)``."""
    sel = _normalise(prune_channels)
    known = {id(g) for g in prune_groups}
    for g in sel:
        if id(g) not in known:
            raise ValueError(f"prune: group {g.name} is not one of prune_groups")
    prune_groups_dict({g: sel.get(g, []) for g in prune_groups}, optimizer)


def prune_groups_dict(selection, optimizer=None):
    # ---- validate everything before mutating anything
    work, models = [], []
    for g, idxs in selection.items():
        if not idxs:
            continue
        if len(set(idxs)) != len(idxs):
            raise ValueError(f"prune: group {g.name}: duplicate channel indices")
        bad = [i for i in idxs if i < 0 or i >= g.n_channels]
        if bad:
            raise IndexError(f"prune: group {g.name}: channel(s) {bad[:4]} outside [0, {g.n_channels})")
        if g.n_channels - len(idxs) < g.min_channels:
            raise ValueError(f"prune: group {g.name} would keep {g.n_channels - len(idxs)} channel(s), below its minimum "
                             f"of {g.min_channels}")
        work.append((g, sorted(idxs)))
        if g.model is not None and all(m is not g.model for m in models):
            models.append(g.model)
    if not work:
        return
    removals = []
    for g, idxs in work:
        for pm in g.modules:
            removals.append((pm, pm.removed_rows(idxs, g.n_channels)))
    prune_modules(removals, optimizer, models=models, _after=lambda: _update_groups(work))


def _update_groups(work):
    for g, idxs in work:
        for pm in g.modules:
            if pm.next_module_to_offset is not None:
                pm.next_module_to_offset.change_offset(-len(idxs) * pm.n_heads)
        g.n_channels -= len(idxs)
        if "d_model" in g.name and g.main_module is not None:
            for block in g.main_module:
                block.d_model = g.n_channels          # (reference: the Blocks carry d_model too)


def _plan(removals):
    """{id(param): [param, {dim: set(removed rows)}]} for every weight and bias the removals touch."""
    plan = {}

    def add(param, dim, rows):
        ent = plan.setdefault(id(param), [param, {}])
        ent[1].setdefault(dim, set()).update(rows)

    for pm, rows in removals:
        add(pm.param(), pm.dim, rows)
        b = pm.bias()
        if b is not None:
            add(b, 0, rows)
    keeps = {}
    for pid, (param, dims) in plan.items():
        kd = {}
        for dim, rows in dims.items():
            n = param.shape[dim]
            if any(r < 0 or r >= n for r in rows):
                raise IndexError(f"prune: rows outside a parameter of shape {tuple(param.shape)} along dim {dim}")
            keep = [i for i in range(n) if i not in rows]
            if not keep:
                raise ValueError(f"prune: a parameter of shape {tuple(param.shape)} would lose every row along dim {dim}")
            if len(keep) < n:
                kd[dim] = keep
        if kd:
            keeps[pid] = (param, kd)
    return keeps


def _modules_touched(removals):
    mods = []
    for pm, _ in removals:
        m = pm.module
        if not any(m is x for x in mods):
            mods.append(m)
    return mods


def prune_modules(removals, optimizer=None, model=None, models=None, _after=None):
    """Remove ``rows`` along each PruningModule's dim (weights, their biases, gradients and optimizer state), update the
    modules' size attributes and drop every derived cache.  Raises before any change if the request cannot be done."""
    from ..training.flat_optim import FlatAdam
    models = list(models or ([] if model is None else [model]))
    keeps = _plan(removals)
    params = [p for p, _ in keeps.values()]
    flats = []
    for p in params:
        f = _flat_of(p)
        if f is not None and all(f is not x for x in flats):
            flats.append(f)
    if len(flats) > 1:
        raise ValueError("prune: the parameters belong to several FlatParams")
    flat = flats[0] if flats else None
    adam = None
    if flat is not None:
        if any(_flat_of(p) is not flat for p in params):
            raise ValueError("prune: some parameters of the group are flat-managed and some are not")
        buckets = flat.buckets() if getattr(flat, "buckets", None) is not None else None
        if buckets is not None and buckets.exchanging:
            raise NotImplementedError("prune: pruning under a gradient exchange (several ranks) is not supported: every "
                                      "rank would have to select the same channels, which is a later step")
        if optimizer is not None and not (isinstance(optimizer, FlatAdam) and optimizer.flat is flat):
            raise ValueError("prune: the parameters are flat-managed; pass their FlatAdam (TrainStep.optimizer) or None")
        adam = flat.optimizer() if getattr(flat, "optimizer", None) is not None else None
        if not flat.data.is_cuda:
            hip.require_gpu(flat.data)
        if not flat.intact():
            flat.require_intact()
    elif isinstance(optimizer, FlatAdam):
        raise ValueError("prune: a FlatAdam was given but the parameters are not flat-managed by it")
    elif optimizer is not None and not isinstance(optimizer, torch.optim.Optimizer):
        raise TypeError(f"prune: unsupported optimizer {type(optimizer).__name__}")
    refuse_live_streams(models, "prune", "pruning")

    # ---- mutate
    if flat is not None:
        _compact_flat(flat, adam, {id(p): kd for p, kd in keeps.values()})
    else:
        with torch.no_grad():
            for p, kd in keeps.values():
                _slice_tensor_state(p, kd, optimizer)
    for m in _modules_touched(removals):
        _resize_module(m)
    if _after is not None:
        _after()
    _drop_caches(models, _modules_touched(removals), adam)


def refuse_live_streams(models, who, doing):
    """Raise if a model has a live ``feed`` stream or a stream pool with open slots: their state has the current widths
    and weights, which pruning (or a calibration trial) changes."""
    for m in models:
        stream = getattr(m, "stream", None)
        if stream is not None and stream.live:
            raise RuntimeError(f"{who}: the model has a live stream whose state has the old widths; flush() or "
                               f"reset_stream() before {doing}")
        for pool in m.__dict__.get("_stream_pools", ()):
            if pool.live:
                raise RuntimeError(f"{who}: a stream pool of the model has open slots {pool.live} whose state has the old "
                                   f"widths; close() them before {doing}")


def _select(t, kd):
    for dim, keep in sorted(kd.items()):
        t = torch.index_select(t, dim, torch.tensor(keep, dtype=torch.long, device=t.device))
    return t


def _slice_tensor_state(p, kd, optimizer):
    """The reference's prune_parameter_and_grad: index_select of the weight, its gradient and the Adam moments."""
    new = _select(p.data, kd)
    grad = p.grad
    if grad is not None:
        p.grad = None
    p.data = new
    if grad is not None:
        p.grad = _select(grad, kd)
    if optimizer is not None and len(optimizer.state) > 0 and p in optimizer.state:
        st = optimizer.state[p]
        for key in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
            if key in st and torch.is_tensor(st[key]) and st[key].shape != p.shape:
                st[key] = _select(st[key], kd)


def _compact_flat(flat, adam, keeps):
    """One gather launch from the old flat layout to the new one (same parameter order, 16-byte aligned starts, zero
    padding) for parameters, gradients and both moments; then every view is re-pointed."""
    lib = hip.lib()
    dev = flat.data.device
    old_off, old_numel = list(flat.offsets), flat.numel
    new_shapes, keep_ints = [], []
    off = 0
    descs = (hip.PruneGatherDesc * len(flat.params))()
    for i, p in enumerate(flat.params):
        shape = list(p.shape)
        kd = keeps.get(id(p), {})
        for dim, keep in kd.items():
            shape[dim] = len(keep)
        if p.dim() > 3:
            raise ValueError("prune: parameters of more than 3 dimensions")
        d = descs[i]
        d.src, d.dst = old_off[i], off
        nd = max(1, p.dim())
        d.ndim = nd
        old = list(p.shape) or [1]
        new = shape or [1]
        for k in range(3):
            d.old_dims[k] = old[k] if k < nd else 1
            d.new_dims[k] = new[k] if k < nd else 1
            if k in kd:
                d.keep[k] = len(keep_ints)
                keep_ints.extend(kd[k])
            else:
                d.keep[k] = -1
        n_new = 1
        for s in new:
            n_new *= s
        d.n_new = n_new
        new_shapes.append(tuple(shape))
        off += (n_new + flat.ALIGN - 1) // flat.ALIGN * flat.ALIGN
    numel = off
    new_data = torch.zeros(numel, dtype=torch.float32, device=dev)
    new_grad = torch.zeros_like(new_data)
    if adam is not None:                               # no FlatAdam: parameters and gradients only (NULL moments)
        src_m, src_v = adam.exp_avg, adam.exp_avg_sq
        new_m, new_v = torch.zeros_like(new_data), torch.zeros_like(new_data)
    else:
        src_m = src_v = new_m = new_v = None
    keep_arr = (ctypes.c_int32 * max(1, len(keep_ints)))(*keep_ints)
    wsb = lib.cum_prune_gather_workspace_bytes(len(flat.params), len(keep_ints))
    ws = torch.empty(max(int(wsb), 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        hip.check(lib.cum_prune_gather(descs, len(flat.params), keep_arr, len(keep_ints), hip.ptr(flat.data),
                                       hip.ptr(flat.grad), hip.ptr(src_m), hip.ptr(src_v), old_numel, hip.ptr(new_data),
                                       hip.ptr(new_grad), hip.ptr(new_m), hip.ptr(new_v), numel, hip.ptr(ws), int(wsb),
                                       hip.stream_ptr()))
    flat.replace_storage(new_data, new_grad, new_shapes)
    if adam is not None:
        adam.layout_changed(new_m, new_v)              # moments, norm partials, the group membership tables
    buckets = flat.buckets() if getattr(flat, "buckets", None) is not None else None
    if buckets is not None:
        buckets.rebuild()


def _resize_module(m):
    """Size attributes as load_pruned_state_dict sets them (network/CleanUMamba.py)."""
    if isinstance(m, nn.LayerNorm):
        m.normalized_shape = tuple(m.weight.shape)
    elif isinstance(m, nn.ConvTranspose1d):
        m.in_channels, m.out_channels = m.weight.shape[0], m.weight.shape[1]
    elif isinstance(m, nn.Conv1d):
        m.in_channels, m.out_channels = m.weight.shape[1], m.weight.shape[0]
        if m.groups > 1:
            m.groups = m.weight.shape[0]
    elif isinstance(m, nn.Linear):
        m.in_features, m.out_features = m.weight.shape[1], m.weight.shape[0]


def _mixers(models, modules):
    out = []
    for m in list(models) + [x.module if hasattr(x, "get") else x for x in modules]:
        for sub in (m.modules() if isinstance(m, nn.Module) else ()):
            if type(sub).__name__ == "Mamba" and not any(sub is x for x in out):
                out.append(sub)
    return out


def _drop_caches(models, modules, adam):
    """Every cache derived from the old tensors: a new tensor can land at a freed address with version 0, so caches keyed
    on (data_ptr, _version) could otherwise hit."""
    for mx in _mixers(models, modules):
        mx.d_model = mx.in_proj.in_features
        mx.d_inner = mx.x_proj.in_features
        mx.dt_rank = mx.dt_proj.in_features
        mx.d_state = (mx.x_proj.out_features - mx.dt_rank) // 2
        mx.expand = mx.d_inner / mx.d_model
        mx.__dict__.pop("_A_cache", None)                  # -exp(A_log) of inference
    for m in models:
        m.invalidate_packed_weights()                      # pack plans, hop plan / graph
        for pool in list(m.__dict__.get("_stream_pools", ())):
            pool.relayout()                                # (no slot is open: checked before the prune)
    if adam is not None:
        adam.hyper_changed()                               # the TrainStep's captured graph (drop_graph)



# ------------------------------------------------------------------------------------------------- in-place trial masks
class TrialMask:
    """The elements ``group.prune(idxs)`` would remove, zeroed in place and restored bit-exact (csrc/prune.hip
    cum_prune_mask): one descriptor per weight / bias and pruned dimension, the removed rows as a device index list.
    ``mask()`` saves and zeroes, ``restore()`` writes the saved values back; both bump the version counters of the
    touched parameters, so that caches keyed on them (the pack plan's ``packed_version``, ``-exp(A_log)``) refresh.
    The rows are ``PruningModule.removed_rows`` -- offset + h * n_channels + c -- not the rows the importance sums read
    (offset + c * n_heads + h)."""

    def __init__(self, group, idxs):
        from .pruninggroup import _as_index_list
        idxs = sorted(_as_index_list(idxs))
        if len(set(idxs)) != len(idxs) or any(i < 0 or i >= group.n_channels for i in idxs):
            raise IndexError(f"trial mask: group {group.name}: indices must be distinct and in [0, {group.n_channels})")
        rows = {}                               # id(tensor) -> [tensor, parameter, dim, set(rows)]
        for pm in group.modules:
            removed = pm.removed_rows(idxs, group.n_channels)
            for t, dim in ((pm.param(), pm.dim), (pm.bias(), 0)):
                if t is None:
                    continue
                ent = rows.setdefault((id(t), dim), [t, dim, set()])
                ent[2].update(removed)
        self.params = []
        descs, index = [], []
        for t, dim, rs in rows.values():
            rs = sorted(rs)
            w = t.data
            if not w.is_contiguous() or w.dtype != torch.float32:
                raise ValueError(f"trial mask: group {group.name} needs contiguous f32 parameters")
            d = hip.PruneMaskDesc()
            d.w, d.numel = w.data_ptr(), w.numel()
            d.rows = w.shape[dim] if w.dim() else 1
            if w.dim() <= 1:
                d.row_stride, d.n0, d.s0, d.n1, d.s1 = 1, 1, 0, 1, 0
            elif dim == 0:
                d.row_stride, d.n0, d.s0, d.n1, d.s1 = w.stride(0), w[0].numel(), 1, 1, 0
            elif w.dim() == 2:
                d.row_stride, d.n0, d.s0, d.n1, d.s1 = w.stride(1), w.shape[0], w.stride(0), 1, 0
            else:
                d.row_stride, d.n0, d.s0, d.n1, d.s1 = w.stride(1), w.shape[0], w.stride(0), w[0, 0].numel(), 1
            d.first, d.n_rows = len(index), len(rs)
            d.rows_fastest = int(dim != 0)
            index.extend(rs)
            descs.append(d)
            if all(t is not p for p in self.params):
                self.params.append(t)
        self.device = hip.require_gpu(*[t.data for t in self.params])
        self.n_desc = len(descs)
        self.descs = (hip.PruneMaskDesc * self.n_desc)(*descs)
        self.index = (ctypes.c_int32 * max(1, len(index)))(*index)
        self.n_index = len(index)
        lib = hip.lib()
        self.n_save = int(lib.cum_prune_mask_save_elems(self.descs, self.n_desc))
        wsb = int(lib.cum_prune_mask_workspace_bytes(self.n_desc, self.n_index))
        if self.n_save < 0 or wsb < 0:
            raise ValueError(f"trial mask: group {group.name}: bad descriptors")
        self.save = torch.empty(max(1, self.n_save), dtype=torch.float32, device=self.device)
        self.ws = torch.empty(max(1, wsb), dtype=torch.uint8, device=self.device)
        self.masked = False

    def _launch(self, restore):
        lib = hip.lib()
        with torch.cuda.device(self.device):
            hip.check(lib.cum_prune_mask(self.descs, self.n_desc, self.index, self.n_index, hip.ptr(self.save),
                                         self.n_save, int(restore), hip.ptr(self.ws), self.ws.numel(), hip.stream_ptr()))
        torch._C._increment_version(self.params)

    def mask(self):
        if self.masked:
            raise RuntimeError("trial mask: already masked")
        self._launch(False)
        self.masked = True

    def restore(self):
        if not self.masked:
            raise RuntimeError("trial mask: nothing to restore")
        self._launch(True)
        self.masked = False
