"""Flat parameter / gradient storage and the clip + Adam (+ loss scaling) step on it.

Optimizer section of the reference's hot loop (src/training/train.py:145-160, 303-310):
``scaler.unscale_`` -> ``clip_grad_norm_(10)`` -> ``scaler.step(Adam)`` -> ``scaler.update``.  There it runs over
103 separate tensors; here every parameter is a view of ONE flat fp32 buffer and every ``p.grad`` a view of a
second one, so that

  * the gradient exchange all-reduces contiguous slices (training/train_distributed.py) with no flatten / copy-back,
  * the norm, the clip, the unscale, the inf check, the loss-scale update and Adam are three kernel launches
    (csrc/optim.hip) with nothing returning to the host -- which is also what lets the whole train step be
    captured in a hipGraph (training/train_step.py).

The host only writes the learning rate into the device-side state vector before each step.

The reference's optimizer choice (src/training/train.py:126-154) is covered by the same three launches: ``"adam"`` is
the default FlatAdam (one group, L2 decay), ``"adamw"`` is ``FlatAdam(groups=..., decoupled_weight_decay=True)``, whose
update kernel (cum_optim_adam_groups) reads each group's learning rate and decay from a small device table and finds a
float4's group through the tile / segment tables of ``group_tables`` below.
"""
import ctypes
import math
import weakref

import torch

from .. import hip

# layout of the device-side state vector (csrc/optim.hip)
ST_NORM, ST_MULT, ST_FOUND_INF, ST_SCALE, ST_TRACKER, ST_STEP, ST_BC1, ST_BC2_SQRT, ST_LR, ST_SKIPPED, ST_GRAD_SCALE = range(11)


_SINKS = {}          # parameter data_ptr -> weakref(FlatParams) that owns it


def _forget(ptrs, ref):
    """A FlatParams was collected: drop its entries (unless a newer FlatParams has taken the address over)."""
    for ptr in ptrs:
        if _SINKS.get(ptr) is ref:
            del _SINKS[ptr]


def sink_of(param):
    """The FlatParams whose flat buffers hold ``param`` (None if the parameter is not flat-managed)."""
    ref = _SINKS.get(param.data_ptr())
    flat = ref() if ref is not None else None
    if flat is None or flat.by_ptr.get(param.data_ptr()) is None:
        return None
    return flat


class FlatParams:
    """Moves the parameters of ``module`` into one flat fp32 buffer (``p.data`` becomes a view) and gives every
    parameter a gradient view of a second flat buffer.  Parameters are laid out in REVERSE registration order:
    that is the order backward produces gradients in (decoder first), so slices from the front of the gradient
    buffer complete first.  Every parameter starts 16-byte aligned (zero padding in between)."""

    ALIGN = 4      # elements

    def __init__(self, module):
        params = [p for p in module.parameters() if p.requires_grad]
        if not params:
            raise ValueError("no trainable parameters")
        dev = params[0].device
        for p in params:
            if p.dtype != torch.float32 or p.device != dev:
                raise RuntimeError("FlatParams needs fp32 parameters on one device (master weights are fp32, "
                                   "as in the reference's autocast training)")
        self.params = list(reversed(params))
        self.offsets, off = [], 0
        for p in self.params:
            self.offsets.append(off)
            off += (p.numel() + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        self.numel = off
        self.data = torch.zeros(off, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(off, dtype=torch.float32, device=dev)
        self.grad_views = []
        with torch.no_grad():
            for p, o in zip(self.params, self.offsets):
                view = self.data[o:o + p.numel()].view_as(p)
                view.copy_(p.detach())
                p.data = view
                gview = self.grad[o:o + p.numel()].view_as(p)
                if p.grad is not None:
                    gview.copy_(p.grad)
                p.grad = gview
                self.grad_views.append(gview)
        self.index = {id(p): i for i, p in enumerate(self.params)}
        self.by_ptr = {p.data_ptr(): i for i, p in enumerate(self.params)}
        # fresh[i]: nothing has been accumulated into gradient i since zero_grad() -- a producer may then WRITE its
        # result into the view (GradSink below) instead of handing it to autograd's AccumulateGrad (read-read-write)
        self.fresh = [False] * len(self.params)
        # Lazy zeroing (see zero_grad): indices whose gradient memory still holds the PREVIOUS cycle's values
        self.stale = set()
        self.sunk_now, self.sunk_last = set(), None
        ref = weakref.ref(self)
        for i, p in enumerate(self.params):
            p.register_hook(self._pre_accumulate(ref, i))
        ptrs = [p.data_ptr() for p in self.params]
        for ptr in ptrs:
            _SINKS[ptr] = ref
        weakref.finalize(self, _forget, ptrs, ref)

    # weak references set by the FlatAdam whose moments and the GradBuckets whose slices follow this storage (pruning,
    # pruning/device.py, rebuilds them with it)
    optimizer = None
    buckets = None

    def __getstate__(self):
        # (the weak back-references cannot be pickled: a saved model -- torch.save(net) with net.grad_buckets -- drops them)
        state = self.__dict__.copy()
        state.pop("optimizer", None)
        state.pop("buckets", None)
        return state

    def replace_storage(self, data, grad, shapes):
        """Take over new flat buffers that already hold every parameter and gradient in the FlatParams layout (same
        order, 16-byte aligned starts, zero padding) with the new ``shapes`` (pruning, pruning/device.py): every
        ``p.data`` / ``p.grad`` becomes a view of them; the Parameter objects, their hooks and the lazy-zeroing state
        stay."""
        offsets, off = [], 0
        for s in shapes:
            offsets.append(off)
            off += (math.prod(s) + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        if off != data.numel() or off != grad.numel():
            raise ValueError("replace_storage: buffer size does not match the layout")
        ref = weakref.ref(self)
        for p in self.params:
            if _SINKS.get(p.data_ptr()) is ref:
                del _SINKS[p.data_ptr()]
        self.data, self.grad, self.offsets, self.numel = data, grad, offsets, off
        self.grad_views = []
        with torch.no_grad():
            for p, o, s in zip(self.params, offsets, shapes):
                n = math.prod(s)
                p.grad = None
                p.data = data[o:o + n].view(s)
                gview = grad[o:o + n].view(s)
                p.grad = gview
                self.grad_views.append(gview)
        self.by_ptr = {p.data_ptr(): i for i, p in enumerate(self.params)}
        ptrs = [p.data_ptr() for p in self.params]
        for ptr in ptrs:
            _SINKS[ptr] = ref
        weakref.finalize(self, _forget, ptrs, ref)

    def intact(self):
        """False once somebody re-pointed a parameter (``.to()``, pruning, load_pruned_state_dict ...)."""
        base = self.data.data_ptr()
        return all(p.data_ptr() == base + 4 * o for p, o in zip(self.params, self.offsets))

    def require_intact(self):
        """The optimizer, the gradient sinks and the exchange all work on the flat buffers: once a parameter points
        somewhere else (``net.to()`` / ``.half()``, ``load_pruned_state_dict``, pruning, ``p.data = ...``) they would
        silently keep training an orphaned copy.  Raise instead."""
        if not self.intact():
            raise RuntimeError("a parameter was re-allocated after FlatParams took it over (net.to() / .half() / pruning / "
                               "load_pruned_state_dict after the TrainStep was built): its flat view is orphaned and the "
                               "live parameter would silently stop training; build a new TrainStep / GradBuckets")

    def bump_versions(self):
        """The kernels update the flat buffer through raw pointers, which no autograd version counter sees.  Caches
        keyed on ``p._version`` (packed conv weights, the captured streaming hop's weight copies, -exp(A_log)) would
        go stale: count the update on every parameter (6 us for 103 tensors)."""
        torch._C._increment_version(self.params)

    def attach_grads(self):
        """Make every ``p.grad`` the bucket view again (after ``zero_grad(set_to_none=True)`` or a foreign ``.grad``)."""
        for p, g in zip(self.params, self.grad_views):
            if p.grad is not g:
                if p.grad is not None and p.grad.data_ptr() != g.data_ptr():
                    g.copy_(p.grad)
                p.grad = g

    @staticmethod
    def _pre_accumulate(ref, i):
        """Tensor hook of parameter i: autograd is about to ADD a gradient into its view.  If that view was left un-zeroed
        by a lazy zero_grad() it is cleared first (sink-written gradients never come through here: their producers return
        None to autograd)."""
        def hook(grad):
            flat = ref()
            if flat is not None and i in flat.stale:
                flat.stale.discard(i)
                flat.grad_views[i].zero_()
            return grad
        return hook

    # The whole-buffer memset (165 MB for the 41.4 M model, every step) is only needed by gradients that autograd
    # ACCUMULATES into their views.  A gradient that a kernel WRITES through the sink below needs no zero underneath it, and
    # in a TrainStep every gradient is such a write.  zero_grad() therefore clears only the views that were not sink-written
    # in the previous cycle and marks the others stale; a stale view is cleared the moment something else than a sink
    # write is about to touch it (the hook above) or, if nothing touches it at all, in settle() before anybody reads the
    # buffer (optimizer, exchange).  The alignment padding between parameters is written by nobody and stays zero.
    LAZY_ZERO = True
    # set by GradBuckets when a gradient exchange reads whole bucket slices at the end of the backward (before settle()):
    # untouched stale views would be exchanged as they are, so every view is zeroed up front there
    exchange_reads_buffer = False

    def zero_grad(self):
        last = self.sunk_last
        self.sunk_last, self.sunk_now = None, set()
        if self.LAZY_ZERO and last and not self.exchange_reads_buffer:
            self.stale = set(last)
            start = None
            for i in range(len(self.params) + 1):          # contiguous runs of the views that do need zeros
                need = i < len(self.params) and i not in last
                if need and start is None:
                    start = self.offsets[i]
                if not need and start is not None:
                    self.grad[start:(self.offsets[i] if i < len(self.params) else self.numel)].zero_()
                    start = None
        else:
            self.stale = set()
            self.grad.zero_()
        self.attach_grads()
        self.fresh = [True] * len(self.params)

    def settle(self):
        """End of an accumulation cycle, before the flat gradient is read: views still stale (no gradient reached them in
        this cycle) become zeros; what was sink-written in this cycle may stay un-zeroed at the next zero_grad()."""
        for i in sorted(self.stale):
            self.grad_views[i].zero_()
        self.stale = set()
        self.sunk_last = set(self.sunk_now)

    # ---- gradient sink: kernels write parameter gradients straight into the flat buffer
    def slot(self, param):
        """(index, element offset) of ``param`` if its gradient view may be overwritten now, else None."""
        i = self.by_ptr.get(param.data_ptr())
        if not self.armed or i is None or not self.fresh[i] or param.grad is not self.grad_views[i]:
            return None
        return i, self.offsets[i]

    # The sink is taken only inside a backward that its owner started (TrainStep.micro_step arms it): any other
    # backward -- torch.autograd.grad(loss, params), a user's own loss.backward() -- sees plain autograd semantics
    # (gradients returned / accumulated by AccumulateGrad), not None results and silently overwritten .grad views.
    armed = False

    def wrote(self, indices):
        """The gradients of these parameters now sit in their views (they are no longer fresh); tell the exchange."""
        for i in indices:
            self.fresh[i] = False
            self.stale.discard(i)
            self.sunk_now.add(i)
        if self.on_write is not None:
            self.on_write([self.params[i] for i in indices])

    on_write = None

    def slices(self, max_bytes):
        """Contiguous (start, end, [param indices]) ranges of at most ``max_bytes`` (cut at parameter boundaries)."""
        cap = max(1, max_bytes // 4)
        out, start, members = [], 0, []
        for i, (p, o) in enumerate(zip(self.params, self.offsets)):
            end = o + (p.numel() + self.ALIGN - 1) // self.ALIGN * self.ALIGN
            if members and end - start > cap:
                out.append((start, o, members))
                start, members = o, []
            members.append(i)
        out.append((start, self.numel, members))
        return out


def group_tables(offsets, numels, group_ids, tile_elems, align=FlatParams.ALIGN):
    """Membership tables of cum_optim_adam_groups (csrc/optim.hip) for parameters laid out back to back at ``offsets``
    (elements, ascending, each a multiple of ``align`` = 4, each parameter padded to a multiple of 4) with ``numels``
    elements and the group ``group_ids[i]`` each.  A pure function of its arguments (CPU int32 tensors out):

      tile_group[t]  for tile t = float4 [t * T, (t + 1) * T), T = tile_elems / 4: the group if one segment covers the
                     whole tile, else -(s) - 1 with s the first segment that reaches into it
      seg_end[s], seg_group[s]  runs of neighbouring parameters of one group: exclusive end in float4 units, group

    O(tiles + segments) memory; a parameter's padding belongs to the parameter's group."""
    if tile_elems <= 0 or tile_elems % 4 or align != 4:
        raise ValueError("group_tables: the tile must be a positive multiple of 4 elements")
    if not (len(offsets) == len(numels) == len(group_ids)) or not len(offsets):
        raise ValueError("group_tables: offsets, numels and group_ids must have one entry per parameter")
    tile4 = tile_elems // 4
    seg_end, seg_group, at = [], [], 0
    for off, n, k in zip(offsets, numels, group_ids):
        if off != at or n < 0 or k < 0:
            raise ValueError("group_tables: parameters must follow each other without gaps, 4-element aligned")
        at = off + (n + 3) // 4 * 4
        if at == off:
            continue                                     # an empty parameter owns no float4
        if seg_group and seg_group[-1] == k:
            seg_end[-1] = at // 4
        else:
            seg_end.append(at // 4)
            seg_group.append(int(k))
    if not seg_end:
        raise ValueError("group_tables: no elements")
    total4 = seg_end[-1]
    if total4 >= 2 ** 31:
        raise ValueError("group_tables: more than 2^33 elements")
    ends = torch.tensor(seg_end, dtype=torch.int64)
    first4 = torch.arange(0, total4, tile4, dtype=torch.int64)             # first float4 of every tile
    last4 = torch.clamp(first4 + tile4, max=total4) - 1                     # its last one
    s_first = torch.searchsorted(ends, first4, right=True)                  # first segment with end > float4
    s_last = torch.searchsorted(ends, last4, right=True)
    groups = torch.tensor(seg_group, dtype=torch.int64)
    tile_group = torch.where(s_first == s_last, groups[s_first], -s_first - 1)
    return tile_group.to(torch.int32), ends.to(torch.int32), groups.to(torch.int32)


class FlatAdam:
    """Adam with gradient-norm clipping and (optionally) dynamic loss scaling on a FlatParams.

    Arithmetic of ``torch.optim.Adam`` (no amsgrad; weight decay in the L2 form), ``clip_grad_norm_`` and
    ``torch.amp.GradScaler`` (init_scale 65536, growth 2 every 2000 clean steps, backoff 0.5; a step whose
    gradients hold inf / nan is skipped).  ``param_groups`` has one group so that the LR schedulers written
    for torch optimizers (``group["lr"] = ...``) drive it unchanged.

    groups: parameter groups in torch's form, ``[{"params": [...], "weight_decay": ..., "lr": ...}, ...]``; missing keys
      take the constructor's values.  Every parameter of ``flat`` belongs to exactly one group; betas and eps are shared
      (one pair of bias corrections).  ``param_groups`` then has one dict per group, and the update is ONE launch of
      cum_optim_adam_groups whatever their number.  None: one group, cum_optim_adam, as ever.
    decoupled_weight_decay: ``torch.optim.AdamW``'s form, ``p *= 1 - lr * weight_decay`` before the update, instead of
      the L2 term in the gradient.  Membership follows the Parameter objects, so it survives pruning."""

    def __init__(self, flat, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=0.0,
                 loss_scaling=False, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000,
                 groups=None, decoupled_weight_decay=False):
        self.flat = flat
        self.decoupled = bool(decoupled_weight_decay)
        self.grouped = groups is not None or self.decoupled
        if groups is None:
            self.param_groups = [{"params": flat.params, "lr": lr, "betas": tuple(betas), "eps": eps,
                                  "weight_decay": weight_decay}]
        else:
            self.param_groups = self._checked_groups(flat, groups, lr, tuple(betas), eps, weight_decay)
        self.max_grad_norm = float(max_grad_norm or 0.0)
        self.loss_scaling = bool(loss_scaling)
        self.growth, self.backoff, self.growth_interval = growth_factor, backoff_factor, int(growth_interval)
        dev = flat.data.device
        lib = hip.lib()
        if self.grouped and len(self.param_groups) > lib.cum_optim_max_groups():
            raise ValueError(f"FlatAdam: {len(self.param_groups)} parameter groups; the update kernel takes at most "
                             f"{lib.cum_optim_max_groups()}")
        self.exp_avg = torch.zeros_like(flat.data)
        self.exp_avg_sq = torch.zeros_like(flat.data)
        self.state_vec = torch.zeros(lib.cum_optim_state_elems(), dtype=torch.float32, device=dev)
        self.state_vec[ST_SCALE] = init_scale if loss_scaling else 1.0
        self.state_vec[ST_LR] = lr
        self._lr_written = lr
        self._listeners = []
        if self.grouped:
            # {lr, weight_decay, 1 - lr * weight_decay, unused} per group, at a fixed address: a captured step reads
            # the values of the replay (write_lr), as it reads state_vec[ST_LR] with one group
            self.group_hyper = torch.zeros(len(self.param_groups), 4, dtype=torch.float32, device=dev)
            self._hyper_written = None
        self.layout_changed()
        flat.optimizer = weakref.ref(self)

    @staticmethod
    def _checked_groups(flat, groups, lr, betas, eps, weight_decay):
        """torch-style group dicts with the constructor's defaults filled in; every parameter of ``flat`` exactly once."""
        def name(p):
            i = flat.index.get(id(p))
            return f"parameter {tuple(p.shape)}" + (f" (flat index {i})" if i is not None else "")
        out, seen = [], set()
        if not groups:
            raise ValueError("FlatAdam: groups is empty")
        for gi, g in enumerate(groups):
            if not isinstance(g, dict) or "params" not in g:
                raise ValueError(f"FlatAdam: group {gi} is not a dict with a 'params' list")
            unknown = set(g) - {"params", "lr", "betas", "eps", "weight_decay"}
            if unknown:
                raise ValueError(f"FlatAdam: group {gi}: unsupported keys {sorted(unknown)}")
            if tuple(g.get("betas", betas)) != betas or g.get("eps", eps) != eps:
                raise ValueError(f"FlatAdam: group {gi}: betas and eps are shared by all groups (one pair of bias "
                                 "corrections per step)")
            params = list(g["params"])
            for p in params:
                if id(p) not in flat.index:
                    raise ValueError(f"FlatAdam: group {gi}: {name(p)} is not a parameter of the FlatParams")
                if id(p) in seen:
                    raise ValueError(f"FlatAdam: group {gi}: {name(p)} is in more than one group")
                seen.add(id(p))
            out.append({"params": params, "lr": g.get("lr", lr), "betas": betas, "eps": eps,
                        "weight_decay": g.get("weight_decay", weight_decay)})
        for p in flat.params:
            if id(p) not in seen:
                raise ValueError(f"FlatAdam: {name(p)} is in no group")
        return out

    def layout_changed(self, exp_avg=None, exp_avg_sq=None):
        """Everything that follows the flat layout: the partial-sum buffer of the norm and, with groups, the membership
        tables of the update kernel.  Pruning (pruning/device.py) passes the moment buffers of the new layout."""
        f, lib = self.flat, hip.lib()
        dev = f.data.device
        if exp_avg is not None:
            self.exp_avg, self.exp_avg_sq = exp_avg, exp_avg_sq
        self.nparts = lib.cum_optim_sumsq_parts(f.numel)
        self.partials = torch.zeros(self.nparts, dtype=torch.float32, device=dev)
        if self.grouped:
            self.tile_group, self.seg_end, self.seg_group = (t.to(dev) for t in self.membership())

    def membership(self):
        """group_tables of the current layout (CPU tensors)."""
        gid = {id(p): k for k, g in enumerate(self.param_groups) for p in g["params"]}
        f = self.flat
        return group_tables(f.offsets, [p.numel() for p in f.params], [gid[id(p)] for p in f.params],
                            hip.lib().cum_optim_group_tile_elems())

    # ---- loss scaling (device scalars: no host sync)
    def scale_loss(self, loss):
        self.grads_scale_slot = ST_SCALE
        return loss * self.state_vec[ST_SCALE] if self.loss_scaling else loss

    # Slot of state_vec holding the scale the gradients in the flat buffer carry: the current scale while they are being
    # accumulated (scale_loss), the one the last step used once a step has run (its update may have changed the current
    # one; cum_optim_prepare writes ST_GRAD_SCALE).  Read by the pruning importances (pruning/device.py).
    grads_scale_slot = ST_SCALE

    @property
    def loss_scale(self):
        return self.state_vec[ST_SCALE]

    @property
    def grad_norm(self):
        """Total norm of the (unscaled, unclipped) gradient of the last step -- a device scalar."""
        return self.state_vec[ST_NORM]

    def zero_grad(self, set_to_none=False):
        self.flat.zero_grad()

    def write_lr(self):
        """Push the host-side learning rate to the device (one fill kernel; call outside a captured graph).  With groups:
        every group's lr, weight decay and 1 - lr * weight_decay (formed in double here, rounded once) go to the device
        table -- fill kernels for the columns that changed, one per column while the groups agree; no synchronisation."""
        if not self.grouped:
            lr = float(self.param_groups[0]["lr"])
            self.state_vec[ST_LR:ST_LR + 1].fill_(lr)
            self._lr_written = lr
            return
        rows = [(float(g["lr"]), float(g["weight_decay"]), 1.0 - float(g["lr"]) * float(g["weight_decay"]))
                for g in self.param_groups]
        old = self._hyper_written
        for c in range(3):
            col = [r[c] for r in rows]
            if old is not None and col == [r[c] for r in old]:
                continue
            if all(x == col[0] for x in col):
                self.group_hyper[:, c].fill_(col[0])
            else:
                for k, x in enumerate(col):
                    if old is None or old[k][c] != x:
                        self.group_hyper[k, c:c + 1].fill_(x)
        self._hyper_written = rows
        self._lr_written = rows[0][0]

    def step(self, write_lr=True):
        """unscale + clip + Adam + scale update; three launches on the current stream."""
        g = self.param_groups[0]
        if write_lr:
            self.write_lr()
        lib, f = hip.lib(), self.flat
        f.require_intact()
        f.settle()
        st = hip.stream_ptr()
        with torch.cuda.device(f.data.device):
            hip.check(lib.cum_optim_sumsq(hip.ptr(f.grad), f.numel, hip.ptr(self.partials), st))
            hip.check(lib.cum_optim_prepare(hip.ptr(self.state_vec), hip.ptr(self.partials), self.nparts,
                                            self.max_grad_norm, g["betas"][0], g["betas"][1], int(self.loss_scaling),
                                            self.growth, self.backoff, self.growth_interval, st))
            if self.grouped:
                hip.check(lib.cum_optim_adam_groups(hip.ptr(f.data), hip.ptr(f.grad), hip.ptr(self.exp_avg),
                                                    hip.ptr(self.exp_avg_sq), f.numel, hip.ptr(self.state_vec),
                                                    g["betas"][0], g["betas"][1], g["eps"], int(self.decoupled),
                                                    hip.ptr(self.group_hyper), len(self.param_groups),
                                                    hip.ptr(self.tile_group), hip.ptr(self.seg_end),
                                                    hip.ptr(self.seg_group), self.seg_end.numel(), st))
            else:
                hip.check(lib.cum_optim_adam(hip.ptr(f.data), hip.ptr(f.grad), hip.ptr(self.exp_avg),
                                             hip.ptr(self.exp_avg_sq), f.numel, hip.ptr(self.state_vec), g["betas"][0],
                                             g["betas"][1], g["eps"], g["weight_decay"], st))
        f.bump_versions()
        self.grads_scale_slot = ST_GRAD_SCALE

    # ---- checkpoint format of torch.optim.Adam (src/training/train.py:183-186, 367: optimizer_state_dict)
    def _numbering(self):
        """{id(param): index in the checkpoint}.  One group: registration order, as torch numbers ``net.parameters()``.
        Groups: through the groups in order, as torch numbers the parameters of a list of group dicts."""
        if not self.grouped:
            return {id(p): i for i, p in enumerate(reversed(self.flat.params))}
        return {id(p): i for i, p in enumerate(p for g in self.param_groups for p in g["params"])}

    def state_dict(self):
        f = self.flat
        order = self._numbering()
        step = self.state_vec[ST_STEP].detach().clone()
        state = {}
        for p, o in zip(f.params, f.offsets):
            n = p.numel()
            state[order[id(p)]] = {"step": step.clone(), "exp_avg": self.exp_avg[o:o + n].view_as(p).clone(),
                                   "exp_avg_sq": self.exp_avg_sq[o:o + n].view_as(p).clone()}
        groups = []
        for g in self.param_groups:
            d = dict(g)
            d["params"] = [order[id(p)] for p in g["params"]] if self.grouped else list(range(len(f.params)))
            groups.append(d)
        if self.grouped:
            state = {k: state[k] for k in sorted(state)}
        return {"state": state, "param_groups": groups, "flat_state": self.state_vec.detach().clone(),
                "loss_scaling": bool(self.loss_scaling)}

    def load_state_dict(self, sd):
        """Moments and the step count come from the checkpoint; the loss scale and its growth tracker only when both the
        checkpoint and this optimizer use loss scaling (a bf16 / f32 run saved scale 1.0: loaded into an fp16 run it
        would underflow the gradients for thousands of steps); the learning rate is the scheduler's to write.  The
        checkpoint must have this optimizer's groups (their number and sizes): the parameter numbering depends on them."""
        f = self.flat
        saved_groups = sd["param_groups"]
        if len(saved_groups) != len(self.param_groups):
            raise ValueError(f"FlatAdam.load_state_dict: the checkpoint has {len(saved_groups)} parameter group(s), this "
                             f"optimizer {len(self.param_groups)}")
        if self.grouped:
            b0, e0 = saved_groups[0].get("betas"), saved_groups[0].get("eps")
            for k, (mine, theirs) in enumerate(zip(self.param_groups, saved_groups)):
                if len(theirs.get("params", mine["params"])) != len(mine["params"]):
                    raise ValueError(f"FlatAdam.load_state_dict: group {k} of the checkpoint has "
                                     f"{len(theirs['params'])} parameters, this optimizer's {len(mine['params'])}")
                if (b0 is not None and tuple(theirs.get("betas", b0)) != tuple(b0)) or theirs.get("eps", e0) != e0:
                    raise ValueError("FlatAdam.load_state_dict: betas and eps differ between the checkpoint's groups")
        order = self._numbering()
        step = None
        with torch.no_grad():
            for p, o in zip(f.params, f.offsets):
                ent = sd["state"].get(order[id(p)])
                if ent is None:
                    continue
                n = p.numel()
                self.exp_avg[o:o + n].copy_(ent["exp_avg"].reshape(-1))
                self.exp_avg_sq[o:o + n].copy_(ent["exp_avg_sq"].reshape(-1))
                if step is None:
                    step = float(ent["step"])                     # one host read, not one per parameter
            saved = sd.get("flat_state")
            if saved is not None:
                saved = saved.detach().float().cpu()
                if step is None:
                    step = float(saved[ST_STEP])
                # the checkpoint scaled its loss too: said by its flag (a scale that had backed off to <= 1.0 is still a
                # loss scale and is restored); checkpoints written before the flag existed: inferred from scale > 1
                scaled = sd.get("loss_scaling")
                if scaled is None:
                    scaled = float(saved[ST_SCALE]) > 1.0
                if self.loss_scaling and scaled:
                    self.state_vec[ST_SCALE] = float(saved[ST_SCALE])
                    self.state_vec[ST_TRACKER] = float(saved[ST_TRACKER])
            if step is not None:
                self.state_vec[ST_STEP] = step
        for mine, theirs in zip(self.param_groups, saved_groups):
            for k in ("lr", "weight_decay"):
                if k in theirs:
                    mine[k] = theirs[k]
            for k in ("betas", "eps"):                            # shared: the first group's
                if k in saved_groups[0]:
                    mine[k] = tuple(saved_groups[0][k]) if k == "betas" else saved_groups[0][k]
        t = float(step or 0.0)
        b1, b2 = self.param_groups[0]["betas"]
        if t > 0:
            self.state_vec[ST_BC1] = 1.0 - b1 ** t
            self.state_vec[ST_BC2_SQRT] = (1.0 - b2 ** t) ** 0.5
        self.hyper_changed()

    # ---- a captured train step bakes host-side values in (betas, eps, weight decay, clip norm): tell whoever captured
    def hyper_changed(self):
        for fn in list(self._listeners):
            fn()

    def on_hyper_change(self, fn):
        self._listeners.append(fn)
