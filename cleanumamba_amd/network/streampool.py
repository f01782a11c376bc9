"""Stream pool: streams that join, feed and leave independently, on the one-launch hop (csrc/hop.hip) or, for models
too large for it, on the per-layer fused hop (backend "layers", below).

``feed_batch`` runs S streams in lock-step: they start together, every call gives each the same number of samples, and
they end together.  A pool has a fixed number of SLOTS that share one packed weight blob and one state block
([capacity, state_stride], the layout of hopplan.HopPlan); any subset of the open slots can be fed in a call, with any
number of samples each, and every slot opens and closes on its own.  Per call:

  1. the host schedules the call (``schedule``: a pure function of the slots' pending counts and chunk lengths) -- it
     knows every slot's pending count, nothing is read back from the device;
  2. one staging launch (``cum_stream_pool_stage``) builds each named slot's input row from its history (the samples no
     hop has consumed yet, ``hist`` [capacity, frame_len - 1]) and the new chunk, and writes back what will be left;
  3. slots that reach their FIRST frame in this call (whole windows, no history) run it together on the per-layer fused
     path, in a private streaming context (the model's own stream is not touched), and their state rows are imported
     into the block with a frame count of 1;
  4. one launch of the slotted hop (``cum_stream_hop_slots``) runs every named slot's hops: one workgroup per slot that
     has a hop to run, whatever the capacity, longest first.

``close`` gives each slot what ``flush`` gives a lone stream: zeros up to the slot's own ``valid_length``, its remaining
hops, the decoder drain from its state rows (each at its own ring phase), then the rows are zeroed and the slot id can be
reused.

Backend "layers" (models ``hopplan.pool_backend`` finds only too large for the one-launch hop; network/layerpool.py): the
state block is a slot store -- a slot's row holds what one stream of ``streaming._fused_hop`` carries between hops, laid
out by ``layerpool.segment_table`` -- and step 4 runs in ROUNDS: the slots that have a hop to run, longest first, round r
those with more than r hops, as one dense batch of the fused hop on scratch sized once for the capacity.  One launch of
``cum_stream_slots_move`` gathers the call's running slots' rows into the scratch before round 0; where the cohort
shrinks one launch scatters the rows of the slots that leave, and one behind the last round those of the rest (a
lock-step call gathers once and scatters once).  The running std is kept per slot with the slot's own frame
count: the host computes each round's pair (1 / f, 1 - 1 / f), it rides in the call's table, the device evaluates
``(frame.std + 1e-3) * a + b * std``.  Steps 1 - 3, ``close``, the rated slots and all host bookkeeping are shared; the
first-frame cohort's state is scattered as it is instead of converted.

A slot can work at its own sample rate (``open(rate=...)``): the host keeps, per slot and direction, what a
``StreamResampler`` keeps (``resample.stream_step``), the device the inputs its unfinished outputs still read
(``rs_hist``), and a call that names such a slot converts all of them in ONE launch in front of step 2 and ONE behind
step 4 (``cum_resample_slots``), bit-identical to a ``StreamResampler`` per slot and direction.  A call that names none
runs steps 1 - 4 exactly as before.  Reference semantics: CleanUMamba.feed / flush, src/network/CleanUMamba.py:358-418, as ``feed`` / ``flush`` of
this package implement them.
"""
import collections

import numpy as np
import torch

from .. import hip
from ..util import resample as rs
from . import convstack as cs
from . import hopplan
from . import layerpool
from . import streaming

_REC = 8        # int32 per record of both tables (csrc/hop.hip: kHopItemInts, kStageRecInts)

Schedule = collections.namedtuple("Schedule", "first n_hops offset consumed remainder")


def schedule(pending, started, lengths, frame_len, hop):
    """One call of the pool for the named slots (arrays of one entry per slot):
      pending   samples the slot holds that no hop has consumed (< frame_len);
      started   whether the slot's first frame has run;
      lengths   samples the call brings.
    Returns ``Schedule`` arrays:
      first     the slot runs its first frame in this call (the cohort of the per-layer path);
      n_hops    hops of the slotted launch;
      offset    where the slot's first kernel frame starts in its row (pending ++ chunk): ``hop`` behind a first frame;
      consumed  samples the call consumes = samples it emits (a frame emits ``hop``);
      remainder samples left pending (< frame_len)."""
    pending = np.asarray(pending, dtype=np.int64)
    lengths = np.asarray(lengths, dtype=np.int64)
    started = np.asarray(started, dtype=bool)
    total = pending + lengths
    first = ~started & (total >= frame_len)
    offset = np.where(first, hop, 0)
    avail = total - offset
    n_hops = np.where((started | first) & (avail >= frame_len), (avail - frame_len) // hop + 1, 0)
    consumed = offset + n_hops * hop
    return Schedule(first, n_hops, offset, consumed, total - consumed)


class StreamPool:
    """``capacity`` stream slots of one model; see the module docstring.  Made by ``CleanUMamba.stream_pool``.

    ``backend`` ("kernel", "layers" or None: chosen) is what runs the slots' hops.  "kernel": the one-launch hop, for the
    models it runs (``hopplan.unsupported_reason``: Mamba1 bottleneck, at most ``hopplan.MAX_PARAMS`` parameters, f32) --
    every slot re-reads the weight blob per hop, and a slot's whole state lives in one row of the kernel's state block.
    "layers": the per-layer fused hop on dense batches of slots, for models only too large for the kernel (and for any
    model the kernel runs, when forced); f32 only.  Models neither runs raise ``ValueError``."""

    def __init__(self, model, capacity, model_rate=16000, backend=None):
        self.model_rate = rs._rate(model_rate, "model_rate")
        if backend not in (None, "kernel", "layers"):
            raise ValueError('stream pool: backend is None, "kernel" or "layers"')
        self._forced = backend
        capacity = int(capacity)
        self.model, self.capacity = model, capacity
        backend, plan = self._choose()
        if capacity < 1:
            raise ValueError("stream pool: capacity must be >= 1")
        self._rs, self.rs_hist = rs.PlanTable("cpu"), None    # rated slots' plan pairs (_adopt moves them)
        self._adopt(backend, plan)
        self._open = np.zeros(capacity, dtype=bool)
        self._pend = np.zeros(capacity, dtype=np.int64)       # samples in hist[slot]
        self._frames = np.zeros(capacity, dtype=np.int64)     # frames run (the first one included)
        self._rate = np.zeros(capacity, dtype=np.int64)       # 0: the slot works at the model's rate
        self._rs_par = np.zeros((capacity, 2, 5), dtype=np.int64)   # per direction (in, out): plan id, up, down, H, K
        self._rs_pos = np.zeros((capacity, 2, 3), dtype=np.int64)   # ... received, emitted, where the history starts
        self._rs_parity = np.zeros((capacity, 2), dtype=np.int64)   # ... the row of rs_hist that holds the history
        self._fed = np.zeros(capacity, dtype=np.int64)        # samples a rated slot was fed / has returned, at its rate
        self._given = np.zeros(capacity, dtype=np.int64)

    def _choose(self):
        """(backend, plan) for the model as it is now: the forced backend, else "kernel" wherever a HopPlan can be built and
        "layers" where only size stands against one (``hopplan.pool_backend``).  ValueError for every other model."""
        model = self.model
        if self._forced == "kernel":
            why = hopplan.unsupported_reason(model)
        else:
            try:
                backend, why = hopplan.pool_backend(model), None
            except ValueError as exc:
                why = str(exc)
        if why is not None:
            raise ValueError(f"stream pool: {why}")
        if not cs.supported(model):
            raise ValueError("stream pool: the first frame of a slot runs on the fused per-layer hop, which does not "
                             "cover this model")
        if self._forced == "kernel":
            return "kernel", hopplan.HopPlan(model)
        if self._forced is None and backend == "kernel":
            try:
                return "kernel", hopplan.HopPlan(model)
            except ValueError:                      # e.g. the LDS budget: an obstacle of size
                pass
        if streaming.switch(model, "stream_bf16"):
            raise ValueError("stream pool: the per-layer backend is f32 only (stream_bf16 is set on the model)")
        return "layers", layerpool.LayerPlan(model)

    # ------------------------------------------------------------------ slots
    @property
    def live(self):
        """The open slots, ascending."""
        return [int(s) for s in np.flatnonzero(self._open)]

    def pending(self, slots):
        """Samples each slot holds that no hop has consumed yet: samples at the MODEL's rate, also for a rated slot
        (what its in-conversion still holds back is not counted)."""
        return [int(self._pend[s]) for s in self._slots(slots)]

    def rate(self, slots):
        """The sample rate each slot is fed and answers at (``model_rate`` for an unrated slot)."""
        return [int(self._rate[s]) or self.model_rate for s in self._slots(slots)]

    def open(self, n=1, rate=None):
        """Open ``n`` slots (the lowest free ids); returns their ids.  Each starts a fresh stream.  ``rate``: the sample
        rate the slots are fed and answer at; None or ``model_rate`` gives slots at the model's rate.  Any other must be
        a positive integer both conversions exist for (reduced factors up to 1024, a tile's input span within the
        kernel's LDS): ValueError otherwise, before anything else happens."""
        rate = self._check_rate(rate)
        n = int(n)
        free = np.flatnonzero(~self._open)
        if n < 0 or n > free.size:
            raise ValueError(f"stream pool: {n} slots asked for, {free.size} of {self.capacity} free")
        got = free[:n]
        if rate and n:
            for d, pair in enumerate(((rate, self.model_rate), (self.model_rate, rate))):
                p = rs.plan(*pair)
                self._rs_par[got, d] = (self._rs.add(p), p.up, p.down, p.H, p.K)
            self._rs_size_hist()
        self._rate[got] = rate
        self._open[got] = True
        return [int(s) for s in got]

    def _check_rate(self, rate):
        """0 for a slot at the model's rate, else the rate: both of its plans exist and fit the kernel."""
        if rate is None:
            return 0
        r = rs._rate(rate, "the rate of a pool slot")
        if r == self.model_rate:
            return 0
        for pair in ((r, self.model_rate), (self.model_rate, r)):
            try:
                rs.check_fits(rs.plan(*pair))
            except ValueError as exc:
                raise ValueError(f"stream pool: rate {r}: {exc}") from exc
        return r

    def _rs_size_hist(self):
        """History rows on the pool's device that hold the longest filter of the plan table (none while it is empty)."""
        pitch = hopplan._rup(max([rs.history_bound(p.K) for p in self._rs.plans] + [1]), 4)
        old = self.rs_hist
        if self._rs.plans and (old is None or old.shape[3] < pitch or old.device != self.device):
            # [direction][slot][parity][pitch]: the inputs a slot's unfinished outputs may still read, two rows each
            self.rs_hist = torch.zeros(2, self.capacity, 2, pitch, dtype=torch.float32, device=self.device)
            if old is not None and old.device == self.device:
                self.rs_hist[..., :old.shape[3]] = old

    def reset(self):
        """Close every slot without output; all state is zeroed."""
        self.state.zero_()
        self.hist.zero_()
        if self.rs_hist is not None:
            self.rs_hist.zero_()
        self._open[:] = False
        self._pend[:] = 0
        self._frames[:] = 0
        self._rate[:] = 0
        self._rs_par[:], self._rs_pos[:], self._rs_parity[:] = 0, 0, 0
        self._fed[:], self._given[:] = 0, 0

    def relayout(self):
        """The model's widths changed (pruning) while no slot is open: take the new plan and size the state blocks to it;
        the backend is chosen again unless it was forced.  A model no backend runs any more leaves the pool stale (its
        next call raises)."""
        if self._open.any():
            raise RuntimeError("stream pool: close the slots before the model's widths change")
        try:
            backend, plan = self._choose()
        except ValueError:
            self._stale = True
            return
        self._adopt(backend, plan)
        self.reset()

    def _adopt(self, backend, plan):
        """Take ``plan`` (of the model's current weights) and size zeroed state blocks to it."""
        self.backend, self.plan, self._wv, self._stale = backend, plan, streaming.weights_version(self.model), False
        self.hop, self.frame_len, self.device = plan.hop, plan.frame_len, plan.device
        self.state = torch.zeros(self.capacity, plan.state_stride, dtype=torch.float32, device=self.device)
        self.hist = torch.zeros(self.capacity, hopplan._rup(self.frame_len - 1, 4), dtype=torch.float32, device=self.device)
        # the "layers" backend's dense side: scratch in the fused hop's layout, sized once for the capacity
        self.dense = layerpool.Dense(self.model, plan, self.capacity) if backend == "layers" else None
        self._ar = torch.arange(self.frame_len, device=self.device) if backend == "layers" else None
        self._rs.to(self.device)            # (the conversion tables follow the model's device)
        self._rs_size_hist()

    def invalidate_packed_weights(self):
        """Re-pack the weight blob on the next call (``CleanUMamba.invalidate_packed_weights`` calls this)."""
        self._stale = True

    def _slots(self, slots):
        a = np.asarray([int(s) for s in slots], dtype=np.int64)
        if a.size and (a.min() < 0 or a.max() >= self.capacity):
            raise ValueError(f"stream pool: slot ids must lie in [0, {self.capacity})")
        if np.unique(a).size != a.size:
            raise ValueError("stream pool: a slot is named twice in one call")
        shut = a[~self._open[a]]
        if shut.size:
            raise ValueError(f"stream pool: slot {int(shut[0])} is not open")
        return a

    # ------------------------------------------------------------------ feed / close
    @torch.no_grad()
    def feed(self, slots, x):
        """New samples of the named slots: ``x`` (len(slots), L) f32 on the pool's GPU, or a list of 1-D tensors (one per
        slot, any lengths).  Returns one 1-D tensor per slot, a multiple of ``total_stride`` long: views of one buffer.
        A rated slot's chunk is at the slot's rate, and so is what it gets back: the samples that became final, any
        number of them (none while the chunks are shorter than the filters' delay)."""
        a = self._slots(slots)
        if isinstance(x, (list, tuple)):
            if len(x) != a.size or any(t.dim() != 1 for t in x):
                raise ValueError("stream pool: feed takes one 1-D tensor per slot")
            lengths = np.asarray([t.shape[0] for t in x], dtype=np.int64)
            x = torch.nn.utils.rnn.pad_sequence(list(x), batch_first=True) if a.size else None
        else:
            if x.dim() != 2 or x.shape[0] != a.size:
                raise ValueError("stream pool: x must be (len(slots), samples)")
            lengths = np.full(a.size, x.shape[1], dtype=np.int64)
            if x.shape[1] > 1 and x.stride(1) != 1:
                x = x.contiguous()
        if x is not None and (x.dtype != torch.float32 or x.device != self.device):
            raise ValueError(f"stream pool: samples must be f32 on {self.device}")
        rated = self._rate[a] > 0
        if not rated.any():
            return self._run(a, x, lengths)
        return self._feed_rated(a, x, lengths, rated)

    @torch.no_grad()
    def close(self, slots):
        """End the named slots' streams: what ``flush`` gives a lone stream (its pending samples padded with the zeros
        ``forward`` adds, the remaining hops, the decoder's drain), one 1-D tensor per slot.  The slots are free again.

        A rated slot: its in-conversion ends (outputs through ``out_length(received)``), what that gives is fed, the
        model's close follows, and all of it with the end of the signal goes through the out-conversion, cropped so that
        everything the slot returned adds up to exactly the samples it was fed.  Its conversion state is zeroed."""
        a = self._slots(slots)
        rated = self._rate[a] > 0
        if not rated.any():
            return self._close_model(a)
        if self.device.type != "cuda":
            raise RuntimeError("stream pool: the model is not on a GPU")
        n, ri = a.size, np.flatnonzero(rated)
        sr, none = a[ri], np.zeros(ri.size, dtype=np.int64)
        count, base = self._rs_step(0, sr, none, True)
        mlen = np.zeros(n, dtype=np.int64)
        mlen[ri] = count
        xm = torch.empty(n, hopplan._rup(max(int(mlen.max()), 1), 4), dtype=torch.float32, device=self.device)
        self._rs_launch(0, sr, none, count, base, True, None, ri, xm, ri)
        heads = self._run(a, xm, mlen)
        outs = self._close_model(a)
        rows = [torch.cat([heads[i], outs[i]]) for i in ri]
        olen = np.asarray([r.numel() for r in rows], dtype=np.int64)
        count, base = self._rs_step(1, sr, olen, True)
        if int(count.max()) > 0:
            src = torch.nn.utils.rnn.pad_sequence(rows, batch_first=True) if int(olen.max()) else None
            z = torch.empty(ri.size, int(count.max()), dtype=torch.float32, device=self.device)
            self._rs_launch(1, sr, olen, count, base, True, src, np.arange(ri.size), z, np.arange(ri.size))
        # a round trip never shortens a signal: the slot gets back exactly what it was fed
        crop = np.clip(self._fed[sr] - self._given[sr], 0, count)
        for j, i in enumerate(ri):
            outs[i] = z[j, :int(crop[j])] if crop[j] else torch.zeros(0, dtype=torch.float32, device=self.device)
        self.rs_hist.index_fill_(1, self._index(sr), 0.0)
        self._rate[sr] = 0
        self._rs_par[sr], self._rs_pos[sr], self._rs_parity[sr] = 0, 0, 0
        self._fed[sr], self._given[sr] = 0, 0
        return outs

    def _close_model(self, a):
        """``close`` at the model's rate."""
        hop = self.hop
        pend, frames = self._pend[a].copy(), self._frames[a].copy()
        total = frames * hop + pend
        pad = np.asarray([self.model.valid_length(int(t)) - int(t) if t > 0 else 0 for t in total], dtype=np.int64)
        x = torch.zeros(a.size, int(pad.max()) if a.size else 0, dtype=torch.float32, device=self.device)
        heads = self._run(a, x, pad)
        outs = [torch.zeros(0, dtype=torch.float32, device=self.device) for _ in range(a.size)]
        live = np.flatnonzero(total > 0)
        if live.size:
            if self.backend == "layers":
                # a gather of exactly the closing slots: their per-layer buffers are the drain's input as they are
                layers, _, std, clears = self.dense.cohort(live.size)
                layerpool.move(0, self.state, a[live], self.dense.table, clears)
                tail = streaming.drain(self.model, layers, std)
            else:
                idx = self._index(a[live])
                st = self.state.index_select(0, idx)
                std = st[:, 0:1] if self.plan.hdr["normalize"] else None
                tail = streaming.drain(self.model, self.plan.export_rows(st), std)
            for j, i in enumerate(live):
                outs[i] = torch.cat([heads[i], tail[j].to(heads[i].dtype)])[:int(pend[i])]
        if a.size:
            idx = self._index(a)
            self.state.index_fill_(0, idx, 0.0)
            self.hist.index_fill_(0, idx, 0.0)
        self._open[a] = False
        self._pend[a] = 0
        self._frames[a] = 0
        return outs

    def _index(self, a):
        """Slot ids as a device int64 index (pinned host copy: no wait on the device)."""
        if self.device.type != "cuda":
            return torch.from_numpy(a.astype(np.int64))
        return torch.from_numpy(a.astype(np.int64)).pin_memory().to(self.device, non_blocking=True)

    def _refresh_weights(self):
        wv = streaming.weights_version(self.model)
        if wv == self._wv and not self._stale:
            return
        if self.backend == "layers":
            # no blob: the fused hop re-packs through the model's pack plan; only the shapes must still be the store's
            plan = layerpool.LayerPlan(self.model)
            if (plan.shapes, plan.normalize) != (self.plan.shapes, self.plan.normalize):
                if (self._frames > 0).any() or self._pend.any():
                    raise RuntimeError("stream pool: the model's shapes changed under live slots")
                self._adopt("layers", plan)                 # (no slot holds a sample yet: nothing is lost)
            self._wv, self._stale = wv, False
            return
        try:
            plan = hopplan.HopPlan(self.model)
        except ValueError as exc:
            raise RuntimeError(f"stream pool: the weights changed into a model the one-launch hop cannot run ({exc}); "
                               "close the slots before changing them") from exc
        if plan.state_stride != self.plan.state_stride:
            raise RuntimeError("stream pool: the model's shapes changed under live slots")
        self.plan, self._wv, self._stale = plan, wv, False

    # ------------------------------------------------------------------ rated slots
    def _rs_step(self, d, s, lens, ends):
        """What ``lens`` new samples (and, with ``ends``, the end of the signal) make of direction ``d`` of slots ``s``:
        (outputs that become final, where the history starts afterwards).  Host arithmetic only."""
        pos, par = self._rs_pos[s, d], self._rs_par[s, d]
        return rs.stream_step(pos[:, 0], pos[:, 1], pos[:, 2], lens, par[:, 1], par[:, 2], par[:, 3], par[:, 4], ends)

    def _rs_launch(self, d, s, lens, count, base, ends, src, src_rows, dst, dst_rows):
        """Direction ``d`` of slots ``s`` in ONE launch of cum_resample_slots, whatever their rates: slot s[j] takes
        src[src_rows[j]][:lens[j]] behind its history and writes its ``count[j]`` new outputs to dst[dst_rows[j]]; the
        history from ``base[j]`` on goes to the slot's other row.  Slots that neither get a sample nor give one are left
        out (nothing of theirs changes)."""
        pos = self._rs_pos[s, d]
        got = pos[:, 0] + lens
        self._rs_pos[s, d] = np.stack([got, pos[:, 1] + count, base], 1)
        act = np.flatnonzero((lens > 0) | (count > 0))
        if act.size == 0:
            return
        sa = s[act]
        rec = np.zeros((act.size, rs.REC_INTS), dtype=np.int32)
        rec[:, rs.SLOT_SLOT], rec[:, rs.SLOT_PLAN] = sa, self._rs_par[sa, d, 0]
        rec[:, rs.SLOT_N_HIST], rec[:, rs.SLOT_KEEP] = pos[act, 0] - pos[act, 2], got[act] - base[act]
        rec[:, rs.SLOT_X_ROW], rec[:, rs.SLOT_N_NEW], rec[:, rs.SLOT_N_OUT] = src_rows[act], lens[act], count[act]
        rec[:, rs.SLOT_Y_ROW], rec[:, rs.SLOT_ENDS] = dst_rows[act], int(bool(ends))
        rec[:, rs.SLOT_PARITY] = self._rs_parity[sa, d]
        wide = rec.view(np.int64)                        # the history's position, the first output's
        wide[:, rs.REC_IN0 // 2], wide[:, rs.REC_OUT0 // 2] = pos[act, 2], pos[act, 1]
        self._rs_parity[sa, d] ^= 1
        host = torch.from_numpy(rec).pin_memory()
        drec = host.to(self.device, non_blocking=True)
        hist = self.rs_hist[d]
        rows, pitch = (0, 0) if src is None else (src.shape[0], max(src.stride(0), src.shape[1]))
        with torch.cuda.device(self.device):
            hip.check(hip.lib().cum_resample_slots(
                hip.ptr(hist), hist.stride(1), self.capacity, *self._rs.args(), hip.ptr(host), hip.ptr(drec), act.size,
                None if rows == 0 else hip.ptr(src), rows, pitch, hip.ptr(dst), dst.shape[0],
                max(dst.stride(0), dst.shape[1]), hip.stream_ptr()))

    def _feed_rated(self, a, x, lengths, rated):
        """``feed`` of a call that names rated slots: their chunks become model-rate chunks in one launch (the others'
        are copied beside them), the call runs as any other, and what it gives the rated slots goes back to their rates
        in one launch."""
        if self.device.type != "cuda":
            raise RuntimeError("stream pool: the model is not on a GPU")
        n, ri, ui = a.size, np.flatnonzero(rated), np.flatnonzero(~rated)
        sr = a[ri]
        empty = torch.zeros(0, dtype=torch.float32, device=self.device)
        self._fed[sr] += lengths[ri]
        count, base = self._rs_step(0, sr, lengths[ri], False)
        mlen = lengths.copy()
        mlen[ri] = count
        xm = torch.empty(n, hopplan._rup(max(int(mlen.max()), 1), 4), dtype=torch.float32, device=self.device)
        wu = int(lengths[ui].max()) if ui.size else 0
        if wu:
            idx = self._index(ui)
            xm[:, :wu].index_copy_(0, idx, x[:, :wu].index_select(0, idx))
        self._rs_launch(0, sr, lengths[ri], count, base, False, x, ri, xm, ri)
        res = self._hops(a, xm, mlen)
        outs = [empty] * n
        olen = np.zeros(ri.size, dtype=np.int64)
        if res is not None:
            out, row, width = res
            for i in ui:
                outs[i] = out[row[i], :width[i]]
            olen = width[ri]
        count, base = self._rs_step(1, sr, olen, False)
        if res is not None and int(olen.max()) > 0:
            z = torch.empty(ri.size, max(int(count.max()), 1), dtype=torch.float32, device=self.device)
            self._rs_launch(1, sr, olen, count, base, False, out, row[ri], z, np.arange(ri.size))
            for j, i in enumerate(ri):
                outs[i] = z[j, :count[j]]
        self._given[sr] += count
        return outs

    # ------------------------------------------------------------------ the call at the model's rate
    def _run(self, a, x, lengths):
        res = self._hops(a, x, lengths)
        if res is None:
            # nothing arrives: no slot reaches a frame (pending < frame_len), nothing changes
            return [torch.zeros(0, dtype=torch.float32, device=self.device) for _ in range(a.size)]
        out, row, width = res
        if (width == width[0]).all():
            rows = out.unbind(0)
            return [rows[r] for r in row]
        return [out[r, :w] for r, w in zip(row, width)]

    def _hops(self, a, x, lengths):
        """The staging launch, the first-frame cohort and the slotted hop of one call.  -> (out, row, width): slot a[i]'s
        output is out[row[i], :width[i]]; None when no sample arrives."""
        n = a.size
        hop, F = self.hop, self.frame_len
        if n == 0 or int(lengths.sum()) == 0:
            return None
        if self.device.type != "cuda":
            raise RuntimeError("stream pool: the model is not on a GPU")
        self._refresh_weights()
        pend = self._pend[a]
        sch = schedule(pend, self._frames[a] > 0, lengths, F, hop)
        # stage / output rows: the first-frame cohort first (its frames are then one slice of the staged rows)
        order = np.argsort(~sch.first, kind="stable")
        row = np.empty(n, dtype=np.int64)
        row[order] = np.arange(n)
        k = int(sch.first.sum())
        total = pend + lengths
        stage = torch.empty(n, hopplan._rup(max(int(total.max()), 1), 4), dtype=torch.float32, device=self.device)
        out = torch.empty(n, int(sch.consumed.max()), dtype=torch.float32, device=self.device)
        # one host table, one copy: staging records, slotted-hop records (longest first), the cohort's slot ids
        hops = np.flatnonzero(sch.n_hops > 0)
        hops = hops[np.argsort(-sch.n_hops[hops], kind="stable")]
        m = hops.size
        rounds = self._rounds(a, sch, hops, row, stage.stride(0), out.stride(0)) if self.backend == "layers" else None
        ids = (n + m) * _REC                            # the cohort's slot ids, padded to keep the rounds 8-byte aligned
        rnd = ids + k + (k & 1)
        tab = np.zeros(rnd + (0 if rounds is None else rounds[1].size), dtype=np.int32)
        srec = tab[:n * _REC].reshape(n, _REC)
        srec[:, 0], srec[:, 1], srec[:, 2], srec[:, 3] = a, pend, lengths, sch.consumed
        srec[:, 4], srec[:, 5] = np.arange(n), row
        hrec = tab[n * _REC:(n + m) * _REC].reshape(m, _REC)
        hrec[:, 0], hrec[:, 1] = a[hops], sch.n_hops[hops]
        hrec[:, 2], hrec[:, 3] = row[hops], sch.offset[hops]
        hrec[:, 4], hrec[:, 5] = row[hops], sch.offset[hops]
        tab[ids:ids + k] = a[order[:k]]
        if rounds is not None:
            tab[rnd:] = rounds[1]
        host = torch.from_numpy(tab).pin_memory()
        dtab = host.to(self.device, non_blocking=True)
        lib = hip.lib()
        xs = x if x.numel() else stage              # (a call of empty chunks reads no sample)
        with torch.cuda.device(self.device):
            hip.check(lib.cum_stream_pool_stage(hip.ptr(self.hist), self.hist.stride(0), self.capacity, hip.ptr(host),
                                                hip.ptr(dtab), n, hip.ptr(xs), xs.stride(0), hip.ptr(stage),
                                                stage.stride(0), hip.stream_ptr()))
        if k:
            self._first_frames(stage[:k, :F], out[:k, :hop], dtab[ids:ids + k].long(), a[order[:k]])
        if m and rounds is not None:
            self._layer_rounds(a[hops], rounds[0], dtab[rnd:], stage, out)
        elif m:
            p = self.plan
            with torch.cuda.device(self.device):
                hip.check(lib.cum_stream_hop_slots(
                    hip.ptr(p.plan), hip.ptr(p.weights), hip.ptr(self.state), p.state_stride, self.capacity,
                    hip.ptr(host[n * _REC:]), hip.ptr(dtab[n * _REC:]), m, hip.ptr(stage), stage.stride(0),
                    hip.ptr(out), out.stride(0), p.lds_bytes, hip.stream_ptr()))
        self._pend[a] = sch.remainder
        self._frames[a] += sch.first + sch.n_hops
        return out, row, sch.consumed

    def _first_frames(self, frame, dst, slot_idx, slots):
        """The first frame of the slots ``slots`` (``slot_idx``: the same on the device) (k, frame_len) on the per-layer
        fused path, in a private streaming context, as ``feed_batch`` runs a stream's first frame; their state goes into
        the pool's block: converted rows (the kernel's layout), or one scatter of the buffers as they are ("layers")."""
        state = streaming.StreamState()
        state.params = streaming.new_params(self.model, frame.shape[0])
        dst.copy_(streaming.first_frame(self.model, state, frame, streaming.fused_hop))
        if self.backend == "layers":
            std = state.input_std if self.plan.normalize else self.dense.std[:frame.shape[0]]
            table = layerpool.MoveTable(self.plan, state.layers, state.params.key_value_memory_dict, std)
            layerpool.move(1, self.state, slots, table)
            return
        self.plan.import_state(state, into=self.state, at=slot_idx)

    # ------------------------------------------------------------------ the hops of the "layers" backend
    def _rounds(self, a, sch, hops, row, stage_pitch, out_pitch):
        """The running slots' hops as rounds of dense batches: round r runs the slots with n_hops > r, the first ``counts[r]``
        of ``hops`` (longest first).  -> (counts, the rounds' part of the call's table): per round the position of every
        slot's frame in the staged rows and of its output (int64), and the pair (1 / f, 1 - 1 / f) of its running std,
        f the frame's number in the slot's own stream (Python floats, as ``streaming.first_frame`` computes them)."""
        nh = sch.n_hops[hops]
        counts = [int((nh > r).sum()) for r in range(int(nh[0]) if hops.size else 0)]
        frames = self._frames[a[hops]] + sch.first[hops]
        start = sch.offset[hops]
        parts = []
        for r, c in enumerate(counts):
            at = start[:c] + r * self.hop
            f = (frames[:c] + r + 1).astype(np.float64)
            coef = np.stack([1.0 / f, 1.0 - 1.0 / f], 1).astype(np.float32)
            pos = np.concatenate([row[hops[:c]] * stage_pitch + at, row[hops[:c]] * out_pitch + at]).astype(np.int64)
            parts += [pos.view(np.int32), coef.reshape(-1).view(np.int32)]       # (positions as int64: 2 ints each)
        return counts, np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)

    def _layer_rounds(self, slots, counts, dtab, stage, out):
        """Run the rounds (``_rounds``) of the slots ``slots`` (longest first).  A round whose cohort equals the previous
        round's runs on the dense state as it stands: rows move only where the cohort changes -- all of them in before
        round 0, a slot's out behind its last round -- so every row is gathered once and scattered once per call."""
        model, hop, norm = self.model, self.hop, self.plan.normalize
        flat_in, flat_out, ar = stage.view(-1), out.view(-1), self._ar
        cur, o = 0, 0
        for c in counts:
            if c != cur:
                layers, params, std, clears = self.dense.cohort(c)
                if cur:
                    # the cohort shrinks to its first c slots, which stay where they are: the others' rows go back, then
                    # the framing rows of a batch of c are cleared (they lie where stream c was)
                    layerpool.move(1, self.state, slots[c:cur], self.dense.tail(c))
                    layerpool.move(0, self.state, slots[:0], self.dense.table, clears)
                else:
                    layerpool.move(0, self.state, slots[:c], self.dense.table, clears)
                cur = c
            pos = dtab[o:o + 4 * c].view(torch.int64)
            at_in, at_out = pos[:c], pos[c:]
            coef = dtab[o + 4 * c:o + 6 * c].view(torch.float32).view(c, 2)
            o += 6 * c
            frame = flat_in[at_in[:, None] + ar[None, :]]
            if norm:
                std.copy_((frame.std(1, keepdim=True) + 1e-3) * coef[:, 0:1] + coef[:, 1:2] * std)
                frame = frame / std
            with cs.small_m_gemms():
                y = streaming._fused_hop(model, layers, params, frame)[:, :hop]
            flat_out[at_out[:, None] + ar[None, :hop]] = y * std if norm else y
        if cur:
            layerpool.move(1, self.state, slots[:cur], self.dense.table)
