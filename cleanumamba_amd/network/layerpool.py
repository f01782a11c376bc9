"""Slot store and dense scratch of the stream pool's "layers" backend (network/streampool.py, csrc/slotstate.hip).

A pool on the per-layer hop keeps, per slot, everything one stream of ``streaming._fused_hop`` carries between hops, in
one row of an f32 store [capacity, state_stride]:

  std                 the running std (4 bytes)
  encin{i}, enc{i}    per encoder layer the compact input of the incremental hops and the layer's window, all P = T + 2
                      rows by Cp of the stream (pad rows included)
  dec{j}              per decoder layer the overlap tail (2, Cp)
  conv{k}, ssm{k}     per Mamba block the conv and SSM state of ``InferenceParams.key_value_memory_dict``

(``decbuf{j}`` is rewritten every hop and is not state.)  ``segment_table`` derives the row's layout from the model on
the host.  The hops of a cohort of n slots run on the ``Geo(n, ...)``-sized prefix of scratch tensors in the fused hop's
own layout, sized once for ``capacity`` (``Dense``); ``cum_stream_slots_move`` carries the slots' rows in and out, one
launch per direction whatever the number of segments.  Reference: the same state, for one stream, is Python attributes
of the model in CleanUMamba.feed / _denoise_frame, src/network/CleanUMamba.py:358-490.
"""
import numpy as np
import torch

from ..mamba_ssm.utils.generation import InferenceParams
from .. import hip
from . import convstack as cs

_ALIGN = 16         # every segment starts at a multiple of 16 bytes: the mover's vector path


def _shapes(model):
    """Per-stream shapes of the fused hop's state, in the row's order: (name, kind, T, C); kind "rows" is a row buffer of
    Geo(S, T, C), "tail" a (S, 2, Cp) tensor, "conv" / "ssm" a Mamba state (S, T, C), "scratch" a row buffer that carries
    nothing between hops."""
    K, st, E = model.kernel_size, model.stride, model.encoder_n_layers
    out = [("std", "std", 1, 1)]
    T, c_in, n_new = model.valid_length(1), model.encoder[0][0].weight.shape[1], model.total_stride
    for i, enc in enumerate(model.encoder):
        T = (T - K) // st + 1
        n_new //= st
        out.append((f"encin{i}", "rows", st * n_new + K - st, c_in))
        c_in = enc[2].weight.shape[0] // 2
        out.append((f"enc{i}", "rows", T, c_in))
    L = T                                           # rows of the bottleneck: 1 at valid_length(1)
    for j, dec in enumerate(model.decoder):
        C = dec[2].weight.shape[1]
        out.append((f"dec{j}", "tail", 2, C))
        if j != E - 1:
            out.append((f"decbuf{j}", "scratch", 2 * L, C))
        L *= 2
    for k, blk in enumerate(model.tsfm_Mamba_layers):
        m = blk.mixer
        di = m.in_proj.weight.shape[0] // 2
        out.append((f"conv{k}", "conv", di, m.conv1d.weight.shape[-1]))
        out.append((f"ssm{k}", "ssm", di, m.A_log.shape[1]))
    return out


def _bytes(kind, T, C):
    if kind == "rows":
        g = cs.Geo(1, T, C)
        return g.P * g.Cp * 4
    if kind == "tail":
        return 2 * cs.rup(C, 8) * 4
    return T * C * 4


def segment_table(model):
    """The layout of a slot's row: ([(name, offset in the row, bytes per stream)], row length in bytes).  Pure host
    arithmetic on the model's shapes; every offset (and the row length) is a multiple of 16 bytes."""
    segs, off = [], 0
    for name, kind, T, C in _shapes(model):
        if kind == "scratch":
            continue
        n = _bytes(kind, T, C)
        segs.append((name, off, n))
        off = cs.rup(off + n, _ALIGN)
    return segs, off


class LayerPlan:
    """What the pool needs of the model at one set of shapes (the "layers" counterpart of hopplan.HopPlan)."""

    def __init__(self, model):
        self.device = model.tsfm_conv1.weight.device
        self.hop, self.frame_len = model.total_stride, model.valid_length(1)
        self.normalize = bool(model.normalize_input)
        self.shapes = _shapes(model)
        self.segs, row_bytes = segment_table(model)
        self.state_stride = row_bytes // 4


class Dense:
    """Scratch of the dense side, sized once for ``capacity`` streams: the fused hop's per-layer buffers, the Mamba
    states and the running std; ``cohort(n)`` gives the prefix views a batch of n streams runs on."""

    def __init__(self, model, plan, capacity):
        dev, f32 = plan.device, torch.float32
        self.plan, self.capacity, self.device = plan, capacity, dev
        self.layers, self.geos = {}, {}
        for name, kind, T, C in plan.shapes:
            if kind in ("rows", "scratch"):
                self.geos[name] = (T, C)
                self.layers[name] = cs.Geo(capacity, T, C).new(f32, dev, zero=True)
            elif kind == "tail":
                self.layers[name] = torch.zeros(capacity, 2, cs.rup(C, 8), dtype=f32, device=dev)
        self.kv = model.allocate_inference_cache(capacity, 1)
        self.std = torch.zeros(capacity, 1, dtype=f32, device=dev)
        self.table = MoveTable(plan, self.layers, self.kv, self.std)
        self._cohorts, self._tails = {}, {}

    def tail(self, first):
        """The move table of the dense streams from ``first`` on (made once per ``first``)."""
        if first not in self._tails:
            self._tails[first] = _Shifted(self.table, first, self.device)
        return self._tails[first]

    def cohort(self, n):
        """(layers, InferenceParams, std (n, 1), clear records) of a batch of n streams: views, nothing is allocated on
        the device."""
        hit = self._cohorts.get(n)
        if hit is None:
            layers, clears = {}, []
            for name, t in self.layers.items():
                if name in self.geos:
                    g = cs.Geo(n, *self.geos[name])
                    layers[name] = t[:g.R]
                    clears.append((t.data_ptr(), g.head * 4, (1 + g.M) * g.Cp * 4, g.tail * 4))
                else:
                    layers[name] = t[:n]
            kv = {k: tuple(s[:n] for s in v) for k, v in self.kv.items()}
            params = InferenceParams(max_seqlen=1, max_batch_size=n, key_value_memory_dict=kv, seqlen_offset=1)
            hit = self._cohorts[n] = (layers, params, self.std[:n], np.asarray(clears, dtype=np.int64).reshape(-1, 4))
        return hit


class MoveTable:
    """The segment table of cum_stream_slots_move for one set of dense tensors (``layers`` in the fused hop's layout,
    ``kv`` a key_value_memory_dict, ``std`` (S, 1)): host copy and device copy, made once per set."""

    def __init__(self, plan, layers, kv, std):
        shapes = {name: (kind, T, C) for name, kind, T, C in plan.shapes}
        rec, self.keep = [], [std]
        self.streams = std.shape[0]              # how many streams every dense tensor holds: the bound of a move's n
        for name, off, nbytes in plan.segs:
            kind, T, C = shapes[name]
            if kind == "std":
                t, base, pitch = std, std.data_ptr(), 4
            elif kind == "rows":
                t, g = layers[name], cs.Geo(1, T, C)
                base, pitch = t.data_ptr() + g.Cp * 4, nbytes           # row 1: the first stream's first row
                if t.dim() != 2 or t.shape[1] != g.Cp or t.stride(0) != g.Cp:
                    raise RuntimeError(f"layer pool: {name} is not a row buffer of {g.Cp} columns")
                self.streams = min(self.streams, (t.shape[0] - 1 - g.slack) // g.P)
            elif kind == "tail":
                t = layers[name]
                base, pitch = t.data_ptr(), nbytes
            else:
                t = kv[int(name[4:] if kind == "conv" else name[3:])][0 if kind == "conv" else 1]
                base, pitch = t.data_ptr(), nbytes
            if t.dtype != torch.float32 or not t.is_contiguous() or (kind not in ("std", "rows")
                                                                      and t[0].numel() * 4 != nbytes):
                raise RuntimeError(f"layer pool: {name} does not have the layout of the segment table")
            if kind != "rows":
                self.streams = min(self.streams, t.shape[0])
            self.keep.append(t)
            rec.append((base, pitch, off, nbytes))
        self.n = len(rec)
        self.host = torch.from_numpy(np.asarray(rec, dtype=np.int64))
        self.dev = self.host
        if plan.device.type == "cuda":
            self.host = self.host.pin_memory()
            self.dev = self.host.to(plan.device, non_blocking=True)



class _Shifted:
    """``table`` with its dense streams counted from stream ``first`` on (the tail of a batch that shrinks)."""

    def __init__(self, table, first, device):
        rec = table.host.clone()
        rec[:, 0] += first * rec[:, 1]
        self.n, self.streams, self.keep = table.n, table.streams - first, table
        self.host = rec.pin_memory() if device.type == "cuda" else rec
        self.dev = self.host.to(device, non_blocking=True)


def move(direction, store, slots, table, clears=None):
    """One launch of cum_stream_slots_move: direction 0 gathers rows ``slots`` (host int array) of ``store`` into the dense
    tensors of ``table`` (stream j = slots[j]) and clears the ``clears`` records (with no slot: only that), 1 scatters
    them back."""
    dev = store.device
    n = int(len(slots))
    if n == 0 and (clears is None or direction == 1):
        return
    if n > table.streams or store.dtype != torch.float32 or store.stride(1) != 1:
        raise RuntimeError(f"layer pool: {n} slots moved through dense tensors of {table.streams} streams")
    nc = 0 if clears is None or direction == 1 else clears.shape[0]
    tab = np.zeros(4 * nc + (n + 1) // 2, dtype=np.int64)             # clear records, then the slot ids as int32
    if nc:
        tab[:4 * nc] = clears.reshape(-1)
    tab[4 * nc:].view(np.int32)[:n] = slots
    host = torch.from_numpy(tab).pin_memory()
    dtab = host.to(dev, non_blocking=True)
    with torch.cuda.device(dev):
        hip.check(hip.lib().cum_stream_slots_move(
            direction, hip.ptr(store), store.stride(0), store.shape[0], hip.ptr(host[4 * nc:]), hip.ptr(dtab[4 * nc:]), n,
            hip.ptr(table.host), hip.ptr(table.dev), table.n, hip.ptr(host) if nc else None,
            hip.ptr(dtab) if nc else None, nc, hip.stream_ptr()))
