"""Ragged batches: clips of different lengths through ONE fused forward, each equal to its forward alone.

The reference denoises a folder one file per forward (src/examples/denoise.py:42-60: ``batch_size=1``, then
``sampling(model, noisy_audio)``), because a batch there is a rectangle and padding changes the answer.  Why it does, and
what repairs it: the encoder (row t reads rows 2t .. 2t + 3 below it) and the Mamba bottleneck (causal)
give a clip's own rows the same values whatever stands behind them in the batch; a transposed conv's output rows
2T, 2T + 1 take taps from input row T, which does not exist when the clip runs alone and is not zero in a padded batch
(biases, skips).  Clearing rows ``t >= T_j(b)`` of the GLU output of each of the E decoder layers -- ``T_j(b)`` the row
count of that level when clip b runs alone, ``level_rows`` -- makes the padded batch equal the lone forwards (1e-15 on the
f64 oracle).  Nothing else changes: the encoder, the bottleneck, tsfm_conv2 and every GEMM are the launches ``forward``
makes.

  level_rows        rows of every level of the U-net for a clip of L samples (pure)
  plan_batches      which clips share a batch: bounded batch, sample budget and padding waste (pure)
  forward_ragged    one padded batch: per-clip std, framing, the masked decoder, per-clip crop (csrc/ragged.hip)
  denoise_batch     a list of clips of any lengths -> their denoised versions, in order; with ``rates`` each clip at
                    its own sample rate (converted to the model's and back by util/resample.py)
  denoise_batch_pcm16  the same plan and forwards, quantised on the device into one flat int16 buffer (the layout
                    util/metrics.py scores): nothing of the audio comes back to the host
"""
import collections
import ctypes

import numpy as np
import torch

from .. import hip
from . import convstack as cs

Batch = collections.namedtuple("Batch", ["indices", "long"])
PCM_SCALE = 1.0 / 32768.0


def level_rows(L, E, kernel_size=4, stride=2):
    """[t_0, ..., t_E]: rows of the padded input and of every encoder level for a clip of L samples -- t_0 =
    valid_length(L) (src/network/CleanUMamba.py:210-225), t_{i+1} = (t_i - k) / s + 1.  Decoder layer j (0 = deepest) reads
    t_{E-j} rows and limits its GLU output to them."""
    t = int(L)
    for _ in range(E):
        t = 1 if t < kernel_size else 1 + -(-(t - kernel_size) // stride)
    rows = [t]
    for _ in range(E):
        rows.append((rows[-1] - 1) * stride + kernel_size)
    return rows[::-1]


def plan_batches(lengths, valid_length, max_batch=32, budget_samples=32 * 160000, max_waste=0.25):
    """Batches for ``forward_ragged``: [Batch(indices, long)], every index exactly once.  Clips are taken longest first;
    a clip joins the open batch only if afterwards the batch has at most ``max_batch`` clips, B * valid_length(longest)
    <= ``budget_samples`` and waste = 1 - sum(valid_length(L_i)) / (B * valid_length(longest)) <= ``max_waste`` -- so the
    padded share of a batch is capped by construction.  A clip that alone exceeds the budget is a batch of one marked
    ``long`` (it goes through ``denoise_long``).  The defaults are the benched E6 shape: 32 clips of 10 s."""
    if max_batch < 1:
        raise ValueError("plan_batches: max_batch must be at least 1")
    vl = [int(valid_length(int(n))) for n in lengths]
    order = sorted(range(len(vl)), key=lambda i: (-int(lengths[i]), i))
    batches, cur, cur_sum = [], [], 0
    for i in order:
        if vl[i] > budget_samples:
            batches.append(Batch([i], True))
            continue
        if cur:
            n, top = len(cur) + 1, vl[cur[0]]
            if n <= max_batch and n * top <= budget_samples and 1 - (cur_sum + vl[i]) / (n * top) <= max_waste:
                cur.append(i)
                cur_sum += vl[i]
                continue
            batches.append(Batch(cur, False))
        cur, cur_sum = [i], vl[i]
    if cur:
        batches.append(Batch(cur, False))
    return batches


class RaggedTables:
    """What a ragged batch carries through ``_forward_fused`` (the way ``carry=`` travels): the clips' lengths and, per
    decoder layer, the rows of the GLU output each clip keeps -- one i32 device tensor [1 + E, B], uploaded once."""

    def __init__(self, lengths, Lmax, E, kernel_size, stride, device):
        self.lengths = [int(n) for n in lengths]
        levels = [level_rows(n, E, kernel_size, stride) for n in self.lengths]
        self.batch_rows = level_rows(Lmax, E, kernel_size, stride)
        dec = [[lv[E - j] for lv in levels] for j in range(E)]
        self.full = [all(r == self.batch_rows[E - j] for r in dec[j]) for j in range(E)]
        self.table = torch.tensor([self.lengths] + dec, dtype=torch.int32).to(device)
        self.len = self.table[0]
        self.dec_rows = [self.table[1 + j] for j in range(E)]
        self.E = E
        self.routes = []

    def rows_of(self, j, geo):
        """Device i32[B] row limits of decoder layer j's GLU output (geometry ``geo``), or None where every clip of the
        batch has all of the batch's rows at that layer (nothing to clear: the plain launch)."""
        if geo.T != self.batch_rows[self.E - j] or geo.B != len(self.lengths):
            raise RuntimeError("ragged tables do not belong to this batch geometry")
        return None if self.full[j] else self.dec_rows[j]


def _check_lengths(lengths, normalize, Lmax=None):
    low = 2 if normalize else 1
    for n in lengths:
        if n < low or (Lmax is not None and n > Lmax):
            raise ValueError(f"ragged batch: a clip of {n} samples -- lengths must be at least {low}"
                             + (" (the std of one sample is undefined)" if normalize else "")
                             + (f" and at most the batch's {Lmax}" if Lmax is not None else ""))


def _rows2d(x):
    if x.dim() == 3:
        if x.shape[1] != 1:
            raise ValueError("forward_ragged takes (B, Lmax) or (B, 1, Lmax)")
        x = x[:, 0]
    if x.dim() != 2:
        raise ValueError("forward_ragged takes (B, Lmax) or (B, 1, Lmax)")
    if x.dtype not in (torch.int16, torch.float32):
        raise ValueError(f"forward_ragged takes int16 PCM or float32 samples (got {x.dtype})")
    if not x.is_cuda:
        raise RuntimeError("forward_ragged: the batch must be on the GPU (there is no CPU fallback)")
    if x.stride(1) != 1:
        x = x.contiguous()
    return x


def clip_std_ragged(x2, lens, eps):
    """(B, Lmax) int16 / f32 rows, device i32[B] -> (B,) f32: unbiased std of each clip's own samples + eps."""
    B, Lmax = x2.shape
    out = torch.empty(B, dtype=torch.float32, device=x2.device)
    with torch.cuda.device(x2.device):
        hip.check(hip.lib().cum_clip_std_ragged(int(x2.dtype == torch.int16), hip.ptr(x2), B, Lmax, x2.stride(0),
                                                hip.ptr(lens), ctypes.c_float(eps), hip.ptr(out), hip.stream_ptr()))
    return out


def frame_input_ragged(x2, lens, std, T, dtype):
    """Rows / std (int16 rows times 2^-15 first) -> the row buffer of Geo(B, T, 1): zeros from each clip's length on."""
    B, Lmax = x2.shape
    geo = cs.Geo(B, T, 1)
    buf = geo.new(dtype, x2.device)
    with torch.cuda.device(x2.device):
        hip.check(hip.lib().cum_frame_rows_ragged(hip.dtype_code(dtype), int(x2.dtype == torch.int16), hip.ptr(x2), B, Lmax,
                                                  x2.stride(0), hip.ptr(lens), T, geo.R, hip.ptr(std), hip.ptr(buf),
                                                  hip.stream_ptr()))
    return buf


def unframe_ragged(buf, geo, lens, std, Lmax):
    """Row buffer of the 1-channel output -> (B, 1, Lmax) f32: rows * std in each clip's own length, zeros behind."""
    y = torch.empty(geo.B, 1, Lmax, dtype=torch.float32, device=buf.device)
    with torch.cuda.device(buf.device):
        hip.check(hip.lib().cum_unframe_rows_ragged(hip.dtype_code(buf.dtype), hip.ptr(buf), geo.B, Lmax, geo.T, hip.ptr(lens),
                                                    hip.ptr(std), hip.ptr(y), hip.stream_ptr()))
    return y


def _check_flat(flat, offsets, B, what):
    if not (torch.is_tensor(flat) and flat.is_cuda and flat.dtype == torch.int16 and flat.dim() == 1
            and flat.is_contiguous()):
        raise ValueError(f"{what}: the flat buffer must be a contiguous 1-D int16 tensor on the GPU")
    if not (torch.is_tensor(offsets) and offsets.device == flat.device and offsets.dtype == torch.int64
            and offsets.shape == (B,) and offsets.is_contiguous()):
        raise ValueError(f"{what}: offsets must be a contiguous int64[{B}] tensor on the flat buffer's device")


def unframe_ragged_pcm16(buf, geo, lens, std, Lmax, flat, offsets, mode):
    """Row buffer of the 1-channel output -> int16 PCM in ``flat``: clip b's rows * std, quantised by ``mode`` (0:
    * 32767, truncated; 1: * 32768, rounded half to even), at flat[offsets[b] : offsets[b] + lens[b]] (device i64[B])."""
    _check_flat(flat, offsets, geo.B, "unframe_ragged_pcm16")
    with torch.cuda.device(buf.device):
        hip.check(hip.lib().cum_unframe_rows_ragged_pcm16(hip.dtype_code(buf.dtype), hip.ptr(buf), geo.B, Lmax, geo.T,
                                                          hip.ptr(lens), hip.ptr(std), int(mode), hip.ptr(flat),
                                                          hip.ptr(offsets), hip.stream_ptr()))


def pcm16_from_f32_ragged(x, lens, flat, offsets, mode):
    """(B, pitch) f32 device rows (``resample_ragged``'s output), device i32[B] lengths -> int16 PCM in ``flat`` at the
    device i64[B] sample offsets, quantised by ``mode`` as ``unframe_ragged_pcm16`` does."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1):
        raise ValueError("pcm16_from_f32_ragged takes (B, pitch) float32 rows on the GPU")
    B, Lmax = x.shape
    _check_flat(flat, offsets, B, "pcm16_from_f32_ragged")
    with torch.cuda.device(x.device):
        hip.check(hip.lib().cum_pcm16_from_f32_ragged(hip.ptr(x), B, Lmax, x.stride(0), hip.ptr(lens), int(mode),
                                                      hip.ptr(flat), hip.ptr(offsets), hip.stream_ptr()))


def ragged_supported(model):
    """What ``forward_ragged`` needs of a model: the fused conv stack and one output channel."""
    return bool(getattr(model, "use_fused_convs", True)) and hasattr(model, "encoder_n_layers") and cs.supported(model) \
        and model.channels_output == 1


def forward_ragged(model, x, lengths, pcm16=None):
    """pcm16 = (flat int16 device buffer, device i64[B] sample offsets, mode): the last step quantises each clip into
    ``flat`` (``unframe_ragged_pcm16``) and nothing is returned; None: the (B, 1, Lmax) f32 result."""
    if torch.is_grad_enabled():
        raise RuntimeError("forward_ragged is inference only: call it under torch.no_grad()")
    x2 = _rows2d(x)
    B, Lmax = x2.shape
    if B < 1 or Lmax < 1:
        raise ValueError("forward_ragged: an empty batch")
    if not getattr(model, "use_fused_convs", True) or not cs.supported(model) or model.channels_output != 1:
        raise NotImplementedError("forward_ragged runs on the fused conv stack: kernel 4 / stride 2 / ungrouped / "
                                  "sigmoid-GLU layers, one output channel")
    if torch.is_tensor(lengths):
        lengths = lengths.tolist()               # (a device table comes back once: the row limits are built on the host)
    lengths = [int(n) for n in lengths]
    if len(lengths) != B:
        raise ValueError(f"forward_ragged: {len(lengths)} lengths for {B} clips")
    _check_lengths(lengths, model.normalize_input, Lmax)
    if pcm16 is not None:                        # before any launch
        _check_flat(pcm16[0], pcm16[1], B, "forward_ragged")
        if pcm16[2] not in (0, 1):
            raise ValueError("forward_ragged: pcm16 mode must be 0 (* 32767, truncated) or 1 (* 32768, rounded)")
    E = model.encoder_n_layers
    tables = RaggedTables(lengths, Lmax, E, model.kernel_size, model.stride, x2.device)
    std = clip_std_ragged(x2, tables.len, 1e-3) if model.normalize_input else None
    T0 = model.valid_length(Lmax)
    dt = model._fused_dtype()
    buf = frame_input_ragged(x2, tables.len, std, T0, dt)
    with cs.small_m_gemms():                     # as ``forward`` without grad
        buf, geo, _, _ = model._forward_fused(buf, B, T0, dt, ragged=tables)
    model.__dict__["_ragged_routes"] = tables.routes
    if pcm16 is not None:
        flat, offsets, mode = pcm16
        unframe_ragged_pcm16(buf, geo, tables.len, std, Lmax, flat, offsets, mode)
        return None
    return unframe_ragged(buf, geo, tables.len, std, Lmax)


def stack_clips(clips, device, pinned=None):
    """1-D clips (all int16, or f32 / mixed: int16 ones are scaled by 2^-15) -> ((B, pitch) device tensor, Lmax): host
    clips are gathered in one pinned staging tensor and uploaded ONCE; device clips are copied row by row.  The samples
    behind a clip's length are never read by the ragged kernels and are left as they are."""
    Lmax = max(int(c.shape[0]) for c in clips)
    pitch = cs.rup(Lmax, 8)                      # 16-byte rows for both element types
    dtype = torch.int16 if all(c.dtype == torch.int16 for c in clips) else torch.float32
    host = not any(c.is_cuda for c in clips)
    if host:
        stage = pinned if pinned is not None and pinned.dtype == dtype and pinned.numel() >= len(clips) * pitch else \
            torch.empty(len(clips) * pitch, dtype=dtype, pin_memory=True)
        rows = stage[:len(clips) * pitch].view(len(clips), pitch)
    else:
        rows = torch.empty(len(clips), pitch, dtype=dtype, device=device)
    for b, c in enumerate(clips):
        if c.dtype == torch.int16 and dtype == torch.float32:
            c = c.to(torch.float32) * PCM_SCALE
        rows[b, :c.shape[0]].copy_(c)
    if host:
        rows = rows.to(device, non_blocking=True)
    return rows, Lmax


def denoise_batch(model, clips, max_batch=32, budget_samples=32 * 160000, max_waste=0.25, rates=None, model_rate=16000):
    if torch.is_grad_enabled():
        with torch.no_grad():
            return denoise_batch(model, clips, max_batch, budget_samples, max_waste, rates, model_rate)
    clips = list(clips)
    for c in clips:
        if not torch.is_tensor(c) or c.dim() != 1 or c.dtype not in (torch.int16, torch.float32):
            raise ValueError("denoise_batch takes 1-D int16 or float32 tensors")
    if rates is not None:
        rates = [rates] * len(clips) if not isinstance(rates, (list, tuple)) else list(rates)
        if len(rates) != len(clips):
            raise ValueError(f"denoise_batch: {len(rates)} rates for {len(clips)} clips")
        if any(r != model_rate for r in rates):
            return _denoise_batch_at_rates(model, clips, rates, model_rate, max_batch, budget_samples, max_waste)
    lengths = [int(c.shape[0]) for c in clips]
    _check_lengths(lengths, model.normalize_input)
    device = next(model.parameters()).device
    out = [None] * len(clips)
    for batch in plan_batches(lengths, model.valid_length, max_batch, budget_samples, max_waste):
        if batch.long:
            i = batch.indices[0]
            c = clips[i]
            c = (c.to(torch.float32) * PCM_SCALE) if c.dtype == torch.int16 else c
            y = model.denoise_long(c.to(device).view(1, -1))
            out[i] = y[0, 0, :lengths[i]]
            continue
        rows, Lmax = stack_clips([clips[i] for i in batch.indices], device)
        lens = [lengths[i] for i in batch.indices]
        y = forward_ragged(model, rows[:, :Lmax], lens)
        for b, i in enumerate(batch.indices):
            out[i] = y[b, 0, :lens[b]]
    return out


def denoise_batch_pcm16(model, clips, mode=0, max_batch=32, budget_samples=32 * 160000, max_waste=0.25):
    """``denoise_batch`` whose result stays on the device as int16 PCM: the same plan, the same staging and the same
    forwards, every batch quantised by its last kernel (``mode`` 0: * 32767, clamped, truncated -- validate's rule; 1:
    * 32768, rounded half to even, clamped) into ONE flat int16 device buffer, clips packed back to back in the caller's
    order -- the layout of util/metrics.py ``Batch``.  -> (flat, offsets, lengths): the buffer and two host int64 arrays;
    clip i is flat[offsets[i] : offsets[i] + lengths[i]].  A clip over the budget goes through ``denoise_long`` and is
    quantised by ``pcm16_from_f32_ragged``."""
    if torch.is_grad_enabled():
        with torch.no_grad():
            return denoise_batch_pcm16(model, clips, mode, max_batch, budget_samples, max_waste)
    clips = list(clips)
    for c in clips:
        if not torch.is_tensor(c) or c.dim() != 1 or c.dtype not in (torch.int16, torch.float32):
            raise ValueError("denoise_batch_pcm16 takes 1-D int16 or float32 tensors")
    if mode not in (0, 1):
        raise ValueError("denoise_batch_pcm16: mode must be 0 (* 32767, truncated) or 1 (* 32768, rounded)")
    lengths = np.array([int(c.shape[0]) for c in clips], np.int64)
    _check_lengths(lengths.tolist(), model.normalize_input)
    offsets = (np.cumsum(lengths) - lengths).astype(np.int64)
    device = next(model.parameters()).device
    flat = torch.empty(int(lengths.sum()), dtype=torch.int16, device=device)
    batches = plan_batches(lengths.tolist(), model.valid_length, max_batch, budget_samples, max_waste)
    # one upload for the offsets of every batch (and one for the lengths of the long clips): a batch takes its slice
    order = [i for batch in batches for i in batch.indices]
    offs_dev = torch.from_numpy(offsets[order]).to(device)
    lens_dev = torch.from_numpy(lengths[order].astype(np.int32)).to(device)
    at = 0
    for batch in batches:
        B = len(batch.indices)
        offs, at = offs_dev[at:at + B], at + B
        if batch.long:
            i = batch.indices[0]
            c = clips[i]
            c = (c.to(torch.float32) * PCM_SCALE) if c.dtype == torch.int16 else c
            y = model.denoise_long(c.to(device).view(1, -1))
            pcm16_from_f32_ragged(y[0, :, :int(lengths[i])], lens_dev[at - 1:at], flat, offs, mode)
            continue
        rows, Lmax = stack_clips([clips[i] for i in batch.indices], device)
        forward_ragged(model, rows[:, :Lmax], [int(lengths[i]) for i in batch.indices], pcm16=(flat, offs, mode))
    return flat, offsets, lengths


def _resample_group(clips, rate_in, rate_out, device, max_batch, pcm16=None):
    """1-D clips of one rate -> their conversions to ``rate_out`` (f32 device tensors), ``max_batch`` clips a launch.
    int16 clips stay int16 up to the kernel.  pcm16 = (flat int16 device buffer, device i64[len(clips)] sample offsets,
    mode): every launch's rows are quantised into ``flat`` at their clips' offsets instead (``pcm16_from_f32_ragged``)
    and nothing is returned; the lengths table is uploaded once per launch and stays on the device."""
    from ..util.resample import resample_ragged
    out = []
    for k in range(0, len(clips), max_batch):
        part = clips[k:k + max_batch]
        rows, Lmax = stack_clips(part, device)
        if pcm16 is not None:
            flat, offsets, mode = pcm16
            lens = torch.tensor([int(c.shape[0]) for c in part], dtype=torch.int32).to(device)
            y, n = resample_ragged(rows[:, :Lmax], lens, rate_in, rate_out)
            pcm16_from_f32_ragged(y, n, flat, offsets[k:k + len(part)], mode)
            continue
        y, n = resample_ragged(rows[:, :Lmax], [int(c.shape[0]) for c in part], rate_in, rate_out)
        out += [y[b, :n[b]] for b in range(len(part))]
    return out


def _denoise_batch_at_rates(model, clips, rates, model_rate, max_batch, budget_samples, max_waste):
    """``denoise_batch`` for clips at their own sample rates: every clip whose rate is not the model's is converted to
    it (one launch per rate and ``max_batch`` clips, util/resample.py), the whole list is denoised as one
    ``denoise_batch`` call at the model's rate -- so the batches are planned, and the lengths checked, on the converted
    lengths -- and every converted clip is taken back to its own rate and cropped to its own length (a round trip never
    shortens a clip).  Clips at the model's rate pass through untouched."""
    from ..util.resample import plan
    groups = {}
    for i, r in enumerate(rates):
        if r != model_rate:
            plan(r, model_rate), plan(model_rate, r)         # ValueError for a rate that cannot be converted, before any work
            groups.setdefault(int(r), []).append(i)
    device = next(model.parameters()).device
    at_model = list(clips)
    for r, idx in groups.items():
        for i, y in zip(idx, _resample_group([clips[i] for i in idx], r, model_rate, device, max_batch)):
            at_model[i] = y
    out = denoise_batch(model, at_model, max_batch, budget_samples, max_waste)
    for r, idx in groups.items():
        for i, y in zip(idx, _resample_group([out[i] for i in idx], model_rate, r, device, max_batch)):
            out[i] = y[:clips[i].shape[0]]
    return out
