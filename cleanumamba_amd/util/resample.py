"""Sample-rate conversion on the GPU (csrc/resample.hip): what lets the 16 kHz model take recordings at
8, 22.05, 32, 44.1 or 48 kHz and give them back at their own rate and length.  The reference has no resampler (it drops
the rate ``torchaudio.load`` returns, src/util/dataset.py:203).

For ``rate_in -> rate_out`` with g = gcd: up = rate_out / g, down = rate_in / g, taps h[0 .. 2H] from
``metrics.resample_taps`` (Kaiser-windowed sinc, cut-off at the lower Nyquist rate, 60 dB, odd, symmetric, sum = up), and

    n_out = ceil(L up / down)
    y[m]  = sum_{j < K} x[n_hi - j] h[r + j up],   c = m down + H, r = c mod up, n_hi = c // up, K = ceil((2H + 1) / up)

with samples outside [0, L) zero.  One f32 fma chain per output, j ascending: its bits depend on (m, up, down, H) and the
samples only, which is what makes a clip's result independent of its batch and a stream's of how it was cut.

  plan             (rate_in, rate_out) -> Plan: up, down, H, K, the f64 taps; ``plan.table(device)`` the polyphase table
  out_length       ceil(L up / down) (pure)
  final_outputs    outputs that no later input can change (pure)
  stream_step      one push of a stream: outputs now final, history to keep (pure; StreamResampler and the stream pool's
                   rated slots, network/streampool.py); history_bound: what sizes the pool's rows
  tile_span        what the kernels' LDS admits; check_fits(plan): ValueError for a pair beyond it
  crop_window      the source samples that outputs [m0, m0 + count) of a file read; window_bound: the longest such range
                   (pure; what a rated training/feeder.py stages for cum_pcm_batch_resample_f32)
  PlanTable        the pairs of one user (the stream pool, the feeder) as the plan table and tap blob of the slots and
                   feeder entries; PLAN_INTS, REC_INTS, SLOT_*, FEED_*, REC_IN0 / REC_OUT0: their rows' sizes and fields
  resample_ragged  a ragged batch in one launch
  StreamResampler  push / finish over signals of any length, bit-identical to ``resample_ragged`` on the whole signal

There is no CPU or PyTorch implementation: a tensor that is not on the GPU raises.
"""
import math
import numbers

import numpy as np
import torch

from .. import hip
from .metrics import resample_taps

MAX_FACTOR = 1024
RS_TILE = 768                # outputs of one workgroup (csrc/resample.hip: RS_TILE = cum_resample_tile())
LDS_SPAN_FLOATS = 12288      # ... and the longest input span it stages (RS_LDS_SPAN_FLOATS)
PCM_SCALE = 1.0 / 32768.0
# int32 per plan row / record of the slots and feeder entries and their fields (layouts: include/cleanumamba_hip.h)
PLAN_INTS, REC_INTS = 8, 16
(SLOT_SLOT, SLOT_PLAN, SLOT_N_HIST, SLOT_X_ROW, SLOT_N_NEW, SLOT_N_OUT, SLOT_Y_ROW, SLOT_ENDS, SLOT_KEEP, SLOT_PARITY,
 SLOT_Y_COL) = range(11)                                 # a slot record's ints
FEED_PLAN, FEED_N_SRC, FEED_M, FEED_N = range(4)         # a feeder record's ints
REC_IN0, REC_OUT0 = 12, 14                               # both records' int64 positions: ints 12-13 and 14-15
_PLANS = {}


def out_length(L, up, down):
    """Samples of an L-sample signal after up / down conversion: ceil(L up / down)."""
    return -(-int(L) * int(up) // int(down))


def final_outputs(received, up, down, H):
    """Outputs that can never change once ``received`` inputs are known: output m reads inputs up to
    floor((m down + H) / up), so it is final when m down + H < received up -- max(0, ceil((received up - H) / down)),
    capped at ``out_length(received)``."""
    return min(max(0, -(-(int(received) * int(up) - int(H)) // int(down))), out_length(received, up, down))


def stream_step(received, emitted, base, n, up, down, H, K, ends=False):
    """The bookkeeping of one push of ``n`` samples (or, with ``ends``, of the signal's end) into a stream that has
    ``received`` inputs, has ``emitted`` outputs and keeps its inputs from absolute position ``base`` on.  Returns
    ``(count, base')``: the outputs that become final -- through ``final_outputs(received + n)``, through
    ``out_length(received + n)`` at the end -- and where the history must start afterwards: at the oldest sample the next
    output reads, its n_hi = ((emitted + count) down + H) // up less the K - 1 taps behind it (never before ``base``,
    never behind the samples received).  Pure integer arithmetic; scalars or numpy int64 arrays of one entry per stream."""
    received = received + n
    if isinstance(received, np.ndarray):
        all_ = -(-received * up // down)
        final = np.where(ends, all_, np.minimum(np.maximum(0, -(-(received * up - H) // down)), all_))
        count = final - emitted
        return count, np.minimum(np.maximum(((emitted + count) * down + H) // up - (K - 1), base), received)
    final = out_length(received, up, down) if ends else final_outputs(received, up, down, H)
    count = final - emitted
    return count, min(max(((emitted + count) * down + H) // up - (K - 1), base), received)


def history_bound(K):
    """The most inputs a stream keeps between pushes: output m = final_outputs(received) is the first with
    (m down + H) // up >= received, so the history starts at or after received - (K - 1) -- K - 1 samples, whatever the
    cuts.  (Before the first final output the stream holds all it received: at most H // up <= K - 1.)"""
    return int(K) - 1


def tile_span(up, down, K):
    """Floats of LDS one workgroup's input span needs (csrc/resample.hip: rs_span_cap); the kernels take a pair only if
    this is at most ``LDS_SPAN_FLOATS``."""
    return (int(K) + ((int(up) - 1) + (RS_TILE - 1) * int(down)) // int(up) + 16 + 7) // 8 * 8


def check_fits(p):
    """ValueError for a Plan whose ``tile_span`` the kernels' LDS does not hold (every C entry refuses it as well)."""
    span = tile_span(p.up, p.down, p.K)
    if span > LDS_SPAN_FLOATS:
        raise ValueError(f"{p.rate_in} -> {p.rate_out} reduces to {p.up}/{p.down}, whose input span per tile ({span} "
                         "samples) does not fit the kernel's LDS")


def crop_window(N, up, down, H, K, m0, count):
    """(n_lo, n_cnt): the samples [n_lo, n_lo + n_cnt) of an N-sample file that its outputs [m0, m0 + count) read -- from
    the oldest tap of the first, (m0 down + H) // up - (K - 1), to the n_hi of the last, both cut to the file.  Every other
    sample may be anything (or absent): the outputs' sums over the window alone are the sums over the whole file."""
    N, up, down, H, K, m0, count = (int(v) for v in (N, up, down, H, K, m0, count))
    n_hi = min(((m0 + count - 1) * down + H) // up, N - 1)
    n_lo = min(max((m0 * down + H) // up - (K - 1), 0), n_hi)
    return n_lo, n_hi - n_lo + 1


def window_bound(count, up, down, K):
    """The longest ``crop_window`` of ``count`` outputs, whatever the file and the position: the n_hi of the last output
    is at most ceil((count - 1) down / up) behind that of the first, which has K - 1 taps before it."""
    return ((int(count) - 1) * int(down) + int(up) - 1) // int(up) + int(K)


class Plan:
    """up, down, H, K and the f64 taps of one rate pair; ``table(device)``: the taps as the (up, pitch) f32 polyphase
    table the kernel reads, table[r, j] = h[r + j up], zero padded, built on the host once per device."""

    def __init__(self, rate_in, rate_out):
        g = math.gcd(rate_in, rate_out)
        self.rate_in, self.rate_out = rate_in, rate_out
        self.up, self.down = rate_out // g, rate_in // g
        if max(self.up, self.down) > MAX_FACTOR:
            raise ValueError(f"resample: {rate_in} -> {rate_out} reduces to {self.up}/{self.down}; factors above "
                             f"{MAX_FACTOR} are not supported")
        self.identity = self.up == self.down == 1
        self.taps = resample_taps(p=rate_out, q=rate_in)
        self.H = (len(self.taps) - 1) // 2
        self.K = -(-len(self.taps) // self.up)
        self.pitch = -(-self.K // 4) * 4
        self._tables = {}

    def __iter__(self):                  # up, down, H, K, taps = plan(...)
        return iter((self.up, self.down, self.H, self.K, self.taps))

    def host_table(self):
        tab = torch.zeros(self.up, self.pitch, dtype=torch.float64)
        flat = torch.zeros(self.K * self.up, dtype=torch.float64)
        flat[:len(self.taps)] = torch.from_numpy(self.taps)
        tab[:, :self.K] = flat.view(self.K, self.up).t()
        return tab.float().contiguous()

    def table(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("resample: the table lives on the GPU (there is no CPU fallback)")
        key = device.index if device.index is not None else torch.cuda.current_device()
        if key not in self._tables:
            self._tables[key] = self.host_table().to(device)
        return self._tables[key]


def _rate(r, what):
    if isinstance(r, bool) or not isinstance(r, numbers.Real) or r != int(r) or int(r) < 1:
        raise ValueError(f"resample: {what} must be a positive integer sample rate (got {r!r})")
    return int(r)


def plan(rate_in, rate_out):
    """The Plan of ``rate_in -> rate_out`` (cached).  ValueError for rates that are not positive integers and for pairs
    whose reduced factors exceed 1024."""
    key = (_rate(rate_in, "rate_in"), _rate(rate_out, "rate_out"))
    if key not in _PLANS:
        _PLANS[key] = Plan(*key)
    return _PLANS[key]


class PlanTable:
    """The rate pairs of one user as the slots and feeder entries take them (include/cleanumamba_hip.h): ``plans`` in the
    order they were added, a plan's place its id;  ``host`` (n, PLAN_INTS) int32, row i = (up, down, taps, K, pitch,
    offset, 0, 0) of plans[i];  on ``device``: ``dev``, its copy, and ``blob``, the plans' polyphase tables end to end."""

    def __init__(self, device):
        self.device, self.plans, self._ids = torch.device(device), [], {}
        self.host = self.dev = self.blob = None

    def add(self, p):
        """The id of Plan ``p``; a pair the table does not hold yet extends it, and the device gets the longer table."""
        key = (p.rate_in, p.rate_out)
        if key not in self._ids:
            self._ids[key] = len(self.plans)
            self.plans.append(p)
            self.to(self.device)
        return self._ids[key]

    def to(self, device):
        """Build the table and the blob on ``device`` (nothing while the table is empty)."""
        self.device = torch.device(device)
        if not self.plans:
            return
        offsets = np.cumsum([0] + [p.up * p.pitch for p in self.plans])
        self.host = torch.tensor([(p.up, p.down, len(p.taps), p.K, p.pitch, off) + (0,) * (PLAN_INTS - 6)
                                  for p, off in zip(self.plans, offsets.tolist())], dtype=torch.int32)
        self.dev = self.host.to(self.device)
        self.blob = torch.cat([p.host_table().reshape(-1) for p in self.plans]).to(self.device)

    def args(self):
        """plans_host, plans, n_plans, tables, table_floats of the two entries (nulls and zeros for an empty table)."""
        if not self.plans:
            return None, None, 0, None, 0
        return hip.ptr(self.host), hip.ptr(self.dev), len(self.plans), hip.ptr(self.blob), self.blob.numel()


def _rows(x, what):
    if not torch.is_tensor(x) or x.dim() != 2 or x.dtype not in (torch.int16, torch.float32):
        raise ValueError(f"{what} takes a (B, L) int16 or float32 tensor")
    if not x.is_cuda:
        raise RuntimeError(f"{what}: the samples must be on the GPU (there is no CPU fallback)")
    if x.shape[1] > 0 and x.stride(1) != 1:
        x = x.contiguous()
    return x


def _as_f32(x):
    return x.to(torch.float32) * PCM_SCALE if x.dtype == torch.int16 else x


def _launch(p, x, lens, origin, ends, y, max_out):
    """One cum_resample_ragged launch.  x: (B, L) device rows; lens: device i32[B]; origin: device i64[B, 2] or None;
    y: (B, >= max_out) f32."""
    B, L = x.shape
    tab = p.table(x.device)
    with torch.cuda.device(x.device):
        hip.check(hip.lib().cum_resample_ragged(int(x.dtype == torch.int16), hip.ptr(x) if L else None, B, L,
                                                x.stride(0) if L else 0, hip.ptr(lens), hip.ptr(origin), int(bool(ends)),
                                                p.up, p.down, len(p.taps), p.K, hip.ptr(tab), p.pitch, hip.ptr(y),
                                                y.stride(0), int(max_out), hip.stream_ptr()))


def resample_ragged(x, lengths, rate_in, rate_out, out=None):
    """x: (B, Lmax) int16 PCM (a sample is x 2^-15) or f32 on the GPU, clip b in its first lengths[b] samples; lengths: a
    host sequence or a device i32 tensor.  -> ((B, pitch) f32, out_lengths): clip b converted to ``rate_out`` in its
    first out_lengths[b] = ceil(lengths[b] up / down) samples; what stands behind them is not written.  out_lengths is
    a list for host lengths, a device i32 tensor for device lengths.  ``out``: an f32 device tensor to write into, (B, >= the longest
    output) -- for a device length table (B, >= out_length(Lmax)).  Equal rates return the input as f32 without a launch."""
    p = plan(rate_in, rate_out)
    x = _rows(x, "resample_ragged")
    B, Lmax = x.shape
    if B < 1:
        raise ValueError("resample_ragged: an empty batch")
    if torch.is_tensor(lengths):
        if lengths.shape != (B,) or lengths.dtype != torch.int32 or lengths.device != x.device:
            raise ValueError("resample_ragged: a device length table must be i32[B] on the batch's device")
        lens = lengths.contiguous()
        out_lens = ((lens.long().clamp(0, Lmax) * p.up + p.down - 1) // p.down).to(torch.int32)
    else:
        host = [int(n) for n in lengths]
        if len(host) != B or any(n < 0 or n > Lmax for n in host):
            raise ValueError(f"resample_ragged: {B} clips need {B} lengths in [0, {Lmax}]")
        lens = torch.tensor(host, dtype=torch.int32).to(x.device)
        out_lens = [out_length(n, p.up, p.down) for n in host]
    if p.identity:
        return _as_f32(x), (lengths if torch.is_tensor(lengths) else out_lens)
    n_max = out_length(Lmax, p.up, p.down) if torch.is_tensor(lengths) else max(out_lens)   # columns the launch may write
    if out is None:
        out = torch.empty(B, -(-max(n_max, 1) // 8) * 8, dtype=torch.float32, device=x.device)
    elif (not torch.is_tensor(out) or out.dtype != torch.float32 or out.device != x.device or out.dim() != 2
          or out.shape[0] != B or out.shape[1] < n_max or (out.shape[1] > 0 and out.stride(1) != 1)):
        raise ValueError(f"resample_ragged: out must be a ({B}, >= {n_max}) float32 tensor on the batch's device")
    _launch(p, x, lens, None, True, out, n_max)
    return out, out_lens


class StreamResampler:
    """``push(x)`` / ``finish()`` over one signal per stream, all streams in step.  The concatenation of everything
    returned is bit-identical to ``resample_ragged`` on the whole signal however the samples were cut into pushes: every
    output is the same fma chain over the same samples, and a push returns exactly the ``final_outputs`` no later sample
    can change.  The last ``K`` inputs an unfinished output may still read stay on the device (f32).

    Delay: output m is final once input floor((m down + H) / up) has arrived, i.e. the stream runs ceil(H / up) input
    samples behind (109 at 48 k -> 16 k, 37 at 16 k -> 48 k, 100 at 44.1 k -> 16 k: 2.3 ms each)."""

    def __init__(self, streams, rate_in, rate_out, device):
        self.p = plan(rate_in, rate_out)
        self.S = int(streams)
        if self.S < 1:
            raise ValueError("StreamResampler: at least one stream")
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("StreamResampler runs on the GPU (there is no CPU fallback)")
        self.hist = torch.zeros(self.S, 0, dtype=torch.float32, device=self.dev)
        self.base = 0                    # absolute position of hist[:, 0]
        self.received = 0
        self.emitted = 0
        self.done = False

    def _emit(self, buf, count, ends):
        p = self.p
        if count <= 0:
            return torch.zeros(self.S, 0, dtype=torch.float32, device=self.dev)
        y = torch.empty(self.S, count, dtype=torch.float32, device=self.dev)
        lens = torch.full((self.S,), buf.shape[1], dtype=torch.int32, device=self.dev)
        origin = torch.tensor([[self.base, self.emitted]] * self.S, dtype=torch.int64).to(self.dev)
        _launch(p, buf, lens, origin, ends, y, count)
        self.emitted += count
        return y

    @torch.no_grad()
    def push(self, x):
        """x: (streams, n) int16 or f32, host or device, n >= 0.  Returns the (streams, m) outputs that became final,
        on x's device."""
        if self.done:
            raise RuntimeError("StreamResampler: finish() was called; make a new one for the next signal")
        if not torch.is_tensor(x) or x.dim() != 2 or x.shape[0] != self.S or x.dtype not in (torch.int16, torch.float32):
            raise ValueError(f"StreamResampler.push takes (streams, n) = ({self.S}, n) int16 or float32")
        p = self.p
        new = _as_f32(x.to(self.dev))
        self.received += x.shape[1]
        if p.identity:
            self.emitted = self.received
            return new.to(x.device)
        buf = torch.cat([self.hist, new], 1)
        count, keep = stream_step(self.received - x.shape[1], self.emitted, self.base, x.shape[1], p.up, p.down, p.H, p.K)
        out = self._emit(buf, count, False)
        self.hist = buf[:, keep - self.base:].clone()
        self.base = keep
        return out.to(x.device)

    @torch.no_grad()
    def finish(self, device=None):
        """The signal ends here: returns the remaining outputs, through ``out_length(total)``."""
        if self.done:
            raise RuntimeError("StreamResampler: finish() was already called")
        self.done = True
        p = self.p
        out = self._emit(self.hist, 0 if p.identity else out_length(self.received, p.up, p.down) - self.emitted, True)
        self.hist = None
        return out if device is None else out.to(device)
