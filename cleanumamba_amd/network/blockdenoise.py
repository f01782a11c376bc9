"""Denoise a recording of any length in blocks, with the Mamba state carried from block to block.

What the reference offers for long files is ``sampling(..., split_sampling=True)`` (src/util/util.py:185-212): ``net`` on
independent blocks -- every block normalised on its own, every block edge a restart of the encoder, of the Mamba state
and of the decoder's overlap.  Here a block is one WINDOW of the whole-signal ``forward``:

  * the per-clip std is the whole signal's, taken once;
  * bottleneck column tau reads samples [hop tau, hop tau + F) (hop = total_stride, F = frame_length).  A block owns the
    columns [tau0, tau1); its window is samples [hop (tau0 - c), hop (tau1 - 1) + F) of the zero-padded signal with
    c = 2 context columns (0 for the first block) -- itself a valid_length, so the unchanged fused conv stack runs on it.
    Convs without padding are exact wherever they are computed: every skip in the window is forward's;
  * the Mamba blocks run on the new columns only, from the conv / SSM states the previous block left (the entering-state
    scan and conv: csrc/scan_fwd.hip, scan_seg.hip, dwconv.hip); the previous block's last two norm_f outputs are put
    back in front for tsfm_conv2 and the decoder;
  * a transposed conv's output q needs input columns floor(q/2) and floor(q/2) - 1, so after the D decoder layers the
    window's output is exact from sample hop tau0 - 2 (hence two context columns) up to hop tau1 (the last F - hop
    samples lack the next column): the block emits [hop tau0, hop tau1), the last block through the padded length.

The result is ``forward`` on the whole signal to f32 rounding at the memory of one block (DESIGN.md "Block denoising").
"""
from collections import namedtuple

import torch

from . import convstack as cs
from ..mamba_ssm.utils.generation import InferenceParams

CONTEXT = 2                    # bottleneck columns of the previous block a window starts with
DEFAULT_BLOCK = 160000         # samples: the sequence length the kernels are tuned and benched at

Window = namedtuple("Window", "tau0 tau1 context win_lo win_hi emit_lo emit_hi")


def padded_length(L, F, hop):
    """``valid_length(L)`` in closed form: the smallest F + k hop >= L."""
    return F if L <= F else F + hop * (-(-(L - F) // hop))


def block_schedule(L, block_hops, F, hop):
    """The windows of an L-sample signal: blocks of ``block_hops`` columns, a lone last column joining the block before
    it (every block of a signal with more than one column has at least two).  Pure; sample positions refer to the
    zero-padded signal; the last emit range ends at the padded length."""
    if block_hops < 2:
        raise ValueError("block denoising needs at least 2 columns per block (block_hops >= 2)")
    T0 = padded_length(L, F, hop)
    ncol = (T0 - F) // hop + 1
    out, tau0 = [], 0
    while tau0 < ncol:
        tau1 = min(tau0 + block_hops, ncol)
        if ncol - tau1 == 1:
            tau1 = ncol
        c = 0 if tau0 == 0 else CONTEXT
        out.append(Window(tau0, tau1, c, hop * (tau0 - c), hop * (tau1 - 1) + F, hop * tau0,
                          hop * tau1 if tau1 < ncol else T0))
        tau0 = tau1
    return out


def default_block_hops(hop, block_size=DEFAULT_BLOCK):
    return max(2, int(round(block_size / hop)))


def check_model(model):
    """NotImplementedError with the reason for models the block route does not cover."""
    for layer in model.tsfm_Mamba_layers:
        if type(layer.mixer).__name__ == "Mamba2":
            raise NotImplementedError("block denoising: Mamba2 models are not covered -- the Mamba2 scan (cum_ssd_fwd) "
                                      "takes no entering state")
    if not cs.supported(model) or model.channels_output != 1 or not getattr(model, "use_fused_convs", True):
        raise NotImplementedError("block denoising runs on the fused conv stack: kernel 4 / stride 2 / ungrouped / "
                                  "sigmoid-GLU layers, one output channel")
    if not next(model.parameters()).is_cuda:
        raise NotImplementedError("block denoising: the model's weights are on the CPU; the kernels run on a ROCm GPU")


def host_clip_std(x, eps, piece=1 << 22):
    """cs.clip_std for a host-resident (B, L) signal: one pass over pieces, sums kept in f64.  (B, 1, 1) f32, host."""
    B, L = x.shape
    s = torch.zeros(B, dtype=torch.float64)
    q = torch.zeros(B, dtype=torch.float64)
    for i in range(0, L, piece):
        p = x[:, i:i + piece].double()
        s += p.sum(1)
        q += (p * p).sum(1)
    var = (q - s * s / L).clamp_(min=0) / (L - 1)
    return (var.sqrt() + eps).float().view(B, 1, 1)


class BlockDenoiser:
    """``push(x)`` / ``finish()`` over one signal per stream.  Owns its InferenceParams (the Mamba states), the context
    columns and the samples not yet consumed; the model's own stream state and stream pools are not touched.  Only
    whole blocks run, and a block runs only once the samples of the two columns behind it have arrived (so that it is
    not the one a lone last column would join): the output bits do not depend on how the samples were cut into pushes."""

    def __init__(self, model, streams, std=None, block_hops=None):
        check_model(model)
        self.model, self.S = model, int(streams)
        self.hop, self.F = model.total_stride, model.valid_length(1)
        self.block_hops = default_block_hops(self.hop) if block_hops is None else int(block_hops)
        if self.block_hops < 2:
            raise ValueError("block denoising needs at least 2 columns per block (block_hops >= 2)")
        self.dev = next(model.parameters()).device
        if model.normalize_input:
            if std is None:
                raise ValueError("block_denoiser: this model normalises its input -- give the per-clip std + eps of the "
                                 "WHOLE signal, (streams, 1), e.g. cs.clip_std(x, 1e-3)")
            self.std = std.to(self.dev, torch.float32).reshape(self.S, 1, 1).contiguous()
        else:
            self.std = None
        self.params = InferenceParams(max_seqlen=1, max_batch_size=self.S)
        self.context = 0             # context columns of the window being run (read by _forward_fused)
        self._ctx = None             # norm_f output of the previous block's last CONTEXT columns
        self.pending = torch.zeros(self.S, 0, dtype=torch.float32, device=self.dev)
        self.base = 0                # sample position of pending[:, 0]
        self.received = 0
        self.tau0 = 0                # first column of the next block
        self.done = False

    # -- called by CleanUMamba._forward_fused between norm_f and tsfm_conv2
    def join(self, hidden):
        full = hidden if self._ctx is None else torch.cat([self._ctx.to(hidden.dtype), hidden], 1)
        self._ctx = full[:, -CONTEXT:].clone()
        return full

    def _run(self, w, crop=None):
        hop = self.hop
        assert self.base == w.win_lo and self.tau0 == w.tau0
        Tw = w.win_hi - w.win_lo
        n = min(Tw, self.pending.shape[1])
        x = self.pending[:, :n].unsqueeze(1)
        m = self.model
        dt = m._fused_dtype()
        buf = cs.frame_input(x, self.std, Tw, dt)
        self.context = w.context
        with cs.small_m_gemms():
            obuf, geo, _, _ = m._forward_fused(buf, self.S, Tw, dt, carry=self)
        y = cs.Unframe.apply(obuf, self.std, geo, Tw)
        lo = w.emit_lo - w.win_lo
        hi = (w.emit_hi if crop is None else min(w.emit_hi, crop)) - w.win_lo
        out = y[:, 0, lo:max(hi, lo)]
        self.params.seqlen_offset += w.tau1 - w.tau0
        self.tau0 = w.tau1
        nb = max(hop * (w.tau1 - CONTEXT), self.base)        # where the next window starts
        self.pending = self.pending[:, min(nb - self.base, self.pending.shape[1]):].clone()
        self.base = nb
        return out

    @torch.no_grad()
    def push(self, x):
        """x: (streams, n) f32, on the host or on the GPU.  Returns the (streams, m) samples that became final."""
        if self.done:
            raise RuntimeError("BlockDenoiser: finish() was called; make a new one for the next signal")
        if x.dim() != 2 or x.shape[0] != self.S:
            raise ValueError(f"BlockDenoiser.push takes (streams, n) = ({self.S}, n)")
        self.pending = torch.cat([self.pending, x.to(self.dev, torch.float32)], 1)
        self.received += x.shape[1]
        outs, hop, bh = [], self.hop, self.block_hops
        while self.received >= hop * (self.tau0 + bh + 1) + self.F:
            t0, t1 = self.tau0, self.tau0 + bh
            c = 0 if t0 == 0 else CONTEXT
            outs.append(self._run(Window(t0, t1, c, hop * (t0 - c), hop * (t1 - 1) + self.F, hop * t0, hop * t1)))
        out = torch.cat(outs, 1) if outs else torch.zeros(self.S, 0, dtype=torch.float32, device=self.dev)
        return out.to(x.device)

    @torch.no_grad()
    def finish(self, device=None):
        """Zero-pads to valid_length as ``forward`` does, runs what is left and returns the remaining samples: through
        the signal's length with ``normalize_input``, through the padded length without."""
        if self.done:
            raise RuntimeError("BlockDenoiser: finish() was already called")
        self.done = True
        L = self.received
        if L == 0:
            return torch.zeros(self.S, 0, dtype=torch.float32, device=device or self.dev)
        crop = L if self.model.normalize_input else None
        outs = [self._run(w, crop) for w in block_schedule(L, self.block_hops, self.F, self.hop) if w.tau0 >= self.tau0]
        out = torch.cat(outs, 1)
        return out if device is None else out.to(device)


def _denoise_long_at_rate(model, noisy, bh, rate, model_rate):
    """``denoise_long`` for a (B, L) signal at ``rate``: the chain StreamResampler -> BlockDenoiser.push ->
    StreamResampler, a piece at a time, so device memory does not depend on L.  The std the block denoiser needs is
    that of the WHOLE converted signal: a first conversion pass accumulates its sum and sum of squares in f64 (as
    ``host_clip_std`` does) and discards the samples.  -> (B, 1, L) at ``rate``, on noisy's device: the converted-back
    signal cropped to L (a round trip never shortens a signal)."""
    from ..util.resample import StreamResampler, out_length, plan
    p = plan(rate, model_rate)
    plan(model_rate, rate)
    B, L = noisy.shape
    dev = next(model.parameters()).device
    hop = model.total_stride
    step = max(1, out_length(bh * hop, p.down, p.up))        # input samples of about one block
    std = None
    if model.normalize_input:
        n = out_length(L, p.up, p.down)
        s = torch.zeros(B, dtype=torch.float64, device=dev)
        q = torch.zeros(B, dtype=torch.float64, device=dev)
        first = StreamResampler(B, rate, model_rate, dev)
        for i in range(0, L, step):
            y = first.push(noisy[:, i:i + step].to(dev)).double()
            s += y.sum(1)
            q += (y * y).sum(1)
        y = first.finish().double()
        s += y.sum(1)
        q += (y * y).sum(1)
        var = (q - s * s / n).clamp_(min=0) / (n - 1)          # one converted sample: nan, as torch.std
        std = (var.sqrt() + 1e-3).float().view(B, 1)
    to_model = StreamResampler(B, rate, model_rate, dev)
    den = BlockDenoiser(model, B, std=std, block_hops=bh)
    back = StreamResampler(B, model_rate, rate, dev)
    out = torch.empty(B, 1, L, dtype=torch.float32, device=noisy.device)
    pos = 0

    def emit(y):
        nonlocal pos
        m = min(y.shape[1], L - pos)
        out[:, 0, pos:pos + m] = y[:, :m]
        pos += m
    for i in range(0, L, step):
        emit(back.push(den.push(to_model.push(noisy[:, i:i + step].to(dev)))))
    emit(back.push(den.push(to_model.finish())))
    emit(back.push(den.finish()))
    emit(back.finish())
    assert pos == L
    return out


@torch.no_grad()
def denoise_long(model, noisy, block_size=DEFAULT_BLOCK, block_hops=None, rate=None, model_rate=16000):
    """What ``model(noisy)`` returns -- (B, 1, L) with ``normalize_input``, (B, 1, valid_length(L)) without -- computed
    block by block.  noisy: (B, L) or (B, 1, L), on the GPU or on the host; host input is copied in and out a block at a
    time and gives host output, so device memory does not depend on L.  ``block_size`` (samples) is rounded down to
    whole hops; ``block_hops`` gives the columns per block directly.  ``rate``: the signal's sample rate; one other than
    ``model_rate`` converts the signal to the model's rate and back as a stream (``_denoise_long_at_rate``: (B, 1, L))."""
    check_model(model)
    if noisy.dim() == 3:
        if noisy.shape[1] != 1:
            raise ValueError("denoise_long takes (B, L) or (B, 1, L)")
        noisy = noisy[:, 0]
    if noisy.dim() != 2:
        raise ValueError("denoise_long takes (B, L) or (B, 1, L)")
    B, L = noisy.shape
    hop, F = model.total_stride, model.valid_length(1)
    bh = int(block_hops) if block_hops is not None else int(block_size) // hop
    if bh < 2:
        raise ValueError("block denoising needs at least 2 columns per block: block_size >= 2 * total_stride")
    if rate is not None and rate != model_rate:
        return _denoise_long_at_rate(model, noisy.float(), bh, rate, model_rate)
    dev = next(model.parameters()).device
    host = not noisy.is_cuda
    noisy = noisy.float()
    std = None
    if model.normalize_input:
        if host and L >= 2:
            std = host_clip_std(noisy, 1e-3)
        else:
            std = cs.clip_std(noisy.to(dev).unsqueeze(1), 1e-3)
    den = BlockDenoiser(model, B, std=None if std is None else std.view(B, 1), block_hops=bh)
    Lout = L if model.normalize_input else padded_length(L, F, hop)
    out = torch.empty(B, 1, Lout, dtype=torch.float32, device=noisy.device)
    pos, step = 0, bh * hop
    for i in range(0, L, step):
        o = den.push(noisy[:, i:i + step])
        out[:, 0, pos:pos + o.shape[1]] = o
        pos += o.shape[1]
    o = den.finish(device=noisy.device)
    out[:, 0, pos:pos + o.shape[1]] = o
    assert pos + o.shape[1] == Lout or L == 0
    return out
