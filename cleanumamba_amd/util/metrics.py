"""Speech-quality metrics of a ragged batch of clips on the GPU (csrc/metrics.hip).

``speech_metrics(clean, processed)`` scores any number of clips of any lengths in one launch sequence: the per-clip
``wss_dist``, ``llr_mean`` and ``segSNR`` of the reference's ``python_eval.eval_waveform`` and STOI (``pystoi.stoi``,
Taal et al. 2011).  Samples are int16 values, as the reference scores them; float inputs must hold integers in the int16
range.  Nothing here runs a metric on the CPU: the kernels are the only implementation.

``EXT_METRICS`` names five more per-clip numbers that ``speech_metrics(..., metrics=...)`` computes on request, in the
same batched way: ``estoi`` (extended STOI, Jensen & Taal 2016), ``si_sdr`` (Le Roux et al. 2019, no mean removal),
``snr`` (overall SNR), ``cep_dist`` and ``fwsegSNR`` (LPC cepstrum distance and frequency-weighted segmental SNR as in
Hu & Loizou 2008).  tests/metrics_ext_ref.py states their definitions in f64 numpy.  They are restatements of the
published algorithms: pystoi, pysepm and torchmetrics are not installed where this was written, and NOTHING here has been
compared with them.  Known deviation: pystoi adds eps-sized random noise before each eSTOI normalisation; here every norm
gets an additive eps instead, which keeps the result reproducible.  ``si_sdr`` and ``snr`` come from three exact int64
sums per clip (GPU); the few scalar operations on them run on the host in Python integers, because Sxx Syy - Sxy^2
cancels catastrophically in f64 (it can come out negative for y = 3x).

The constant tables are built here on the host:
  * the 25 critical bands of Klatt's weighted spectral slope measure, as published with the composite measures of Hu &
    Loizou, "Evaluation of objective quality measures for speech enhancement", IEEE TASLP 16(1), 2008: centre
    frequencies and bandwidths in Hz, Gaussian filters of 1024-point FFT bins truncated at -30 dB, kept sparse;
  * the 15 one-third-octave bands of STOI from 150 Hz over a 512-point FFT at 10 kHz, and the 16 k -> 10 k polyphase
    filter (Kaiser-windowed sinc, 60 dB rejection) of STOI's Octave-compatible resampler.
"""
import copy
import ctypes
import math

import numpy as np
import torch

from .. import hip

FRAME_RATE = 16000
WIN, HOP = 480, 120                  # 30 ms frames, 75 % overlap
STOI_RATES = (16000, 10000)
ALPHA = 0.95                         # fraction of the lowest frame values kept by the WSS / LLR means

# Klatt's critical bands (Hu & Loizou 2008): centre frequency and bandwidth, Hz
CRIT_CENTRE = (50.0000, 120.000, 190.000, 260.000, 330.000, 400.000, 470.000, 540.000, 617.372, 703.378, 798.717,
               904.128, 1020.38, 1148.30, 1288.72, 1442.54, 1610.70, 1794.16, 1993.93, 2211.08, 2446.71, 2701.97,
               2978.04, 3276.17, 3597.63)
CRIT_BANDWIDTH = (70.0000, 70.0000, 70.0000, 70.0000, 70.0000, 70.0000, 70.0000, 77.3724, 86.0056, 95.3398, 105.411,
                  116.256, 127.914, 140.423, 153.823, 168.154, 183.457, 199.776, 217.153, 235.631, 255.255, 276.072,
                  298.126, 321.465, 346.136)


def frame_window():
    """The 480-point Hann-type window of the frame metrics: 0.5 (1 - cos(2 pi n / 481)), n = 1..480."""
    return 0.5 * (1 - np.cos(2 * math.pi * np.arange(1, WIN + 1) / (WIN + 1)))


def crit_band_table(rate=FRAME_RATE):
    """Sparse critical-band filters over bins 0..511 of the 1024-point FFT: ``(tab, weights)`` with tab[b] = (first bin,
    bin count, offset into weights).  Each band is exp(-11 ((j - floor(f0)) / bw)^2) scaled by bw_min / bw, its values
    at or below the -30 dB point dropped; the support is one run of bins."""
    n_fft = int(2 ** math.ceil(math.log2(2 * WIN)))
    half, nyq = n_fft // 2, rate // 2
    min_factor = math.exp(-30.0 / (2.0 * 2.303))
    j = np.arange(half)
    tab, weights = [], []
    for cf, bwh in zip(CRIT_CENTRE, CRIT_BANDWIDTH):
        f0, bw = cf / nyq * half, bwh / nyq * half
        w = np.exp(-11 * np.square((j - np.floor(f0)) / bw) + (np.log(CRIT_BANDWIDTH[0]) - np.log(bwh)))
        keep = np.nonzero(w > min_factor)[0]
        lo, hi = int(keep[0]), int(keep[-1]) + 1
        assert hi - lo == keep.size
        tab.append((lo, hi - lo, sum(len(x) for x in weights)))
        weights.append(w[lo:hi])
    return np.array(tab, np.int32), np.concatenate(weights)


def third_octave_table(fs=10000, nfft=512, num_bands=15, min_freq=150):
    """[first, end) FFT bin of each one-third-octave band: the bins nearest to min_freq 2^((2k -+ 1) / 6)."""
    f = np.linspace(0, fs, nfft + 1)[: nfft // 2 + 1]
    k = np.arange(num_bands, dtype=float)
    lo = min_freq * np.power(2.0, (2 * k - 1) / 6)
    hi = min_freq * np.power(2.0, (2 * k + 1) / 6)
    return np.array([(int(np.argmin(np.square(f - a))), int(np.argmin(np.square(f - b)))) for a, b in zip(lo, hi)],
                    np.int32)


def resample_taps(p=10000, q=16000):
    """STOI's anti-aliasing filter for p / q resampling (Kaiser-windowed sinc, 60 dB rejection, transition a tenth of
    the cut-off), normalised to unit sum and scaled by the reduced up factor, as the polyphase resampler applies it."""
    g = math.gcd(p, q)
    up, down = p // g, q // g
    stop = 1.0 / (2 * max(up, down))
    rej = 60.0
    L = math.ceil((rej - 8) / (28.714 * stop / 10))
    t = np.arange(-L, L + 1)
    ideal = 2 * up * stop * np.sinc(2 * stop * t)
    beta = 0.1102 * (rej - 8.7)
    h = np.kaiser(2 * L + 1, beta) * ideal
    return h / np.sum(h) * up


def stoi_window():
    """hanning(258)[1:-1]: the 256-point window of STOI's frames."""
    return np.hanning(258)[1:-1]


def _twiddle(n_fft):
    k = np.arange(n_fft // 2 + 1, dtype=np.float64)
    ang = -2.0 * math.pi * k / n_fft
    return np.stack([np.cos(ang), np.sin(ang)], 1)


_TABLES = {}


def _tables(device):
    if device not in _TABLES:
        tab, w = crit_band_table()
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        _TABLES[device] = dict(window=put(frame_window()), band_tab=put(tab), band_w=put(w), tw1024=put(_twiddle(1024)),
                               taps=put(resample_taps()), stoi_win=put(stoi_window()), tw512=put(_twiddle(512)),
                               bands=put(third_octave_table()))
    return _TABLES[device]


def _as_int16(x, what):
    """One clip as a 1-D int16 tensor (same device); floats must hold integers in [-32768, 32767]."""
    t = x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    t = t.reshape(-1)
    if t.dtype == torch.int16:
        return t
    if t.dtype.is_floating_point:
        bad = ~torch.isfinite(t) | (t != torch.round(t))
    else:
        bad = torch.zeros_like(t, dtype=torch.bool)
    bad |= (t < -32768) | (t > 32767)
    if bool(bad.any()):
        raise ValueError(f"{what}: samples must be int16 values")
    return t.to(torch.int16)


class Batch:
    """A checked ragged batch: flat int16 buffers of both signals on the GPU and host offsets / lengths."""

    def __init__(self, clean, processed, rate, min_len=WIN):
        if isinstance(clean, (np.ndarray, torch.Tensor)) and clean.ndim == 1:
            clean, processed = [clean], [processed]
        clean, processed = list(clean), list(processed)
        if len(clean) == 0:
            raise ValueError("speech metrics: empty batch")
        if len(clean) != len(processed):
            raise ValueError("speech metrics: %d clean clips but %d processed" % (len(clean), len(processed)))
        cs = [_as_int16(c, "clean") for c in clean]
        ps = [_as_int16(p, "processed") for p in processed]
        lengths = []
        for i, (c, p) in enumerate(zip(cs, ps)):
            if c.numel() != p.numel():
                raise ValueError("speech metrics: clip %d: clean has %d samples, processed %d" % (i, c.numel(), p.numel()))
            if c.numel() < min_len:
                raise ValueError("speech metrics: clip %d has %d samples, fewer than one %d-sample window"
                                 % (i, c.numel(), min_len))
            lengths.append(c.numel())
        if len(cs) > 65535:
            raise ValueError("speech metrics: at most 65535 clips per batch")
        self.rate = rate
        self.lengths = np.array(lengths, np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.lengths)[:-1]]).astype(np.int64)
        self.n_clips = len(cs)
        self._cs, self._ps = cs, ps

    @classmethod
    def from_flat(cls, clean_flat, processed_flat, lengths, rate, offsets=None, min_len=WIN):
        """A batch over audio that is already on the device: two flat int16 tensors sharing ONE offsets / lengths table
        (clip i at [offsets[i], offsets[i] + lengths[i]) of both; ``offsets`` None: packed back to back).  Offsets may
        leave gaps (cropped clips stay where they are).  The checks of the constructor apply -- an empty batch, a clip
        under ``min_len`` samples, more than 65535 clips -- and nothing is copied."""
        lengths = np.ascontiguousarray(np.asarray(lengths, np.int64).reshape(-1))
        if lengths.size == 0:
            raise ValueError("speech metrics: empty batch")
        if lengths.size > 65535:
            raise ValueError("speech metrics: at most 65535 clips per batch")
        for i, n in enumerate(lengths.tolist()):
            if n < min_len:
                raise ValueError("speech metrics: clip %d has %d samples, fewer than one %d-sample window" % (i, n, min_len))
        offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64) if offsets is None else \
            np.ascontiguousarray(np.asarray(offsets, np.int64).reshape(-1))
        if offsets.size != lengths.size:
            raise ValueError("speech metrics: %d offsets for %d lengths" % (offsets.size, lengths.size))
        for name, t in (("clean", clean_flat), ("processed", processed_flat)):
            if t.dtype != torch.int16 or t.dim() != 1 or not t.is_contiguous():
                raise ValueError("speech metrics: the flat %s buffer must be a contiguous 1-D int16 tensor" % name)
            if not t.is_cuda:
                raise RuntimeError("speech metrics run only on a ROCm GPU; there is no CPU fallback")
        if clean_flat.device != processed_flat.device or clean_flat.numel() != processed_flat.numel():
            raise ValueError("speech metrics: the flat buffers must have one device and one size")
        if int(offsets.min()) < 0 or int((offsets + lengths).max()) > clean_flat.numel():
            raise ValueError("speech metrics: a clip reaches outside the flat buffers")
        b = cls.__new__(cls)
        b.rate, b.lengths, b.offsets, b.n_clips = rate, lengths, offsets, int(lengths.size)
        b.device, b.clean, b.processed = clean_flat.device, clean_flat, processed_flat
        b._cs = b._ps = None
        return b

    def at_rate(self, rate):
        """The same buffers and tables declared at another rate (no copy, no upload)."""
        b = copy.copy(self)
        b.rate = rate
        return b

    def upload(self):
        if self._cs is None:                     # from_flat: already resident
            return self
        if not torch.cuda.is_available():
            raise RuntimeError("speech metrics run only on a ROCm GPU; there is no CPU fallback")
        dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.clean = torch.cat([c.to(dev) for c in self._cs])
        self.processed = torch.cat([p.to(dev) for p in self._ps])
        return self

    @staticmethod
    def hp(a):
        """a host int64 array as a pointer argument"""
        return a.ctypes.data_as(ctypes.c_void_p)


def frame_counts(lengths):
    return np.maximum((np.asarray(lengths, np.int64) - WIN) // HOP, 0)


def _check_rate(rate, want):
    if rate not in want:
        raise ValueError("speech metrics: rate %r Hz is not supported (%s)" % (rate, ", ".join(map(str, want))))


def _frames(b):
    """Per-frame segSNR, LLR and WSS of an uploaded batch (f64, clip i at frame_off[i]) and the frame offsets."""
    L = hip.lib()
    t = _tables(b.device)
    nf = frame_counts(b.lengths)
    total = int(nf.sum())
    out = torch.empty((3, max(total, 1)), dtype=torch.float64, device=b.device)
    ws = torch.empty(L.cum_metrics_workspace_bytes(b.n_clips, total), dtype=torch.uint8, device=b.device)
    hip.check(L.cum_metrics_frames(hip.ptr(b.clean), hip.ptr(b.processed), b.clean.numel(), b.hp(b.offsets),
                                   b.hp(b.lengths), b.n_clips, b.rate, hip.ptr(t["window"]), hip.ptr(t["band_tab"]),
                                   hip.ptr(t["band_w"]), hip.ptr(t["tw1024"]), hip.ptr(ws), ws.numel(),
                                   hip.ptr(out[0]), hip.ptr(out[1]), hip.ptr(out[2]), total, hip.stream_ptr()))
    return out[:, :total], np.concatenate([[0], np.cumsum(nf)]), ws


def _reduce(b, values, mode, ws):
    out = torch.empty(b.n_clips, dtype=torch.float64, device=b.device)
    hip.check(hip.lib().cum_metrics_clip_reduce(hip.ptr(values), b.hp(b.lengths), b.n_clips, mode, hip.ptr(ws),
                                                ws.numel(), hip.ptr(out), hip.stream_ptr()))
    return out


def _frames_ext(b):
    """Per-frame cepstrum distance and fwseg of an uploaded batch ((2, total) f64) and the workspace."""
    L = hip.lib()
    t = _tables(b.device)
    nf = frame_counts(b.lengths)
    total = int(nf.sum())
    out = torch.empty((2, max(total, 1)), dtype=torch.float64, device=b.device)
    ws = torch.empty(L.cum_metrics_workspace_bytes(b.n_clips, total), dtype=torch.uint8, device=b.device)
    hip.check(L.cum_metrics_frames_ext(hip.ptr(b.clean), hip.ptr(b.processed), b.clean.numel(), b.hp(b.offsets),
                                       b.hp(b.lengths), b.n_clips, b.rate, hip.ptr(t["window"]), hip.ptr(t["band_tab"]),
                                       hip.ptr(t["band_w"]), hip.ptr(t["tw1024"]), hip.ptr(ws), ws.numel(),
                                       hip.ptr(out[0]), hip.ptr(out[1]), total, hip.stream_ptr()))
    return out[:, :total], np.concatenate([[0], np.cumsum(nf)]), ws


def _nanmean(b, values, ws):
    out = torch.empty(b.n_clips, dtype=torch.float64, device=b.device)
    hip.check(hip.lib().cum_metrics_clip_nanmean(hip.ptr(values), b.hp(b.lengths), b.n_clips, hip.ptr(ws), ws.numel(),
                                                 hip.ptr(out), hip.stream_ptr()))
    return out


def clip_sums(b):
    """Exact (sum x^2, sum y^2, sum x y) of every clip of an uploaded batch: an (n_clips, 3) int64 tensor on the GPU."""
    L = hip.lib()
    ws = torch.empty(L.cum_metrics_sums_workspace_bytes(b.hp(b.lengths), b.n_clips), dtype=torch.uint8, device=b.device)
    out = torch.empty((b.n_clips, 3), dtype=torch.int64, device=b.device)
    hip.check(L.cum_metrics_sums(hip.ptr(b.clean), hip.ptr(b.processed), b.clean.numel(), b.hp(b.offsets),
                                 b.hp(b.lengths), b.n_clips, hip.ptr(ws), ws.numel(), hip.ptr(out), hip.stream_ptr()))
    return out


def _db(num, den):
    """10 log10(num / den) of two positive Python integers, the quotient correctly rounded."""
    return 10.0 * math.log10(num / den)


def snr_from_sums(sxx, syy, sxy):
    """Overall SNR 10 log10(sum x^2 / sum (x - y)^2) from the exact integer sums: NaN for a silent clean clip, +inf for
    y = x."""
    d = sxx - 2 * sxy + syy
    if sxx == 0:
        return float("nan")
    return float("inf") if d == 0 else _db(sxx, d)


def si_sdr_from_sums(sxx, syy, sxy):
    """SI-SDR (Le Roux et al. 2019, no mean removal) 10 log10(Sxy^2 / (Sxx Syy - Sxy^2)) in exact integers: NaN for a
    silent clean clip, -inf for Sxy = 0 (a silent or orthogonal processed clip), +inf for y = a x."""
    if sxx == 0:
        return float("nan")
    if sxy == 0:
        return float("-inf")
    q = sxx * syy - sxy * sxy
    return float("inf") if q == 0 else _db(sxy * sxy, q)


def _stoi(b, which=1):
    """(STOI, eSTOI) of an uploaded batch; ``which``: 1 STOI (cum_metrics_stoi, as ever), 2 eSTOI, 3 both on one front
    end (cum_metrics_stoi_ex); what was not asked for is None."""
    L = hip.lib()
    t = _tables(b.device)
    nbytes = L.cum_metrics_stoi_workspace_bytes(b.hp(b.lengths), b.n_clips, b.rate)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=b.device)
    out = [torch.empty(b.n_clips, dtype=torch.float64, device=b.device) if which & m else None for m in (1, 2)]
    head = (hip.ptr(b.clean), hip.ptr(b.processed), b.clean.numel(), b.hp(b.offsets), b.hp(b.lengths), b.n_clips, b.rate,
            hip.ptr(t["taps"]), t["taps"].numel(), hip.ptr(t["stoi_win"]), hip.ptr(t["tw512"]), hip.ptr(t["bands"]),
            hip.ptr(ws), ws.numel())
    if which == 1:
        hip.check(L.cum_metrics_stoi(*head, hip.ptr(out[0]), hip.stream_ptr()))
    else:
        hip.check(L.cum_metrics_stoi_ex(*head, which, hip.ptr(out[0]) if which & 1 else None, hip.ptr(out[1]),
                                        hip.stream_ptr()))
    return out


METRICS = ("wss_dist", "llr_mean", "segSNR", "stoi")
EXT_METRICS = ("estoi", "si_sdr", "snr", "cep_dist", "fwsegSNR")      # on request only: no default changes
_FRAME_NAMES = ("wss_dist", "llr_mean", "segSNR")
_EXT_FRAME_NAMES = ("cep_dist", "fwsegSNR")
_STOI_NAMES = ("stoi", "estoi")


def frame_metrics(clean, processed, rate=FRAME_RATE, extended=False):
    """Per-frame ``segSNR``, ``llr`` and ``wss`` of every clip: a dict of lists of f64 tensors, one per clip.  With
    ``extended`` also ``cep`` (LPC cepstrum distance, [0, 10], NaN where either frame is all zeros) and ``fwseg``
    (frequency-weighted segmental SNR, [-10, 35] dB, NaN where the clean frame is silent)."""
    _check_rate(rate, (FRAME_RATE,))
    b = Batch(clean, processed, rate).upload()
    out, off, _ = _frames(b)
    split = lambda v: [v[off[i]:off[i + 1]] for i in range(b.n_clips)]
    res = {"segSNR": split(out[0]), "llr": split(out[1]), "wss": split(out[2])}
    if extended:
        ext, _, _ = _frames_ext(b)
        res["cep"], res["fwseg"] = split(ext[0]), split(ext[1])
    return res


def speech_metrics(clean, processed=None, rate=FRAME_RATE, metrics=METRICS):
    """Per-clip metrics of a ragged batch: a dict name -> f64 tensor of one value per clip, for each name in ``metrics``
    (``wss_dist``, ``llr_mean``, ``segSNR``: eval_waveform's recipe at 16 kHz; ``stoi`` at 16 or 10 kHz), in the order
    asked.  Names of ``EXT_METRICS`` are accepted too: ``cep_dist`` (mean of the lowest 95 % of the frame values, NaN
    dropped) and ``fwsegSNR`` (mean of the non-NaN frames) at 16 kHz, ``estoi`` at 16 or 10 kHz, ``si_sdr`` and ``snr`` at
    any positive rate; ``stoi`` and ``estoi`` asked together share one front end.

    ``clean`` / ``processed``: lists of 1-D arrays or tensors of int16 values, pairwise of equal length, each at least
    480 samples.  Raises ValueError before any launch for an empty batch, unequal lengths, a short clip or a rate the
    requested metrics do not support.

    ``clean`` may be a ready ``Batch`` (``Batch.from_flat``: audio already on the device) with ``processed`` None: it is
    scored at ``rate`` as it stands, with no copy and no upload; a caller that needs several rate classes passes the same
    batch again with the other rate."""
    metrics = tuple(metrics)
    for m in metrics:
        if m not in METRICS + EXT_METRICS:
            raise ValueError("speech metrics: unknown metric %r (have %s)" % (m, ", ".join(METRICS + EXT_METRICS)))
    frame_names = [m for m in metrics if m in _FRAME_NAMES]
    ext_names = [m for m in metrics if m in _EXT_FRAME_NAMES]
    stoi_names = [m for m in metrics if m in _STOI_NAMES]
    if frame_names or ext_names:
        _check_rate(rate, (FRAME_RATE,))
    elif stoi_names:
        _check_rate(rate, STOI_RATES)
    elif not (isinstance(rate, (int, np.integer)) and rate > 0):      # si_sdr, snr: the rate is not used
        raise ValueError("speech metrics: rate %r Hz is not supported (any positive rate)" % (rate,))
    if isinstance(clean, Batch):
        if processed is not None:
            raise ValueError("speech metrics: a ready Batch holds both signals; processed must be None")
        b = clean.at_rate(rate).upload()
    else:
        b = Batch(clean, processed, rate).upload()
    res = {}
    if ext_names:
        vals, _, ws = _frames_ext(b)
        if "cep_dist" in metrics:
            res["cep_dist"] = _reduce(b, vals[0], 2, ws)
        if "fwsegSNR" in metrics:
            res["fwsegSNR"] = _nanmean(b, vals[1], ws)
    if "si_sdr" in metrics or "snr" in metrics:
        sums = [tuple(int(v) for v in row) for row in clip_sums(b).cpu().tolist()]
        for name, fn in (("si_sdr", si_sdr_from_sums), ("snr", snr_from_sums)):
            if name in metrics:
                res[name] = torch.tensor([fn(*s) for s in sums], dtype=torch.float64, device=b.device)
    if frame_names:
        vals, _, ws = _frames(b)
        if "segSNR" in metrics:
            res["segSNR"] = _reduce(b, vals[0], 0, ws)
        if "llr_mean" in metrics:
            res["llr_mean"] = _reduce(b, vals[1], 2, ws)
        if "wss_dist" in metrics:
            res["wss_dist"] = _reduce(b, vals[2], 1, ws)
    if stoi_names:
        st, est = _stoi(b, ("stoi" in metrics) | 2 * ("estoi" in metrics))
        if st is not None:
            res["stoi"] = st
        if est is not None:
            res["estoi"] = est
    return {m: res[m] for m in metrics}


def stoi(clean, processed, fs, extended=False):
    """STOI of one clip, ``pystoi.stoi(x, y, fs_sig, extended=False)``'s signature; fs 16000 or 10000.  ``extended``
    gives eSTOI (Jensen & Taal 2016; an additive eps where pystoi adds eps-sized noise)."""
    _check_rate(fs, STOI_RATES)
    b = Batch([clean], [processed], fs, min_len=1).upload()
    return float(_stoi(b, 2 if extended else 1)[1 if extended else 0][0])
