"""Speech and noise from two unpaired corpora mixed into the train step's (clean, noisy) pair: what the DNS challenge's
synthesiser does offline, once, over the whole corpus, done per batch on the device.  The reference's loop assumes the
pre-mixed set (src/util/dataset.py:108-150), so the arithmetic is defined here (and in include/cleanumamba_hip.h:
cum_mix_pairs).  It follows the synthesiser's scheme -- SNR against the ACTIVE level of speech and noise, a
target level in dBFS, a guard against clipping -- and has not been compared with its output.

Two halves, kept apart as in training/augment.py:

  Mix.draw(rng, nb)        pure host code: the SNR and the level of every row of one batch, as a ``MixDraws``;
  apply(speech_i16, n_speech, noise_i16, draws)
                           the arithmetic, with nothing random in it: csrc/mix.hip (cum_mix_pairs) on device tensors,
                           a NumPy restatement on CPU tensors.

Row b of a batch of ``len`` samples, x an int16 value:  S[t] = speech[b][t mod n_s] (n_s = n_speech[b] clamped into
[1, len]: a short file fills the row by repetition),  N[t] = noise[b][t].

  1. frames [k frame, min((k + 1) frame, len));  es_k = sum S^2, en_k = sum N^2 per frame, Ss = sum S^2, Snn = sum N^2,
     Ssn = sum S N over the row, exact in int64;  a frame of m samples is active iff e_k > thr m,
     thr = floor(2^30 10^(activity_db / 10))
  2. Ps = (sum es_k over active frames) / (sum m over active frames) in f64, or Ss / len if no frame is active; Pn likewise
  3. a = sqrt(Ps / (Pn q)), q = 10^(snr_db / 10), if Ps > 0, Pn > 0 and q is finite and positive, else 1;  a32 = (float) a
  4. Em = (A Snn + 2 Ssn) A + Ss with A = (double) a32, in f64
  5. g = sqrt(l len 2^30 / Em), l = 10^(level_db / 10), if l is finite and Em > 0, else 1;  g32 = (float) g
  6. m[t] = fmaf(a32, N[t] 2^-15, S[t] 2^-15) in f32;  peak = max |m[t]|
  7. if g32 peak > clip: g32 = clip / peak
  8. clean[t] = g32 (S[t] 2^-15),  noisy[t] = g32 m[t]

and the row's stats are {a32, g32, Ps 2^-30, Pn 2^-30, peak, active share of speech, active share of noise (the samples
of the active frames over len), 1.0 if the guard acted else 0.0}.  ``BatchFeeder(SpeechNoiseDataset(...), ...,
mix=Mix(...))`` (training/feeder.py) draws per batch and runs this in place of the assembling kernel.
"""
import math

import numpy as np
import torch

from .. import hip
from .augment import _rows, _span

REC_INTS = 12                    # one record per row: the fields below, then zeros
REC_N_SPEECH, REC_FRAME, REC_THR, REC_Q, REC_L, REC_CLIP = 0, 1, 2, 4, 6, 8
STATS = 8                        # floats per row of the stats
PCM_SCALE = 1.0 / 32768.0


def _range(value, name, none_ok=False):
    """(lo, hi) of a pair or a single number."""
    if value is None:
        if none_ok:
            return None
        raise ValueError(f"Mix: {name} must be a number or a (lo, hi) pair")
    try:
        lo, hi = (float(v) for v in value)
    except TypeError:
        lo = hi = float(value)
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise ValueError(f"Mix: {name} must be finite with lo <= hi; got {value!r}")
    return lo, hi


def _check_config(who, activity_db, frame, clip):
    if not math.isfinite(activity_db):
        raise ValueError(f"{who}: activity_db must be finite")
    if frame < 1:
        raise ValueError(f"{who}: frame must be at least 1")
    if not 0 < clip <= 1:            # (NaN fails both)
        raise ValueError(f"{who}: clip must lie in (0, 1]")


class MixDraws:
    """Everything random about the mixing of one batch of ``nb`` rows, and the settings the kernel reads with it:
    float64 ``snr_db`` and ``level_db`` (nb,) (level NaN: keep the mixture's level); ``activity_db``, ``frame``, ``clip``
    as in ``Mix``."""

    def __init__(self, snr_db, level_db, activity_db=-50.0, frame=1600, clip=0.99):
        self.snr_db = np.ascontiguousarray(snr_db, dtype=np.float64)
        self.level_db = np.ascontiguousarray(level_db, dtype=np.float64)
        self.activity_db, self.frame, self.clip = float(activity_db), int(frame), float(clip)
        if self.snr_db.ndim != 1 or self.snr_db.shape[0] < 1 or self.level_db.shape != self.snr_db.shape:
            raise ValueError("MixDraws: snr_db and level_db must both be (nb,) with at least one row")
        if not np.isfinite(self.snr_db).all():
            raise ValueError("MixDraws: snr_db must be finite")
        if np.isinf(self.level_db).any():
            raise ValueError("MixDraws: level_db must be finite or NaN (keep)")
        _check_config("MixDraws", self.activity_db, self.frame, self.clip)

    @property
    def batch(self):
        return self.snr_db.shape[0]

    @property
    def thr(self):
        """floor(2^30 10^(activity_db / 10)): a frame is active iff its sum of squares exceeds thr times its samples."""
        return int(math.floor(2.0 ** 30 * 10.0 ** (self.activity_db / 10.0)))

    def q(self, b):
        return 10.0 ** (float(self.snr_db[b]) / 10.0)

    def l(self, b):
        level = float(self.level_db[b])
        return 10.0 ** (level / 10.0) if math.isfinite(level) else math.nan

    def pack(self, n_speech):
        """The record table of include/cleanumamba_hip.h (cum_mix_pairs) as one int32 array: nb records of 12."""
        nb = self.batch
        n_speech = np.asarray(n_speech, dtype=np.int64).reshape(-1)
        if n_speech.shape != (nb,) or n_speech.min() < 1 or n_speech.max() > 0x7fffffff:
            raise ValueError(f"MixDraws.pack: n_speech must be ({nb},) of values in [1, 2^31)")
        out = np.zeros((nb, REC_INTS), dtype=np.int32)
        out[:, REC_N_SPEECH], out[:, REC_FRAME] = n_speech, min(self.frame, 0x7fffffff)
        out[:, REC_THR:REC_THR + 2].view(np.int64)[:, 0] = self.thr
        out[:, REC_Q:REC_Q + 2].view(np.float64)[:, 0] = [self.q(b) for b in range(nb)]
        out[:, REC_L:REC_L + 2].view(np.float64)[:, 0] = [self.l(b) for b in range(nb)]
        out[:, REC_CLIP] = np.full(nb, self.clip, dtype=np.float32).view(np.int32)
        return out.reshape(-1)


class Mix:
    """``Mix(snr_db=(-5.0, 20.0), level_db=(-35.0, -15.0), activity_db=-50.0, frame=1600, clip=0.99, gap=3200,
    max_pieces=8)``

    snr_db: the SNR of a row, uniform in the range (a pair, or one number), measured on the active frames.
    level_db: the level of the mixture in dBFS, uniform in the range; None keeps the level the scaled noise gives.
    activity_db: a frame is active when its mean square is above this many dB of full scale.
    frame: samples per frame of the activity decision (1600: 100 ms at 16 kHz).
    clip: the largest magnitude the mixture may reach; the guard scales a row that would exceed it.
    gap: zero samples behind every piece of a noise row;  max_pieces: noise pieces per row at most (training/feeder.py)."""

    def __init__(self, snr_db=(-5.0, 20.0), level_db=(-35.0, -15.0), activity_db=-50.0, frame=1600, clip=0.99, gap=3200,
                 max_pieces=8):
        self.snr_db = _range(snr_db, "snr_db")
        self.level_db = _range(level_db, "level_db", none_ok=True)
        self.activity_db, self.frame, self.clip = float(activity_db), int(frame), float(clip)
        self.gap, self.max_pieces = int(gap), int(max_pieces)
        _check_config("Mix", self.activity_db, self.frame, self.clip)
        if self.gap < 0:
            raise ValueError("Mix: gap must be at least 0")
        if self.max_pieces < 1:
            raise ValueError("Mix: max_pieces must be at least 1")

    def draw(self, rng, nb):
        """The draws of one batch from ``rng`` (a numpy Generator): nb SNRs, then, with a level range, nb levels."""
        nb = int(nb)
        snr = rng.uniform(*self.snr_db, nb)
        level = rng.uniform(*self.level_db, nb) if self.level_db is not None else np.full(nb, np.nan)
        return MixDraws(snr, level, self.activity_db, self.frame, self.clip)


# ---------------------------------------------------------------------------------------------------------------- apply
def _frame_sums(x2, frame):
    """Per-frame sums of an int64 row (the last frame may be short) and the samples of every frame."""
    n = x2.shape[0]
    k = -(-n // frame)
    padded = np.zeros(k * frame, dtype=np.int64)
    padded[:n] = x2
    m = np.full(k, frame, dtype=np.int64)
    m[-1] = n - (k - 1) * frame
    return padded.reshape(k, frame).sum(axis=1), m


def _host_row(speech, noise, n_speech, length, thr, frame, q, l, clip):
    """(clean, noisy, stats) of one row: the arithmetic of the module's docstring in NumPy."""
    f32 = np.float32
    n_s, frame = min(max(int(n_speech), 1), length), min(max(int(frame), 1), length)
    thr = min(max(int(thr), 0), 1 << 30)
    S = speech[np.arange(length) % n_s].astype(np.int64)
    N = noise[:length].astype(np.int64)
    es, m = _frame_sums(S * S, frame)
    en, _ = _frame_sums(N * N, frame)
    Ss, Snn, Ssn = int(es.sum()), int(en.sum()), int((S * N).sum())
    act_s, act_n = es > thr * m, en > thr * m
    ms, mn = int(m[act_s].sum()), int(m[act_n].sum())
    Ps = float(int(es[act_s].sum())) / float(ms) if ms > 0 else float(Ss) / float(length)
    Pn = float(int(en[act_n].sum())) / float(mn) if mn > 0 else float(Snn) / float(length)
    a = 1.0
    if Ps > 0 and Pn > 0 and math.isfinite(q) and q > 0:
        a = float(np.sqrt(np.float64(Ps) / (np.float64(Pn) * np.float64(q))))
    a32 = f32(a)
    A = float(a32)
    Em = (A * float(Snn) + 2.0 * float(Ssn)) * A + float(Ss)
    g = 1.0
    if math.isfinite(l) and Em > 0:
        g = float(np.sqrt(np.float64(l) * float(length) * 1073741824.0 / np.float64(Em)))
    g32 = f32(g)
    s = (S.astype(np.float64) * PCM_SCALE)
    mixed = (np.float64(A) * (N.astype(np.float64) * PCM_SCALE) + s).astype(f32)      # fmaf: rounded once
    peak = f32(np.abs(mixed).max())
    guard = bool(g32 * peak > f32(clip))
    if guard:
        g32 = f32(clip) / peak
    stats = np.array([a32, g32, f32(Ps / 1073741824.0), f32(Pn / 1073741824.0), peak, f32(float(ms) / float(length)),
                      f32(float(mn) / float(length)), 1.0 if guard else 0.0], dtype=f32)
    return g32 * s.astype(f32), g32 * mixed, stats


def workspace_for(nb, length, device):
    """The workgroup totals' and tile peaks' room for a batch of nb rows of length samples (8-byte aligned: float64)."""
    return torch.empty(max(1, hip.lib().cum_mix_workspace_elems(nb, length) // 2), dtype=torch.float64, device=device)


def launch(pcm, pitch, recs, nb, length, workspace, clean, co, noisy, no, stats):
    """cum_mix_pairs on the current stream.  pcm: the device int16 block of 2 * nb rows; recs: the device int32 tensor of
    ``MixDraws.pack``; workspace: ``workspace_for``; stats: a device float32 tensor of nb rows of 8, or None."""
    hip.check(hip.lib().cum_mix_pairs(hip.ptr(pcm), pitch, hip.ptr(recs), nb, length, hip.ptr(workspace), hip.ptr(clean), co,
                                      hip.ptr(noisy), no, hip.ptr(stats), hip.stream_ptr()))


def apply(speech_i16, n_speech, noise_i16, draws, clean_out=None, noisy_out=None, stats_out=None):
    """(clean, noisy, stats) of the module's docstring for any int16 batch.  speech_i16, noise_i16: int16 (B, L) tensors on
    one device; n_speech: B lengths (a sequence, array or tensor: the host's copy is used) -- row b of speech_i16 holds
    that many samples and is repeated to fill L; draws: a ``MixDraws`` of B rows.  clean_out, noisy_out: float32 (B, L)
    or (B, 1, L), unit stride along time, made here as (B, L) if not given; on a GPU they start on a 16-byte boundary;
    stats_out: float32 (B, 8), contiguous.  Device tensors go through cum_mix_pairs on the current stream, CPU tensors
    through NumPy on the host."""
    if speech_i16.dtype != torch.int16 or noise_i16.dtype != torch.int16 or speech_i16.dim() != 2 \
            or speech_i16.shape != noise_i16.shape:
        raise ValueError("mix.apply: speech_i16 and noise_i16 must be int16 tensors of one (B, L) shape")
    nb, L = speech_i16.shape
    dev = speech_i16.device
    if not isinstance(draws, MixDraws) or draws.batch != nb:
        raise ValueError(f"mix.apply: draws must be a MixDraws of {nb} rows")
    if nb < 1 or L < 1:
        raise ValueError("mix.apply: the batch must have at least one row and one sample")
    n_speech = np.asarray(n_speech.cpu() if isinstance(n_speech, torch.Tensor) else n_speech, dtype=np.int64).reshape(-1)
    recs = draws.pack(n_speech)
    if clean_out is None:
        clean_out = torch.empty(nb, L, dtype=torch.float32, device=dev)
    if noisy_out is None:
        noisy_out = torch.empty(nb, L, dtype=torch.float32, device=dev)
    if stats_out is None:
        stats_out = torch.empty(nb, STATS, dtype=torch.float32, device=dev)
    co, _ = _rows(clean_out, "clean_out", nb, L)
    no, _ = _rows(noisy_out, "noisy_out", nb, L)
    if stats_out.dtype != torch.float32 or tuple(stats_out.shape) != (nb, STATS) or not stats_out.is_contiguous():
        raise ValueError(f"mix.apply: stats_out must be a contiguous float32 ({nb}, {STATS}) tensor")
    if not (noise_i16.device == clean_out.device == noisy_out.device == stats_out.device == dev):
        raise ValueError("mix.apply: all tensors must be on one device")
    outs = [_span(clean_out, co, nb, L), _span(noisy_out, no, nb, L), _span(stats_out, STATS, nb, STATS)]
    if any(x[0] < y[1] and y[0] < x[1] for i, x in enumerate(outs) for y in outs[i + 1:]):
        raise ValueError("mix.apply: the outputs must not overlap each other")
    if dev.type == "cpu":
        speech, noise = speech_i16.contiguous().numpy(), noise_i16.contiguous().numpy()
        out_c = torch.as_strided(clean_out, (nb, L), (co, 1))
        out_n = torch.as_strided(noisy_out, (nb, L), (no, 1))
        for b in range(nb):
            c, y, st = _host_row(speech[b], noise[b], n_speech[b], L, draws.thr, draws.frame, draws.q(b), draws.l(b),
                                 draws.clip)
            out_c[b], out_n[b], stats_out[b] = torch.from_numpy(c), torch.from_numpy(y), torch.from_numpy(st)
        return clean_out, noisy_out, stats_out
    hip.require_gpu(clean_out, noisy_out, stats_out, any_dtype=True)
    with torch.cuda.device(dev):
        pitch = (L + 7) // 8 * 8
        pcm = torch.zeros(2, nb, pitch, dtype=torch.int16, device=dev)
        pcm[0, :, :L], pcm[1, :, :L] = speech_i16, noise_i16
        launch(pcm, pitch, torch.from_numpy(recs).to(dev), nb, L, workspace_for(nb, L, dev), clean_out, co, noisy_out, no,
               stats_out)
    return clean_out, noisy_out, stats_out
