"""Training augmentation on the (noise, clean) pair: the hook of the reference's train loop (src/training/train.py:262-265)

    # noise = noisy_audio - clean_audio
    # noise, clean_audio = augment((noise, clean_audio))
    # noisy_audio = noise + clean_audio

with the augmentation family of the denoiser lineage CleanUNet comes from: exchange the noises within the batch (remix),
shift noise against speech, re-draw the SNR and the level, add a synthetic room (echo), remove a mel band from speech and
noise alike (BandMask), and put the speech into a measured room (Reverb).  DESIGN.md 7h.

Two halves, kept apart:

  Augment.draw(rng, nb, length)   pure host code: everything random about one batch, as an ``AugmentDraws`` of int32 /
                                  float32 numpy arrays -- the values the kernel reads, already rounded;
  apply(clean_src, noisy_src, draws)
                                  the arithmetic, with nothing random in it: csrc/augment.hip (cum_augment_pairs) on
                                  device tensors, a torch restatement on CPU tensors.

The sources are the clean and noisy crops ``shift`` samples LONGER than the batch, (B, L + S); row b of the result is

    c0[t] = C[b, t + off_clean[b]]                       n0[t] = Y[p, t + off_noise[b]] - C[p, t + off_noise[b]],  p = perm[b]
    rc[t] = sum_k tap_gain[b, k] c0[t - delay[b, k]]     rn[t] = sum_k tap_gain[b, k] n0[t - delay[b, k]]
    c1 = c0 + kappa rc                                   n1 = n0 + rn + (1 - kappa) rc
    a  = sqrt(Ec / (En 10^(snr_db / 10))),  Ec = sum c1^2, En = sum n1^2 in f64  (1 if snr_db is NaN or a sum is 0)
    clean' = gain c1                                     noisy' = gain (c1 + a n1)

(k ascending, terms with t < delay dropped).  ``BatchFeeder(..., augment=Augment(...))`` (training/feeder.py) draws per
batch from its own generator and runs this between the assembling kernel and the train step's inputs.

BandMask is a stage of its own in front of that arithmetic: with a band drawn (``band_half`` W > 0, cutoffs ``band_lo``
<= ``band_hi`` in cycles per sample), both source rows, zero outside their L + S samples, are filtered by

    w[k] = 0.54 - 0.46 cos(pi (k + W) / W),  lp_c[k] = 2 c sinc(2 c k) w[k],  h[k] = [k == 0] + lp_lo[k] - lp_hi[k]

(k = -W..W, in f64, h rounded to f32) and everything above reads the filtered rows in place of C and Y.  The filters are
up to 3 201 taps long: csrc/bandmask.hip (cum_band_mask_pairs) applies them by overlap-save on an in-LDS FFT;
``band_mask`` is that stage alone, ``apply`` runs it first when any row has a band.

Reverb is the stage in front of both: row b carries an id ``rir[b]`` into a bank of room impulse responses (``Reverb``:
measured or simulated, cut at the direct path and at -60 dB of the Schroeder integral, at most 16 384 dense taps, unit
energy).  With h = taps[rir[b]] of T taps (an id outside the bank: the row is copied),

    Cr[b, t] = sum_{k = 0 .. min(t, T - 1)} h[k] C[b, t - k]      clean = Cr      noisy = (Y - C) + Cr

so the target is the reverberant speech and the noise Y - C stays free of speech.  csrc/reverb.hip (cum_reverb_pairs)
does it by partitioned overlap-save on the same in-LDS FFT; ``reverb`` is that stage alone, ``apply(..., reverb=...)``
runs it first when any row has a response.  The order is fixed: assemble -> reverb -> band mask -> the arithmetic above.
"""
import ctypes
import math
import os

import numpy as np
import torch

from .. import hip

K_MAX = 512                      # taps per row the kernel takes (csrc/augment.hip)
REC_INTS = 8                     # one record per row: the fields below, then zeros
REC_PERM, REC_OFF_CLEAN, REC_OFF_NOISE, REC_N_TAPS, REC_SNR_DB, REC_GAIN, REC_KAPPA = range(7)
W_MAX = 1600                     # the longest half-width the band-mask kernel takes (csrc/bandmask.hip)
BAND_INTS = 4                    # one band record per row: W, c_lo (f32 bits), c_hi (f32 bits), 0
REVERB_INTS = 4                  # one reverb record per row: rir, 0, 0, 0


def _range(value, name):
    if value is None:
        return None
    lo, hi = (float(v) for v in value)
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise ValueError(f"{name} must be None or a finite (lo, hi) with lo <= hi; got {value!r}")
    return lo, hi


class Echo:
    """A synthetic room: ``repeat`` trains of decaying reflections of the clip added to itself.  With probability
    ``proba`` per row:  init = U(0, 1) initial, fd = U(first_delay) s, rt = U(rt60) s;  then ``repeat`` times, from
    frac = 1, g = init, d = 0, while frac > 1e-3:

        d += 1 + int((1 + jitter U(-1, 1)) fd sample_rate);  tap (d, g) if d < length;
        a = 10^(-3 (1 + jitter U(-1, 1)) fd / rt);  g *= a;  frac *= a

    ``keep_clean`` (kappa) is the share of the speech's reverberation that stays in the target; the rest goes to the
    noise.  The constructor counts the taps of the worst case -- the smallest first delay, the largest rt60, the jitter
    at its most negative -- and raises ValueError when they exceed K_MAX."""

    def __init__(self, proba=1.0, initial=0.3, first_delay=(0.01, 0.03), rt60=(0.3, 1.3), repeat=3, jitter=0.1,
                 keep_clean=0.1, sample_rate=16000):
        self.proba, self.initial, self.jitter = float(proba), float(initial), float(jitter)
        self.first_delay, self.rt60 = _range(first_delay, "first_delay"), _range(rt60, "rt60")
        self.repeat, self.keep_clean, self.sample_rate = int(repeat), float(keep_clean), int(sample_rate)
        if self.first_delay is None or self.rt60 is None or self.first_delay[0] <= 0 or self.rt60[0] <= 0:
            raise ValueError("Echo: first_delay and rt60 must be positive (lo, hi) ranges in seconds")
        if not (0 <= self.proba <= 1 and 0 <= self.jitter < 1 and self.repeat >= 1 and self.sample_rate >= 1):
            raise ValueError("Echo: proba in [0, 1], jitter in [0, 1), repeat >= 1 and sample_rate >= 1 are required")
        a = 10.0 ** (-3.0 * (1.0 - self.jitter) * self.first_delay[0] / self.rt60[1])
        frac, per_repeat = 1.0, 0
        while frac > 1e-3 and per_repeat <= K_MAX:
            per_repeat, frac = per_repeat + 1, frac * a
        self.max_taps = self.repeat * per_repeat
        if self.max_taps > K_MAX:
            raise ValueError(f"Echo: the worst case (first_delay {self.first_delay[0]:g} s, rt60 {self.rt60[1]:g} s, "
                             f"jitter -{self.jitter:g}) gives {self.repeat} x {per_repeat}{'+' if per_repeat > K_MAX else ''}"
                             f" taps, more than the kernel's {K_MAX}")

    def draw(self, rng, length):
        """[(delay, gain)] of one row (empty with probability 1 - proba)."""
        taps = []
        if not rng.random() < self.proba:
            return taps
        init = rng.random() * self.initial
        fd = rng.uniform(*self.first_delay)
        rt = rng.uniform(*self.rt60)
        for _ in range(self.repeat):
            frac, g, d = 1.0, init, 0
            while frac > 1e-3:
                d += 1 + int((1 + self.jitter * rng.uniform(-1, 1)) * fd * self.sample_rate)
                if d < length:
                    taps.append((d, g))
                a = 10.0 ** (-3 * (1 + self.jitter * rng.uniform(-1, 1)) * fd / rt)
                g *= a
                frac *= a
        return taps


def mel_edges(bands=120, min_freq=40.0, sample_rate=16000):
    """The ``bands`` band edges in cycles per sample, float32: evenly spaced on the mel scale mel(f) = 2595 log10(1 +
    f / 700) from ``min_freq`` to ``sample_rate / 2``, computed in f64 and rounded once."""
    lo, hi = (2595.0 * np.log10(1.0 + f / 700.0) for f in (float(min_freq), sample_rate / 2.0))
    hz = 700.0 * (10.0 ** (np.linspace(lo, hi, int(bands)) / 2595.0) - 1.0)
    return (hz / sample_rate).astype(np.float32)


def band_taps(W, c_lo, c_hi):
    """h[-W..W] of the module's docstring for float32 cutoffs: evaluated in f64, returned as float32."""
    W, lo, hi = int(W), float(np.float32(c_lo)), float(np.float32(c_hi))
    k = np.arange(-W, W + 1, dtype=np.float64)
    w = 0.54 - 0.46 * np.cos(np.pi * (k + W) / W)
    h = 2 * lo * np.sinc(2 * lo * k) * w - 2 * hi * np.sinc(2 * hi * k) * w
    h[W] += 1.0
    return h.astype(np.float32)


class BandMask:
    """Remove one band between two of ``bands`` mel edges from speech and noise alike.  With probability ``proba`` per
    batch: lo uniform over the edges, hi uniform in [lo, min(bands, lo + bandwidth)), bandwidth = int(maxwidth bands);
    the filter's half-width is W = int(2 / c_lo), c_lo the lower edge in cycles per sample (float32).  The constructor
    refuses a config whose lowest edge needs more than W_MAX."""

    def __init__(self, maxwidth=0.2, bands=120, min_freq=40.0, proba=1.0, sample_rate=16000):
        self.maxwidth, self.bands, self.min_freq = float(maxwidth), int(bands), float(min_freq)
        self.proba, self.sample_rate = float(proba), int(sample_rate)
        if not (self.bands >= 2 and self.sample_rate >= 1 and 0 < self.min_freq < self.sample_rate / 2
                and 0 <= self.proba <= 1):
            raise ValueError("BandMask: bands >= 2, 0 < min_freq < sample_rate / 2 and proba in [0, 1] are required")
        self.bandwidth = int(self.maxwidth * self.bands)
        if self.bandwidth < 1:
            raise ValueError(f"BandMask: maxwidth {self.maxwidth:g} of {self.bands} bands is no band at all")
        self.edges = mel_edges(self.bands, self.min_freq, self.sample_rate)
        self.max_half = int(2.0 / float(self.edges[0]))
        if self.max_half > W_MAX:
            raise ValueError(f"BandMask: the edge at {self.min_freq:g} Hz needs a filter of half-width {self.max_half}, "
                             f"more than the kernel's {W_MAX}")

    def draw(self, rng):
        """(W, c_lo, c_hi) of one batch; (0, 0, 0) with probability 1 - proba."""
        if not rng.random() < self.proba:
            return 0, np.float32(0), np.float32(0)
        lo = int(rng.integers(0, self.bands))
        hi = int(rng.integers(lo, min(self.bands, lo + self.bandwidth)))
        return int(2.0 / float(self.edges[lo])), self.edges[lo], self.edges[hi]


def prepare_rir(h, decay_db=60.0, max_taps=None):
    """One raw response as the kernel gets it, deterministic, in f64: cut in front of the direct path (the first sample
    of the largest magnitude), cut behind the last sample at which the backward-integrated energy (Schroeder) is still
    above ``-decay_db`` of the total, capped at ``max_taps``, scaled to unit energy, rounded to float32."""
    h = np.asarray(h)
    if h.ndim == 2:
        h = h[0]                                         # channels first: channel 0
    if h.ndim != 1 or h.size == 0:
        raise ValueError(f"Reverb: a response must be a non-empty 1-D (or channels-first 2-D) array; got shape {h.shape}")
    h = h.astype(np.float64)
    if not np.isfinite(h).all() or not np.abs(h).max() > 0:
        raise ValueError("Reverb: a response must be finite and not all zero")
    h = h[int(np.argmax(np.abs(h))):]
    tail = np.cumsum((h * h)[::-1])[::-1]                # energy from t to the end
    h = h[:max(1, int(np.count_nonzero(tail > tail[0] * 10.0 ** (-float(decay_db) / 10.0))))]
    if max_taps is not None:
        h = h[:int(max_taps)]
    return (h / math.sqrt(float((h * h).sum()))).astype(np.float32)


class ReverbBank:
    """A ``Reverb``'s responses on one device as cum_reverb_pairs reads them: ``blob`` (float32, every response on a
    16-byte boundary), ``table`` (int32 (R, 4): {offset in floats as int64 in ints 0-1, taps, 0}), ``table_host`` (the
    same as a numpy array, for the library's check before the launch) and ``taps`` (the float32 numpy arrays)."""

    def __init__(self, taps, device):
        self.taps = taps
        self.table_host = np.zeros((len(taps), 4), dtype=np.int32)
        at = 0
        for r, h in enumerate(taps):
            self.table_host[r].view(np.int64)[0], self.table_host[r, 2] = at, h.shape[0]
            at += (h.shape[0] + 3) // 4 * 4
        blob = np.zeros(at, dtype=np.float32)
        for r, h in enumerate(taps):
            o = int(self.table_host[r].view(np.int64)[0])
            blob[o:o + h.shape[0]] = h
        self.blob, self.table = torch.from_numpy(blob).to(device), torch.from_numpy(self.table_host).to(device)
        self.device = self.blob.device

    def __len__(self):
        return len(self.taps)


class Reverb:
    """A bank of room impulse responses.  ``rirs``: a sequence of 1-D (or channels-first 2-D: channel 0) float arrays, or
    a directory: every ``*.wav`` below it, sorted by relative path, read whole (util/dataset.py); a file at another rate
    than ``sample_rate`` or in an encoding the reader does not take is a ValueError naming the file (responses are not
    resampled).  Every response is prepared once, here (``prepare_rir``: direct path first, cut at ``-decay_db`` of the
    Schroeder integral, at most ``min(max_taps, T_MAX)`` taps, T_MAX = cum_reverb_max_taps() = 16 384, unit energy,
    float32); ``taps[r]`` is what the kernel gets.  With probability ``proba`` per row a response is drawn uniformly."""

    def __init__(self, rirs, proba=0.5, sample_rate=16000, decay_db=60.0, max_taps=None):
        self.proba, self.sample_rate, self.decay_db = float(proba), int(sample_rate), float(decay_db)
        if not 0 <= self.proba <= 1:
            raise ValueError("Reverb: proba must lie in [0, 1]")
        if not (math.isfinite(self.decay_db) and self.decay_db > 0):
            raise ValueError("Reverb: decay_db must be positive")
        if max_taps is not None and int(max_taps) < 1:
            raise ValueError("Reverb: max_taps must be at least 1")
        self.t_max = int(hip.lib().cum_reverb_max_taps())
        self.max_taps = min(int(max_taps) if max_taps is not None else self.t_max, self.t_max)
        if isinstance(rirs, (str, os.PathLike)):
            rirs = self._read_tree(os.fspath(rirs))
        rirs = list(rirs)
        if not rirs:
            raise ValueError("Reverb: no room impulse response given")
        self.taps = [prepare_rir(h, self.decay_db, self.max_taps) for h in rirs]
        self._banks = {}

    def _read_tree(self, root):
        from ..util.dataset import _read_whole_float
        names = sorted(os.path.relpath(os.path.join(d, f), root) for d, _, files in os.walk(root) for f in files
                       if f.lower().endswith(".wav"))
        out = []
        for name in names:
            path = os.path.join(root, name)
            try:
                rate, x = _read_whole_float(path)
            except Exception as exc:      # noqa: BLE001 - whatever the reader raises, with the file's name
                raise ValueError(f"Reverb: {path} cannot be read: {exc}") from exc
            if int(rate) != self.sample_rate:
                raise ValueError(f"Reverb: {path} is at {rate} Hz, not {self.sample_rate} (responses are not resampled)")
            out.append(x)
        return out

    def __len__(self):
        return len(self.taps)

    def bank(self, device):
        """The ``ReverbBank`` on ``device``, uploaded once and kept."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._banks:
            self._banks[device] = ReverbBank(self.taps, device)
        return self._banks[device]

    def draw(self, rng):
        """The response id of one row; -1 with probability 1 - proba."""
        if not rng.random() < self.proba:
            return -1
        return int(rng.integers(0, len(self.taps)))


class AugmentDraws:
    """Everything random about one batch of ``nb`` rows of ``length`` samples, as the kernel reads it: int32 ``perm``,
    ``off_clean``, ``off_noise``, ``n_taps`` (nb,) and ``delay`` (nb, K_MAX); float32 ``snr_db`` (NaN: keep), ``gain``,
    ``kappa`` (nb,) and ``tap_gain`` (nb, K_MAX).  ``shift``: the sources are ``length + shift`` long.  The band of every
    row (default: none): int32 ``band_half`` W (0: no band), float32 ``band_lo`` <= ``band_hi`` in cycles per sample.  The
    room of every row (default: none): int32 ``rir``, an id into a ``Reverb``'s bank; an id outside it (-1) is no room."""

    def __init__(self, length, shift, perm, off_clean, off_noise, snr_db, gain, kappa, n_taps, delay, tap_gain,
                 band_half=None, band_lo=None, band_hi=None, rir=None):
        self.length, self.shift = int(length), int(shift)
        self.perm, self.off_clean, self.off_noise, self.n_taps = (np.ascontiguousarray(v, dtype=np.int32)
                                                                  for v in (perm, off_clean, off_noise, n_taps))
        self.snr_db, self.gain, self.kappa = (np.ascontiguousarray(v, dtype=np.float32) for v in (snr_db, gain, kappa))
        self.delay = np.ascontiguousarray(delay, dtype=np.int32)
        self.tap_gain = np.ascontiguousarray(tap_gain, dtype=np.float32)
        nb = self.perm.shape[0]
        zeros = np.zeros(nb)
        self.band_half = np.ascontiguousarray(zeros if band_half is None else band_half, dtype=np.int32)
        self.band_lo, self.band_hi = (np.ascontiguousarray(zeros if v is None else v, dtype=np.float32)
                                      for v in (band_lo, band_hi))
        self.rir = np.ascontiguousarray(np.full(nb, -1) if rir is None else rir, dtype=np.int32)
        if self.length < 1 or self.shift < 0 or nb < 1:
            raise ValueError("AugmentDraws: length >= 1, shift >= 0 and at least one row are required")
        for name in ("off_clean", "off_noise", "n_taps", "snr_db", "gain", "kappa", "band_half", "band_lo", "band_hi",
                     "rir"):
            if getattr(self, name).shape != (nb,):
                raise ValueError(f"AugmentDraws: {name} must have shape ({nb},)")
        if self.delay.shape != self.tap_gain.shape or self.delay.ndim != 2 or self.delay.shape[0] != nb \
                or self.delay.shape[1] > K_MAX:
            raise ValueError(f"AugmentDraws: delay and tap_gain must both be ({nb}, K <= {K_MAX})")
        if sorted(self.perm.tolist()) != list(range(nb)):
            raise ValueError("AugmentDraws: perm must be a permutation of the rows")
        if min(self.off_clean.min(), self.off_noise.min()) < 0 or max(self.off_clean.max(), self.off_noise.max()) > shift:
            raise ValueError("AugmentDraws: offsets must lie in [0, shift]")
        if self.n_taps.min() < 0 or self.n_taps.max() > self.delay.shape[1]:
            raise ValueError("AugmentDraws: n_taps must lie in [0, K]")
        if self.band_half.min() < 0 or self.band_half.max() > W_MAX:
            raise ValueError(f"AugmentDraws: band_half must lie in [0, {W_MAX}]")
        if not (np.isfinite(self.band_lo).all() and np.isfinite(self.band_hi).all() and self.band_lo.min() >= 0
                and (self.band_lo <= self.band_hi).all() and self.band_hi.max() <= 0.5):
            raise ValueError("AugmentDraws: 0 <= band_lo <= band_hi <= 0.5 (cycles per sample) is required")

    @property
    def batch(self):
        return self.perm.shape[0]

    @property
    def rescales(self):
        """Whether any row re-draws its SNR (the kernel then needs its second launch and a workspace)."""
        return bool(np.isfinite(self.snr_db).any())

    @property
    def banded(self):
        """Whether any row has a band to remove (the band-mask stage then runs in front of the rest)."""
        return bool(self.band_half.any())

    @property
    def reverberant(self):
        """Whether any row has a room (the reverb stage then runs in front of everything else)."""
        return bool((self.rir >= 0).any())

    def without_band(self):
        """The same draws with no band on any row."""
        return AugmentDraws(self.length, self.shift, self.perm, self.off_clean, self.off_noise, self.snr_db, self.gain,
                            self.kappa, self.n_taps, self.delay, self.tap_gain, rir=self.rir)

    def without_reverb(self):
        """The same draws with no room on any row."""
        return AugmentDraws(self.length, self.shift, self.perm, self.off_clean, self.off_noise, self.snr_db, self.gain,
                            self.kappa, self.n_taps, self.delay, self.tap_gain, self.band_half, self.band_lo, self.band_hi)

    def pack_reverb(self):
        """The rooms as one int32 array: nb records {rir, 0, 0, 0}."""
        out = np.zeros((self.batch, REVERB_INTS), dtype=np.int32)
        out[:, 0] = self.rir
        return out.reshape(-1)

    def pack_band(self):
        """The bands as one int32 array: nb records {W, c_lo (its bits), c_hi (its bits), 0}."""
        out = np.zeros((self.batch, BAND_INTS), dtype=np.int32)
        out[:, 0], out[:, 1], out[:, 2] = self.band_half, self.band_lo.view(np.int32), self.band_hi.view(np.int32)
        return out.reshape(-1)

    def columns(self):
        """Tap columns a packed table of these draws needs: the longest list, rounded up to 4."""
        return (int(self.n_taps.max()) + 3) // 4 * 4

    def pack(self, k=None):
        """The draws as one int32 array: nb records of 8, then delay[:, :k], then tap_gain[:, :k] (its bits)."""
        k = self.columns() if k is None else int(k)
        nb = self.batch
        if not self.n_taps.max() <= k <= K_MAX:
            raise ValueError(f"AugmentDraws.pack: k = {k} does not hold {int(self.n_taps.max())} taps (or exceeds {K_MAX})")
        out = np.zeros(table_ints(nb, k), dtype=np.int32)
        recs = out[:nb * REC_INTS].reshape(nb, REC_INTS)
        recs[:, REC_PERM], recs[:, REC_OFF_CLEAN], recs[:, REC_OFF_NOISE] = self.perm, self.off_clean, self.off_noise
        recs[:, REC_N_TAPS] = self.n_taps
        recs[:, REC_SNR_DB], recs[:, REC_GAIN] = self.snr_db.view(np.int32), self.gain.view(np.int32)
        recs[:, REC_KAPPA] = self.kappa.view(np.int32)
        have = min(k, self.delay.shape[1])
        taps = out[nb * REC_INTS:].reshape(2, nb, k)
        taps[0, :, :have], taps[1, :, :have] = self.delay[:, :have], self.tap_gain[:, :have].view(np.int32)
        return out


def table_ints(nb, k):
    """int32 entries of a packed table of nb rows with k tap columns."""
    return nb * (REC_INTS + 2 * k)


def band_ints(nb):
    """int32 entries of the packed bands of nb rows."""
    return BAND_INTS * nb


def reverb_ints(nb):
    """int32 entries of the packed rooms of nb rows."""
    return REVERB_INTS * nb


class Augment:
    """``Augment(remix=False, shift=0, snr_db=None, gain_db=None, echo=None, band_mask=None, reverb=None)``

    remix: every row gets the noise of a row drawn by one uniform permutation of the batch.
    shift: speech and noise each start at their own uniform offset in [0, shift] of crops ``shift`` samples longer.
    snr_db: (lo, hi) -- the noise is rescaled so that the row's SNR is uniform in the range -- or None (keep).
    gain_db: (lo, hi) -- both signals are scaled by 10^(g / 20), g uniform in the range -- or None.
    echo: ``Echo(...)`` or None.
    band_mask: ``BandMask(...)`` or None: one band per batch is removed from speech and noise before everything else.
    reverb: ``Reverb(...)`` or None: a row's speech is convolved with a room impulse response, before the band mask.
    A config with every transform off is ``inactive`` and is treated by its users exactly as no augmentation."""

    def __init__(self, remix=False, shift=0, snr_db=None, gain_db=None, echo=None, band_mask=None, reverb=None):
        self.remix, self.shift = bool(remix), int(shift)
        self.snr_db, self.gain_db = _range(snr_db, "snr_db"), _range(gain_db, "gain_db")
        if self.shift < 0:
            raise ValueError("Augment: shift must be at least 0")
        if echo is not None and not isinstance(echo, Echo):
            raise ValueError("Augment: echo must be an Echo or None")
        if band_mask is not None and not isinstance(band_mask, BandMask):
            raise ValueError("Augment: band_mask must be a BandMask or None")
        if reverb is not None and not isinstance(reverb, Reverb):
            raise ValueError("Augment: reverb must be a Reverb or None")
        self.echo, self.band_mask, self.reverb = echo, band_mask, reverb

    @property
    def active(self):
        return self.remix or self.shift > 0 or self.snr_db is not None or self.gain_db is not None \
            or self.echo is not None or self.band_mask is not None or self.reverb is not None

    @property
    def max_taps(self):
        """Tap columns a batch of this config can need, rounded up to 4 (0 without echo)."""
        return 0 if self.echo is None else min(K_MAX, (self.echo.max_taps + 3) // 4 * 4)

    def draw(self, rng, nb, length):
        """The draws of one batch from ``rng`` (a numpy Generator), in this order: the permutation; nb clean offsets;
        nb noise offsets; nb SNRs; nb gains; then row by row the echo (Echo.draw); then the
        batch's one band (BandMask.draw), copied into every row; last, row by row, the room (Reverb.draw).  A transform
        that is off draws nothing."""
        nb, length = int(nb), int(length)
        perm = rng.permutation(nb) if self.remix else np.arange(nb)
        if self.shift > 0:
            off_clean = rng.integers(0, self.shift + 1, nb)
            off_noise = rng.integers(0, self.shift + 1, nb)
        else:
            off_clean = off_noise = np.zeros(nb, np.int64)
        snr = rng.uniform(*self.snr_db, nb) if self.snr_db is not None else np.full(nb, np.nan)
        gain = 10.0 ** (rng.uniform(*self.gain_db, nb) / 20.0) if self.gain_db is not None else np.ones(nb)
        n_taps = np.zeros(nb, np.int32)
        delay, tap_gain = np.zeros((nb, K_MAX), np.int32), np.zeros((nb, K_MAX), np.float32)
        kappa = np.full(nb, self.echo.keep_clean if self.echo is not None else 0.0)
        if self.echo is not None:
            for b in range(nb):
                taps = self.echo.draw(rng, length)
                n_taps[b] = len(taps)          # (at most echo.max_taps <= K_MAX: the constructor's worst case)
                if taps:
                    delay[b, :len(taps)], tap_gain[b, :len(taps)] = zip(*taps)
        band = ()
        if self.band_mask is not None:
            band = [np.full(nb, v) for v in self.band_mask.draw(rng)]
        rir = [self.reverb.draw(rng) for _ in range(nb)] if self.reverb is not None else None
        return AugmentDraws(length, self.shift, perm, off_clean, off_noise, snr, gain, kappa, n_taps, delay, tap_gain,
                            *band, rir=rir)


# ---------------------------------------------------------------------------------------------------------------- apply
def _rows(t, name, nb, n):
    """(row stride in elements, whether t is (B, 1, n)) of a float32 (B, n) or (B, 1, n) tensor with unit time stride."""
    if t.dtype != torch.float32 or tuple(t.shape) not in ((nb, n), (nb, 1, n)):
        raise ValueError(f"augment.apply: {name} must be a float32 ({nb}, {n}) or ({nb}, 1, {n}) tensor; got {t.dtype} "
                         f"{tuple(t.shape)}")
    if n > 1 and t.stride(-1) != 1:
        raise ValueError(f"augment.apply: {name} must have unit stride along time")
    return (t.stride(0) if nb > 1 else n), t.dim() == 3


def _span(t, sb, nb, n):
    lo = t.data_ptr()
    return lo, lo + 4 * ((nb - 1) * sb + n)


def _host(clean_src, cs, noisy_src, ys, draws, clean_out, co, noisy_out, no):
    """The arithmetic of the module's docstring with torch on the host, row by row, tap by tap in ascending k."""
    nb, L, n = draws.batch, draws.length, draws.length + draws.shift
    C = torch.as_strided(clean_src, (nb, n), (cs, 1))
    Y = torch.as_strided(noisy_src, (nb, n), (ys, 1))
    out_c = torch.as_strided(clean_out, (nb, L), (co, 1))
    out_n = torch.as_strided(noisy_out, (nb, L), (no, 1))
    for b in range(nb):
        p, oc, on = int(draws.perm[b]), int(draws.off_clean[b]), int(draws.off_noise[b])
        c0 = C[b, oc:oc + L].clone()
        n0 = Y[p, on:on + L] - C[p, on:on + L]
        rc, rn = torch.zeros(L), torch.zeros(L)
        for k in range(int(draws.n_taps[b])):
            d, g = int(draws.delay[b, k]), float(draws.tap_gain[b, k])
            if 1 <= d < L:
                rc[d:].add_(c0[:L - d], alpha=g)
                rn[d:].add_(n0[:L - d], alpha=g)
        kappa = torch.tensor(draws.kappa[b])
        c1 = c0 + kappa * rc
        n1 = (n0 + rn) + (1 - kappa) * rc
        a = 1.0
        ec, en = float(c1.double().square().sum()), float(n1.double().square().sum())
        snr = float(draws.snr_db[b])
        if math.isfinite(snr) and ec > 0 and en > 0:
            a = math.sqrt(ec / (en * 10.0 ** (snr / 10.0)))
        gain = torch.tensor(draws.gain[b])
        out_c[b] = gain * c1
        out_n[b] = gain * (c1 + torch.tensor(a, dtype=torch.float32) * n1)


def launch(clean_src, cs, noisy_src, ys, nb, length, src_len, table, k, workspace, clean, co, noisy, no):
    """cum_augment_pairs on the current stream.  table: the device int32 tensor of ``AugmentDraws.pack(k)``; workspace:
    a device tensor of cum_augment_workspace_elems floats, or None when no row re-draws its SNR."""
    recs = table.data_ptr()
    delay = recs + 4 * nb * REC_INTS
    hip.check(hip.lib().cum_augment_pairs(
        hip.ptr(clean_src), cs, hip.ptr(noisy_src), ys, nb, length, src_len, ctypes.c_void_p(recs),
        ctypes.c_void_p(delay if k else None), ctypes.c_void_p(delay + 4 * nb * k if k else None), k, hip.ptr(workspace),
        hip.ptr(clean), co, hip.ptr(noisy), no, hip.stream_ptr()))


def workspace_for(nb, length, device):
    """The f64 tile sums' room for a batch of nb rows of length samples (8-byte aligned: a float64 tensor)."""
    return torch.empty(max(1, hip.lib().cum_augment_workspace_elems(nb, length) // 2), dtype=torch.float64, device=device)


def band_workspace_for(nb, device):
    """The twiddle table's and the spectra's room for a batch of nb rows (8-byte aligned: a fresh tensor)."""
    return torch.empty(hip.lib().cum_band_mask_workspace_elems(nb), dtype=torch.float32, device=device)


def launch_band(clean_src, cs, noisy_src, ys, nb, n, recs, workspace, clean, co, noisy, no):
    """cum_band_mask_pairs on the current stream.  recs: the device int32 tensor of ``AugmentDraws.pack_band()``;
    workspace: a device tensor of cum_band_mask_workspace_elems floats."""
    hip.check(hip.lib().cum_band_mask_pairs(hip.ptr(clean_src), cs, hip.ptr(noisy_src), ys, nb, n, hip.ptr(recs),
                                            hip.ptr(workspace), hip.ptr(clean), co, hip.ptr(noisy), no, hip.stream_ptr()))


def band_mask(clean_src, noisy_src, draws, clean_out=None, noisy_out=None):
    """The band-mask stage alone: both sources, float32 (B, n) or (B, 1, n) with n = draws.length + draws.shift, filtered
    row by row with the taps of (draws.band_half, band_lo, band_hi) into clean_out, noisy_out of the same shape (made
    here if not given; on a GPU they start on a 16-byte boundary and must not overlap the sources).  Device tensors go
    through cum_band_mask_pairs on the current stream; CPU tensors through a float32 direct convolution with the same
    float32 taps.  A row with band_half = 0 is copied."""
    nb, n = draws.batch, draws.length + draws.shift
    dev = clean_src.device
    cs, three = _rows(clean_src, "clean_src", nb, n)
    ys, _ = _rows(noisy_src, "noisy_src", nb, n)
    if clean_out is None:
        clean_out = torch.empty((nb, 1, n) if three else (nb, n), dtype=torch.float32, device=dev)
    if noisy_out is None:
        noisy_out = torch.empty((nb, 1, n) if three else (nb, n), dtype=torch.float32, device=dev)
    co, _ = _rows(clean_out, "clean_out", nb, n)
    no, _ = _rows(noisy_out, "noisy_out", nb, n)
    if not (noisy_src.device == clean_out.device == noisy_out.device == dev):
        raise ValueError("augment.band_mask: all tensors must be on one device")
    spans = [_span(clean_src, cs, nb, n), _span(noisy_src, ys, nb, n)]
    outs = [_span(clean_out, co, nb, n), _span(noisy_out, no, nb, n)]
    if any(o[0] < s[1] and s[0] < o[1] for o in outs for s in spans) or (outs[0][0] < outs[1][1] and outs[1][0] < outs[0][1]):
        raise ValueError("augment.band_mask: the outputs must not overlap the sources or each other")
    if dev.type == "cpu":
        for src, sb, out, ob in ((clean_src, cs, clean_out, co), (noisy_src, ys, noisy_out, no)):
            x, y = torch.as_strided(src, (nb, n), (sb, 1)), torch.as_strided(out, (nb, n), (ob, 1))
            for b in range(nb):
                W = int(draws.band_half[b])
                if W == 0:
                    y[b] = x[b]
                    continue
                h = torch.from_numpy(band_taps(W, draws.band_lo[b], draws.band_hi[b]))     # (symmetric: no flip)
                y[b] = torch.nn.functional.conv1d(x[b].reshape(1, 1, n), h.reshape(1, 1, -1), padding=W).reshape(n)
        return clean_out, noisy_out
    hip.require_gpu(clean_src, noisy_src, clean_out, noisy_out)
    with torch.cuda.device(dev):
        recs = torch.from_numpy(draws.pack_band()).to(dev)
        launch_band(clean_src, cs, noisy_src, ys, nb, n, recs, band_workspace_for(nb, dev), clean_out, co, noisy_out, no)
    return clean_out, noisy_out


def reverb_workspace_for(nb, n, device):
    """The twiddle table's and the spectra's room for a batch of nb rows of n samples (8-byte aligned: a fresh tensor)."""
    return torch.empty(hip.lib().cum_reverb_workspace_elems(nb, n), dtype=torch.float32, device=device)


def launch_reverb(clean_src, cs, noisy_src, ys, nb, n, recs, bank, workspace, clean, co, noisy, no):
    """cum_reverb_pairs on the current stream.  recs: the device int32 tensor of ``AugmentDraws.pack_reverb()``; bank: the
    ``ReverbBank`` of the tensors' device; workspace: a device tensor of cum_reverb_workspace_elems floats."""
    hip.check(hip.lib().cum_reverb_pairs(hip.ptr(clean_src), cs, hip.ptr(noisy_src), ys, nb, n, hip.ptr(recs),
                                         hip.ptr(bank.blob), bank.blob.numel(),
                                         ctypes.c_void_p(bank.table_host.ctypes.data), hip.ptr(bank.table), len(bank),
                                         hip.ptr(workspace), hip.ptr(clean), co, hip.ptr(noisy), no, hip.stream_ptr()))


def reverb(clean_src, noisy_src, draws, bank, clean_out=None, noisy_out=None):
    """The reverb stage alone: the sources, float32 (B, n) or (B, 1, n) with n = draws.length + draws.shift; row b with
    h = bank.taps[draws.rir[b]] gives clean = h * C (causal, n samples) and noisy = (Y - C) + clean into clean_out,
    noisy_out of the same shape (made here if not given; on a GPU they start on a 16-byte boundary and must not overlap
    the sources); a row whose id is outside the bank is copied.  ``bank``: ``Reverb.bank(device)``.  Device tensors go
    through cum_reverb_pairs on the current stream; CPU tensors through a float32 direct convolution with the same
    float32 taps."""
    nb, n = draws.batch, draws.length + draws.shift
    dev = clean_src.device
    cs, three = _rows(clean_src, "clean_src", nb, n)
    ys, _ = _rows(noisy_src, "noisy_src", nb, n)
    if not isinstance(bank, ReverbBank):
        raise ValueError("augment.reverb: bank must be a ReverbBank (Reverb.bank(device))")
    if clean_out is None:
        clean_out = torch.empty((nb, 1, n) if three else (nb, n), dtype=torch.float32, device=dev)
    if noisy_out is None:
        noisy_out = torch.empty((nb, 1, n) if three else (nb, n), dtype=torch.float32, device=dev)
    co, _ = _rows(clean_out, "clean_out", nb, n)
    no, _ = _rows(noisy_out, "noisy_out", nb, n)
    if not (noisy_src.device == clean_out.device == noisy_out.device == dev):
        raise ValueError("augment.reverb: all tensors must be on one device")
    spans = [_span(clean_src, cs, nb, n), _span(noisy_src, ys, nb, n)]
    outs = [_span(clean_out, co, nb, n), _span(noisy_out, no, nb, n)]
    if any(o[0] < s[1] and s[0] < o[1] for o in outs for s in spans) or (outs[0][0] < outs[1][1] and outs[1][0] < outs[0][1]):
        raise ValueError("augment.reverb: the outputs must not overlap the sources or each other")
    if dev.type == "cpu":
        C, Y = torch.as_strided(clean_src, (nb, n), (cs, 1)), torch.as_strided(noisy_src, (nb, n), (ys, 1))
        out_c, out_y = torch.as_strided(clean_out, (nb, n), (co, 1)), torch.as_strided(noisy_out, (nb, n), (no, 1))
        for b in range(nb):
            r = int(draws.rir[b])
            if not 0 <= r < len(bank):
                out_c[b], out_y[b] = C[b], Y[b]
                continue
            h = torch.from_numpy(bank.taps[r][:n].copy())          # (taps past n never meet a sample)
            T = h.shape[0]
            x = torch.nn.functional.pad(C[b].reshape(1, 1, n), (T - 1, 0))
            cr = torch.nn.functional.conv1d(x, h.flip(0).reshape(1, 1, T)).reshape(n)
            out_y[b] = (Y[b] - C[b]) + cr
            out_c[b] = cr
        return clean_out, noisy_out
    hip.require_gpu(clean_src, noisy_src, clean_out, noisy_out)
    if bank.device != dev:
        raise ValueError(f"augment.reverb: the bank is on {bank.device}, the tensors on {dev}")
    with torch.cuda.device(dev):
        recs = torch.from_numpy(draws.pack_reverb()).to(dev)
        launch_reverb(clean_src, cs, noisy_src, ys, nb, n, recs, bank, reverb_workspace_for(nb, n, dev), clean_out, co,
                      noisy_out, no)
    return clean_out, noisy_out


_reverb_stage = reverb           # (``apply`` has a parameter of the stage's name)


def apply(clean_src, noisy_src, draws, clean_out=None, noisy_out=None, reverb=None):
    """(clean', noisy') of the module's docstring.  clean_src, noisy_src: float32 (B, L + S) or (B, 1, L + S) tensors on
    one device, unit stride along time, L = draws.length, S = draws.shift; clean_out, noisy_out: (B, L) or (B, 1, L), made
    here (in the sources' form) if not given; on a GPU they start on a 16-byte boundary and must not overlap the sources.
    Device tensors go through cum_augment_pairs on the current stream, CPU tensors through torch on the host.  When any
    row has a band, the sources first pass through ``band_mask`` into scratch allocated here; when any row has a room
    (``draws.reverberant``), they pass through the ``reverb`` stage before that, with the bank of ``reverb`` (the
    ``Reverb`` the ids were drawn from; without it such draws are a ValueError)."""
    nb, L, n = draws.batch, draws.length, draws.length + draws.shift
    dev = clean_src.device
    cs, three = _rows(clean_src, "clean_src", nb, n)
    ys, _ = _rows(noisy_src, "noisy_src", nb, n)
    if draws.reverberant:
        if not isinstance(reverb, Reverb):
            raise ValueError("augment.apply: the draws have rooms (rir >= 0): pass reverb=, the Reverb they were drawn from")
        clean_src, noisy_src = _reverb_stage(clean_src, noisy_src, draws, reverb.bank(dev))
        cs, ys = (t.stride(0) if nb > 1 else n for t in (clean_src, noisy_src))
    if draws.banded:
        clean_src, noisy_src = band_mask(clean_src, noisy_src, draws)
        cs, ys = (t.stride(0) if nb > 1 else n for t in (clean_src, noisy_src))
    if clean_out is None:
        clean_out = torch.empty((nb, 1, L) if three else (nb, L), dtype=torch.float32, device=dev)
    if noisy_out is None:
        noisy_out = torch.empty((nb, 1, L) if three else (nb, L), dtype=torch.float32, device=dev)
    co, _ = _rows(clean_out, "clean_out", nb, L)
    no, _ = _rows(noisy_out, "noisy_out", nb, L)
    if not (noisy_src.device == clean_out.device == noisy_out.device == dev):
        raise ValueError("augment.apply: all tensors must be on one device")
    spans = [_span(clean_src, cs, nb, n), _span(noisy_src, ys, nb, n)]
    outs = [_span(clean_out, co, nb, L), _span(noisy_out, no, nb, L)]
    if any(o[0] < s[1] and s[0] < o[1] for o in outs for s in spans) or (outs[0][0] < outs[1][1] and outs[1][0] < outs[0][1]):
        raise ValueError("augment.apply: the outputs must not overlap the sources or each other")
    if dev.type == "cpu":
        _host(clean_src, cs, noisy_src, ys, draws, clean_out, co, noisy_out, no)
        return clean_out, noisy_out
    hip.require_gpu(clean_src, noisy_src, clean_out, noisy_out)
    k = draws.columns()
    with torch.cuda.device(dev):
        table = torch.from_numpy(draws.pack(k)).to(dev)
        workspace = workspace_for(nb, L, dev) if draws.rescales else None
        launch(clean_src, cs, noisy_src, ys, nb, L, n, table, k, workspace, clean_out, co, noisy_out, no)
    return clean_out, noisy_out
