"""The extended speech metrics of cleanumamba_amd.util.metrics restated in f64 numpy: the specification the kernels are
tested against, and the seeded inputs of those tests.

  * snr, si_sdr: overall SNR and scale-invariant SDR (Le Roux, Wisdom, Erdogan, Hershey, "SDR - half-baked or well
    done?", ICASSP 2019; no mean removal), from exact integer sums;
  * estoi: extended STOI (Jensen & Taal, "An algorithm for predicting the intelligibility of speech masked by modulated
    noise maskers", IEEE/ACM TASLP 24(11), 2016) on the front end of tests/stoi_ref.py;
  * cep_frames / cep_dist: LPC cepstrum distance (Kitawaki, Nagabuchi, Itoh 1988) and
    fwseg_frames / fwseg_snr: frequency-weighted segmental SNR (Tribolet et al. 1978), both as evaluated by Hu & Loizou,
    "Evaluation of objective quality measures for speech enhancement", IEEE TASLP 16(1), 2008, on the frames, window,
    order-16 LPC and 25 critical bands of the project's other frame metrics.

These are restatements of the published algorithms.  NOT verified against pystoi, pysepm or torchmetrics: none of them is
installed where this was written, and nothing has been compared with them.  Known deviation from pystoi: it adds
eps-sized random noise to the segments before each eSTOI normalisation; here every norm gets an additive eps instead.
x is the clean clip and y the processed clip, both as their int16 values.
"""
import math

import numpy as np
from scipy.signal import lfilter

import stoi_ref

EPS = np.finfo(float).eps
WIN, HOP, ORDER, NFFT = 480, 120, 16, 1024


# ---- snr, si_sdr
def sums(x, y):
    """(sum x^2, sum y^2, sum x y) as Python integers"""
    x = [int(v) for v in np.asarray(x).reshape(-1)]
    y = [int(v) for v in np.asarray(y).reshape(-1)]
    return sum(a * a for a in x), sum(b * b for b in y), sum(a * b for a, b in zip(x, y))


def snr(x, y):
    sxx, syy, sxy = sums(x, y)
    d = sxx - 2 * sxy + syy
    if sxx == 0:
        return float("nan")
    if d == 0:
        return float("inf")
    return 10.0 * math.log10(sxx / d)                     # int / int: the correctly rounded quotient


def si_sdr(x, y):
    sxx, syy, sxy = sums(x, y)
    if sxx == 0:
        return float("nan")
    if sxy == 0:
        return float("-inf")
    q = sxx * syy - sxy * sxy                             # exact, >= 0 (Cauchy-Schwarz)
    if q == 0:
        return float("inf")
    return 10.0 * math.log10(sxy * sxy / q)


# ---- eSTOI
def _row_col_normalise(m):
    """(segments, 15 bands, 30 frames): rows to zero mean and unit norm over the frames, then columns over the bands"""
    m = m - m.mean(axis=2, keepdims=True)
    m = m / (np.linalg.norm(m, axis=2, keepdims=True) + EPS)
    m = m - m.mean(axis=1, keepdims=True)
    return m / (np.linalg.norm(m, axis=1, keepdims=True) + EPS)


def estoi(x, y, fs):
    S = stoi_ref
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    if fs != S.FS:
        x, y = S.resample(x, S.FS, fs), S.resample(y, S.FS, fs)
    x, y = S.remove_silent_frames(x, y)
    xs = np.fft.rfft(S.frames(x), n=S.NFFT).T
    ys = np.fft.rfft(S.frames(y), n=S.NFFT).T
    if xs.shape[-1] < S.N:
        return 1e-5
    obm = S.third_octave()
    xt = np.sqrt(obm @ np.square(np.abs(xs)))
    yt = np.sqrt(obm @ np.square(np.abs(ys)))
    xseg = np.array([xt[:, m - S.N:m] for m in range(S.N, xt.shape[1] + 1)])
    yseg = np.array([yt[:, m - S.N:m] for m in range(S.N, yt.shape[1] + 1)])
    xn, yn = _row_col_normalise(xseg), _row_col_normalise(yseg)
    return float(np.sum(xn * yn) / S.N / xn.shape[0])


# ---- frames of the 16 kHz frame metrics
def frame_window():
    return 0.5 * (1 - np.cos(2 * math.pi * np.arange(1, WIN + 1) / (WIN + 1)))


def frames(x):
    x = np.asarray(x, np.float64)
    n = max((x.size - WIN) // HOP, 0)
    if n == 0:
        return np.zeros((0, WIN))
    return np.stack([x[f * HOP:f * HOP + WIN] for f in range(n)])


def lpc(frame):
    """A = [1, a_1 .. a_16] of the order-16 autocorrelation LPC (Levinson-Durbin); NaN for an all-zero frame"""
    R = np.array([np.dot(frame[:WIN - k], frame[k:]) for k in range(ORDER + 1)])
    a = np.ones(ORDER)
    E = R[0]
    with np.errstate(all="ignore"):
        for i in range(ORDER):
            prev = a.copy()
            rc = (R[i + 1] - np.dot(prev[:i], R[i:0:-1])) / E
            a[i] = rc
            a[:i] = prev[:i] - prev[:i][::-1] * rc
            E = (1 - rc * rc) * E
    return np.concatenate([[1.0], -a])


def cepstrum(A):
    """the cepstrum c_1 .. c_16 of 1 / A(z)"""
    c = np.zeros(ORDER + 1)
    for k in range(1, ORDER + 1):
        c[k] = -A[k] - sum(i * c[i] * A[k - i] for i in range(1, k)) / k
    return c[1:]


def cep_frames(x, y):
    w = frame_window()
    out = []
    for fx, fy in zip(frames(x), frames(y)):
        d = cepstrum(lpc(fx * w)) - cepstrum(lpc(fy * w))
        v = 10.0 / math.log(10.0) * math.sqrt(2.0 * float(np.sum(d * d))) if not np.isnan(d).any() else float("nan")
        out.append(v if math.isnan(v) else min(max(v, 0.0), 10.0))
    return np.array(out)


def fwseg_frames(x, y):
    from cleanumamba_amd.util.metrics import crit_band_table
    tab, wts = crit_band_table()
    w = frame_window()
    out = []
    for fx, fy in zip(frames(x), frames(y)):
        A = np.abs(np.fft.rfft(fx / 32768.0 * w, NFFT))[:NFFT // 2]
        B = np.abs(np.fft.rfft(fy / 32768.0 * w, NFFT))[:NFFT // 2]
        A = A / (np.sum(A) + EPS)
        B = B / (np.sum(B) + EPS)
        num = den = 0.0
        for lo, cnt, o in tab:
            ce = float(np.dot(wts[o:o + cnt], A[lo:lo + cnt]))
            pe = float(np.dot(wts[o:o + cnt], B[lo:lo + cnt]))
            if ce > 0:
                W = ce ** 0.2
                num += W * 10.0 * math.log10(ce * ce / max((ce - pe) ** 2, EPS))
                den += W
        out.append(min(max(num / den, -10.0), 35.0) if den > 0 else float("nan"))
    return np.array(out)


def cep_dist(x, y):
    """mean of the lowest round(0.95 n) frame values, NaN sorting last and dropped (NaN if nothing is left)"""
    v = np.sort(cep_frames(x, y))
    v = v[:round(v.size * 0.95)]
    v = v[~np.isnan(v)]
    return float(np.mean(v)) if v.size else float("nan")


def fwseg_snr(x, y):
    v = fwseg_frames(x, y)
    v = v[~np.isnan(v)]
    return float(np.mean(v)) if v.size else float("nan")


# ---- seeded test inputs
def q16(x):
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def voiced(n, rng, f0=140.0, rate=16000, amp=8000.0):
    """the harmonic signal of tools/make_golden_metrics.py: a slow pitch glide under a syllable-rate envelope"""
    t = np.arange(n) / rate
    ph = 2 * np.pi * np.cumsum(f0 * (1 + 0.1 * np.sin(2 * np.pi * 0.7 * t))) / rate
    x = sum(np.sin(k * ph + rng.uniform(0, 2 * np.pi)) / k for k in range(1, 25))
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 3.1 * t + rng.uniform(0, 6))
    return amp * env * x / np.max(np.abs(x))


def _at_db(noise, ref, db):
    """noise scaled to lie db below ref in power"""
    return noise * np.sqrt(np.mean(ref ** 2) / np.mean(noise ** 2) / 10 ** (db / 10))


def speech_like_pairs(n=24000, seed=20261021):
    """[(name, clean int16, processed int16)]: voiced signal at amplitude 6000 over a coloured noise floor 20 dB below it
    (white noise through 1 / (1 - 0.9 z^-1): it keeps the LPC well conditioned), then coloured noise
    (1 / (1 - 0.7 z^-1)) at 10 and 25 dB SNR, and a spectral tilt 1 - 0.3 z^-1"""
    rng = np.random.default_rng(seed)
    v = voiced(n, rng, amp=6000.0)
    clean = v + _at_db(lfilter([1.0], [1.0, -0.9], rng.standard_normal(n)), v, 20.0)
    pairs = []
    for db in (10, 25):
        noise = _at_db(lfilter([1.0], [1.0, -0.7], rng.standard_normal(n)), clean, float(db))
        pairs.append((f"coloured_snr{db}", q16(clean), q16(clean + noise)))
    pairs.append(("tilt", q16(clean), q16(lfilter([1.0, -0.3], [1.0], clean))))
    return pairs
