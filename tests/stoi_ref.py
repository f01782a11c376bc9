"""STOI (Taal, Hendriks, Heusdens, Jensen, "An algorithm for intelligibility prediction of time-frequency weighted noisy
speech", IEEE TASLP 19(7), 2011) restated in f64 numpy / scipy, following the published algorithm and the conventions of
the pystoi package the reference calls (python_eval.py:123, extended=False).

NOT verified against pystoi itself: pystoi is not installed where this was written.  The conventions taken over are:
resampling to 10 kHz by scipy's polyphase resampler with an Octave-style Kaiser-windowed sinc; 256-sample frames, hop
128, window hanning(258)[1:-1]; frame start positions range(0, len - 256, 128) for both the silent-frame removal and the
STFT; silent frames are those more than 40 dB below the loudest clean frame, and the kept windowed frames are
overlap-added back; 512-point FFT; 15 one-third-octave bands from 150 Hz on the nearest FFT bins; 30-frame segments,
beta = -15 dB clipping; fewer than 30 STFT frames gives 1e-5.
"""
import numpy as np
from scipy.signal import resample_poly

FS, N_FRAME, NFFT, NUMBAND, MINFREQ, N, BETA, DYN_RANGE = 10000, 256, 512, 15, 150, 30, -15.0, 40.0
EPS = np.finfo(np.float64).eps


def third_octave(fs=FS, nfft=NFFT, num_bands=NUMBAND, min_freq=MINFREQ):
    f = np.linspace(0, fs, nfft + 1)[: nfft // 2 + 1]
    k = np.arange(num_bands, dtype=float)
    lo = min_freq * np.power(2.0, (2 * k - 1) / 6)
    hi = min_freq * np.power(2.0, (2 * k + 1) / 6)
    obm = np.zeros((num_bands, len(f)))
    for i in range(num_bands):
        obm[i, np.argmin(np.square(f - lo[i])):np.argmin(np.square(f - hi[i]))] = 1
    return obm


def resample_filter(p, q):
    g = np.gcd(p, q)
    up, down = p // g, q // g
    stop = 1.0 / (2 * max(up, down))
    rej = 60.0
    L = int(np.ceil((rej - 8) / (28.714 * stop / 10)))
    t = np.arange(-L, L + 1)
    h = np.kaiser(2 * L + 1, 0.1102 * (rej - 8.7)) * 2 * up * stop * np.sinc(2 * stop * t)
    return h / np.sum(h)


def resample(x, p, q):
    return resample_poly(x, p, q, window=resample_filter(p, q))


def frames(x, hop=N_FRAME // 2):
    w = np.hanning(N_FRAME + 2)[1:-1]
    return np.array([w * x[i:i + N_FRAME] for i in range(0, len(x) - N_FRAME, hop)]).reshape(-1, N_FRAME)


def overlap_add(fr, hop=N_FRAME // 2):
    if len(fr) == 0:
        return np.zeros(0)
    out = np.zeros((len(fr) - 1) * hop + N_FRAME)
    for i, f in enumerate(fr):
        out[i * hop:i * hop + N_FRAME] += f
    return out


def remove_silent_frames(x, y):
    xf, yf = frames(x), frames(y)
    if len(xf) == 0:
        return np.zeros(0), np.zeros(0)
    e = 20 * np.log10(np.linalg.norm(xf, axis=1) + EPS)
    mask = (np.max(e) - DYN_RANGE - e) < 0
    return overlap_add(xf[mask]), overlap_add(yf[mask])


def stoi(x, y, fs):
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    if fs != FS:
        x, y = resample(x, FS, fs), resample(y, FS, fs)
    x, y = remove_silent_frames(x, y)
    xs = np.fft.rfft(frames(x), n=NFFT).T
    ys = np.fft.rfft(frames(y), n=NFFT).T
    if xs.shape[-1] < N:
        return 1e-5
    obm = third_octave()
    xt = np.sqrt(obm @ np.square(np.abs(xs)))
    yt = np.sqrt(obm @ np.square(np.abs(ys)))
    xseg = np.array([xt[:, m - N:m] for m in range(N, xt.shape[1] + 1)])
    yseg = np.array([yt[:, m - N:m] for m in range(N, yt.shape[1] + 1)])
    nc = np.linalg.norm(xseg, axis=2, keepdims=True) / (np.linalg.norm(yseg, axis=2, keepdims=True) + EPS)
    yp = np.minimum(yseg * nc, xseg * (1 + 10 ** (-BETA / 20)))
    yp = yp - yp.mean(axis=2, keepdims=True)
    xs_ = xseg - xseg.mean(axis=2, keepdims=True)
    yp /= np.linalg.norm(yp, axis=2, keepdims=True) + EPS
    xs_ /= np.linalg.norm(xs_, axis=2, keepdims=True) + EPS
    return float(np.sum(yp * xs_) / (xs_.shape[0] * xs_.shape[1]))
