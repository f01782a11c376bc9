"""The resampler's definition in f64 (helper of test_resample_host.py, test_resample_gpu.py): the direct sum

    y[m] = sum over n in [0, L) with 0 <= m down - n up + H <= 2H  of  x[n] h[m down - n up + H],   n_out = ceil(L up / down)

vectorised per output, and A[m] = sum |x[n]| |h[..]|, the scale of the rounding bound of an f32 evaluation."""
import numpy as np


def resample_ref(x, h, up, down, m0=0, m1=None):
    """x: (L,) samples (any real dtype, taken as they are); h: the 2H + 1 taps.  -> (y, A) f64 for outputs [m0, m1)."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    L, H = len(x), (len(h) - 1) // 2
    K = -(-len(h) // up)
    n_out = -(-L * up // down)
    m1 = n_out if m1 is None else m1
    y, A = np.zeros(m1 - m0), np.zeros(m1 - m0)
    j = np.arange(K)[None, :]
    for lo in range(m0, m1, 4096):
        m = np.arange(lo, min(lo + 4096, m1))[:, None]
        c = m * down + H
        n = c // up - j
        t = c % up + j * up
        ok = (n >= 0) & (n < L) & (t <= 2 * H)
        terms = np.where(ok, x[np.clip(n, 0, max(L - 1, 0))] * h[np.clip(t, 0, 2 * H)], 0.0) if L else np.zeros(n.shape)
        y[lo - m0:lo - m0 + len(m)] = terms.sum(1)
        A[lo - m0:lo - m0 + len(m)] = np.abs(terms).sum(1)
    return y, A
