"""The band-mask stage of training/augment.py (include/cleanumamba_hip.h: cum_band_mask_pairs) restated in
f64, for test_bandmask_host.py and test_bandmask_gpu.py.  Nothing here imports the code under test.

    mel(f) = 2595 log10(1 + f / 700);  edges e_j = mel^-1(linspace(mel(min_freq), mel(sample_rate / 2), bands));
    c_j = e_j / sample_rate in f64, rounded to f32;  W = int(2 / c_lo)
    w[k] = 0.54 - 0.46 cos(pi (k + W) / W),  lp_c[k] = 2 c sinc(2 c k) w[k],  h[k] = [k == 0] + lp_lo[k] - lp_hi[k]
    out[b, t] = sum_k h[k] x[b, t - k],  x zero outside [0, n)

The bound: ``|out - ref| <= (c + 1) 2^-24 s_b`` with ``s_b = max_t |x_b[t]| sum_k |h_b[k]|`` (no output can exceed s_b);
the ``+ 1`` covers a tap that rounds differently after another f64 sine.  ``overlap_save_f32`` is the CPU restatement that
sets c: f32 overlap-save at the kernel's N on scipy's pocketfft, which keeps float32 -- an FFT convolution that is not
the code under test.  C_CPU is the worst ``|out - ref| / (2^-24 s_b)`` it gives over exactly the cases of
test_bandmask_gpu.py (``python tests/bandmask_ref.py`` prints it), C = 4 x that, rounded up: the kernel's radix-4
twiddle table and butterfly order are not pocketfft's.
"""
import numpy as np

U = 2.0 ** -24
W_MAX = 1600
C_CPU = 4.99         # measured: python tests/bandmask_ref.py (N = 4096)
C = 20               # 4 x C_CPU (19.95), rounded up


def mel_edges(bands=120, min_freq=40.0, sample_rate=16000):
    """c_j, j = 0..bands-1, as float32."""
    mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)      # noqa: E731
    m = np.linspace(mel(float(min_freq)), mel(sample_rate / 2.0), int(bands))
    return ((700.0 * (10.0 ** (m / 2595.0) - 1.0)) / sample_rate).astype(np.float32)


def half_width(c_lo):
    return int(2.0 / float(np.float32(c_lo)))


def band(lo, hi, edges=None):
    """(W, c_lo, c_hi) of the band between edges lo and hi of the default configuration."""
    e = mel_edges() if edges is None else edges
    return half_width(e[lo]), e[lo], e[hi]


def taps(W, c_lo, c_hi):
    """h[-W..W]: evaluated in f64 from the f32 cutoffs, rounded to f32, returned widened to f64."""
    W, lo, hi = int(W), float(np.float32(c_lo)), float(np.float32(c_hi))
    k = np.arange(-W, W + 1, dtype=np.float64)
    w = 0.54 - 0.46 * np.cos(np.pi * (k + W) / W)
    h = 2.0 * lo * np.sinc(2.0 * lo * k) * w - 2.0 * hi * np.sinc(2.0 * hi * k) * w
    h[W] += 1.0
    return h.astype(np.float32).astype(np.float64)


def reference(C, Y, bands):
    """C, Y: float32 (B, n); bands: per row (W, c_lo, c_hi).  Returns (clean, noisy, s_clean, s_noisy): the filtered rows
    in f64 (B, n) and the per-row scales s_b (B,).  A row with W = 0 is the source itself (s_b = max |x|)."""
    C, Y = np.asarray(C, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    outs, scales = [], []
    for X in (C, Y):
        out, s = np.empty_like(X), np.empty(X.shape[0])
        for b, (W, lo, hi) in enumerate(bands):
            W = int(W)
            if W == 0:
                out[b], s[b] = X[b], np.abs(X[b]).max()
                continue
            h = taps(W, lo, hi)
            out[b] = np.convolve(X[b], h)[W:W + X.shape[1]]
            s[b] = np.abs(X[b]).max() * np.abs(h).sum()
        outs.append(out)
        scales.append(s)
    return outs[0], outs[1], scales[0], scales[1]


def check(got, want, s, what="", c=C):
    """Assert ``|got - want| <= (c + 1) 2^-24 s_b`` per element for (B, n) results; prints the worst ratio to 2^-24 s_b
    first and returns it."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), (what, "not finite")
    err = np.abs(got - want).max(axis=1)
    ratio = np.where(s > 0, err / np.where(s > 0, U * s, 1.0), np.where(err > 0, np.inf, 0.0))
    print(f"bandmask {what}: worst |out - ref| / (2^-24 s_b) per row = {np.array2string(ratio, precision=2)}"
          f" (allowed {c + 1})")
    assert (ratio <= c + 1).all(), (what, ratio.tolist())
    return float(ratio.max())


def pack(bands):
    """The int32 record table {W, c_lo bits, c_hi bits, 0} of per-row (W, c_lo, c_hi)."""
    out = np.zeros((len(bands), 4), dtype=np.int32)
    for b, (W, lo, hi) in enumerate(bands):
        out[b, 0] = W
        out[b, 1:3] = np.array([lo, hi], dtype=np.float32).view(np.int32)
    return out.reshape(-1)


# ---- the cases of test_bandmask_gpu.py, shared with the measurement of C_CPU below -------------------------------------
BANDS = [(0, 23), (5, 20), (60, 80), (100, 119), (119, 119)]
IMPULSE_BANDS = [(0, 23), (60, 80), (100, 119)]


def seam_lengths(W, N):
    V = N - 2 * W
    return [1, 7, W, V - 1, V, V + 1, 2 * V + 1, 3 * V + 5]


def rows(n, seed):
    """A (C, Y) pair of one row of n samples: Gaussian speech at 0.1, Y = C + Gaussian noise at 0.05."""
    rng = np.random.default_rng(seed)
    C = (0.1 * rng.standard_normal((1, n))).astype(np.float32)
    return C, (C + (0.05 * rng.standard_normal((1, n))).astype(np.float32)).astype(np.float32)


def seam_cases(N):
    """[(name, n, [(W, c_lo, c_hi)] per row, seed)]: for every band its eight lengths, each launch holding the band's row,
    one row of every other band and a W = 0 row, all n long."""
    cases = []
    for i, (lo, hi) in enumerate(BANDS):
        for n in seam_lengths(band(lo, hi)[0], N):
            others = [band(*p) for p in BANDS if p != (lo, hi)]
            cases.append((f"band ({lo}, {hi}) n = {n}", n, [band(lo, hi)] + others + [(0, 0.0, 0.0)], 1000 * i + n))
    return cases


def largest_case(N):
    """W = 1600 built by hand (the default edges never ask for it) at n = 2 V + 1."""
    e = mel_edges()
    return "W = 1600", 2 * (N - 2 * W_MAX) + 1, [(W_MAX, e[0], e[23]), (W_MAX, np.float32(0.00125), e[5])], 77


def case_signals(n, nb, seed):
    pairs = [rows(n, seed + b) for b in range(nb)]
    return np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])


def impulse_case(lo, hi, N):
    """(n, bands, positions, C, Y): four rows of one band, n = 2 V + 1, a unit impulse at 0, V - 1, V, n - 1 in the clean
    row and its negative half in the noisy row."""
    W, c_lo, c_hi = band(lo, hi)
    V = N - 2 * W
    n = 2 * V + 1
    pos = [0, V - 1, V, n - 1]
    C = np.zeros((4, n), dtype=np.float32)
    C[np.arange(4), pos] = 1.0
    return n, [(W, c_lo, c_hi)] * 4, pos, C, (-0.5 * C).astype(np.float32)


def overlap_save_f32(x, y, W, h32, N):
    """Both rows filtered as the kernel does it, in float32 on pocketfft: blocks of N samples from j V - W, z = x + i y,
    one forward transform, the product with the f32 spectrum of the circularly placed taps, one inverse."""
    import scipy.fft
    n, V = x.shape[0], N - 2 * W
    g = np.zeros(N, dtype=np.complex64)
    g[np.arange(-W, W + 1) % N] = h32
    G = scipy.fft.fft(g)
    assert G.dtype == np.complex64
    zp = np.zeros(n + 2 * N, dtype=np.complex64)
    zp[N:N + n] = x.astype(np.float32) + 1j * y.astype(np.float32)
    out = np.zeros(n, dtype=np.complex64)
    for j in range(-(-n // V)):
        blk = scipy.fft.ifft(scipy.fft.fft(zp[N + j * V - W:N + j * V - W + N]) * G)
        assert blk.dtype == np.complex64
        t1 = min(j * V + V, n)
        out[j * V:t1] = blk[W:W + t1 - j * V]
    return out.real, out.imag


def measure_c_cpu(N=4096):
    worst = 0.0
    cases = [(name, bands, *case_signals(n, len(bands), seed)) for name, n, bands, seed in seam_cases(N) + [largest_case(N)]]
    for lo, hi in IMPULSE_BANDS:
        n, bands, _, C, Y = impulse_case(lo, hi, N)
        cases.append((f"impulses ({lo}, {hi})", bands, C, Y))
    for name, bands, C, Y in cases:
        rc, ry, sc, sy = reference(C, Y, bands)
        for b, (W, lo, hi) in enumerate(bands):
            if W == 0:
                continue
            gc, gy = overlap_save_f32(C[b], Y[b], W, taps(W, lo, hi).astype(np.float32), N)
            r = max(np.abs(gc - rc[b]).max() / (U * sc[b]), np.abs(gy - ry[b]).max() / (U * sy[b]))
            worst = max(worst, r)
        print(f"{name}: worst so far {worst:.3f}")
    return worst


if __name__ == "__main__":
    print("C_CPU =", measure_c_cpu())
