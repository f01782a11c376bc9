"""The reverb stage of training/augment.py (include/cleanumamba_hip.h: cum_reverb_pairs) restated in f64,
for test_reverb_host.py and test_reverb_gpu.py.  Nothing here imports the code under test.

    h = taps of the row's response (float32, T of them, h[0] the direct path);  a row without one is the sources themselves
    Cr[t] = sum_{k = 0 .. min(t, T - 1)} h[k] C[t - k]        clean = Cr        noisy = (Y - C) + Cr        t in [0, n)

The bounds, with u = 2^-24 and ``s_b = max_t |C_b[t]| sum_k |h_b[k]|`` (no |Cr| can exceed s_b):

    |clean - ref| <= c u s_b
    |noisy - ref| <= (c + 1) u s_b + 2 u max_t |Y_b - C_b|

(the noisy row adds one rounding of the sum, at most u (s_b + max |Y - C|), and one of the difference).
``partitioned_f32`` is the CPU restatement that sets c: the same uniformly partitioned overlap-save (partitions and output
blocks of N / 2, spectra multiplied and added in ascending k) in float32 on scipy's pocketfft at the kernel's N = 4096 --
an FFT convolution that is not the code under test.  C_CPU is the worst ``|out - ref| / (u s_b)`` it gives over exactly the
cases of test_reverb_gpu.py that meet the oracle (``python tests/reverb_ref.py`` prints it), C = 4 x that, rounded up: the
kernel's radix-4 twiddle table and butterfly order are not pocketfft's.
"""
import numpy as np

U = 2.0 ** -24
N = 4096             # the kernel's FFT length; C_CPU holds for it alone
P = N // 2
T_MAX = 16384
C_CPU = 3.54         # measured: python tests/reverb_ref.py (N = 4096) gives 3.5305
C = 15               # 4 x C_CPU (14.2), rounded up

TAPS = [1, 2, P - 1, P, P + 1, 2 * P, 2 * P + 1, T_MAX]
LENGTHS = [1, 7, P - 1, P, P + 1, 2 * P + 1, 3 * P + 5]


DECAY = 400.0        # a decay_db that keeps every tap of a synthetic response (the default 60 cuts its last tenth)


def synth_raw(T, seed):
    """A raw synthetic response of T taps, f64: Gaussian noise decaying by 60 dB over its length, h[0] the peak."""
    rng = np.random.default_rng(seed)
    h = rng.standard_normal(T) * 10.0 ** (-3.0 * np.arange(T) / T)
    h[0] = 1.5 * max(1.0, np.abs(h).max())
    return h


def synth(T, seed):
    """The same prepared with ``decay_db = DECAY``: all T taps, unit energy, float32."""
    h = prepare(synth_raw(T, seed), decay_db=DECAY)
    assert h.shape == (T,)
    return h


def bank_raw():
    """One raw response of every length of TAPS, in that order."""
    return [synth_raw(T, 500 + i) for i, T in enumerate(TAPS)]


def bank():
    """The same as ``Reverb(bank_raw(), decay_db=DECAY).taps`` must hold them."""
    return [synth(T, 500 + i) for i, T in enumerate(TAPS)]


def raw_response(seed=3, pre=37, body=3000, tail=9000):
    """A raw measurement for the preparation rule: ``pre`` samples of weak noise, the direct path, a decaying body (60 dB
    over ``body`` samples), then a long tail 100 dB down: f64, not normalised."""
    rng = np.random.default_rng(seed)
    h = np.concatenate([1e-3 * rng.standard_normal(pre), [2.5],
                        rng.standard_normal(body - 1) * 10.0 ** (-3.0 * np.arange(1, body) / body),
                        1e-5 * rng.standard_normal(tail)])
    return h


def prepare(h, decay_db=60.0, max_taps=T_MAX):
    """The preparation rule in f64: from the first sample of the largest magnitude; up to the last sample t at which
    sum_{s >= t} h[s]^2 > 10^(-decay_db / 10) sum_s h[s]^2; at most min(max_taps, T_MAX) taps; unit energy; float32."""
    h = np.asarray(h, dtype=np.float64)
    i0 = 0
    for i in range(h.shape[0]):                          # (the first of equal peaks)
        if abs(h[i]) > abs(h[i0]):
            i0 = i
    h = h[i0:]
    total = float((h * h).sum())
    back = np.add.accumulate((h * h)[::-1])[::-1]
    last = int(np.nonzero(back > total * 10.0 ** (-decay_db / 10.0))[0].max())
    h = h[:last + 1][:min(int(max_taps), T_MAX)]
    return (h / np.sqrt((h * h).sum())).astype(np.float32)


def reference(C, Y, rows):
    """C, Y: float32 (B, n); rows: per row the float32 taps, or None (a copy).  Returns (clean, noisy, s, d): the f64
    results (B, n), the scales s_b and d_b = max_t |Y_b - C_b| (B,).  A copy row has s_b = 0: it must be the source's bits."""
    C, Y = np.asarray(C, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    n = C.shape[1]
    clean, noisy, s = np.empty_like(C), np.empty_like(Y), np.zeros(C.shape[0])
    for b, h in enumerate(rows):
        if h is None:
            clean[b], noisy[b] = C[b], Y[b]
            continue
        h = np.asarray(h, dtype=np.float64)
        clean[b] = np.convolve(C[b], h)[:n]
        noisy[b] = (Y[b] - C[b]) + clean[b]
        s[b] = np.abs(C[b]).max() * np.abs(h).sum()
    return clean, noisy, s, np.abs(Y - C).max(axis=1)


def ratios(got, want, s):
    """Per row, the worst |got - want| / (u s_b) (inf for an error on a row with s_b = 0)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want).max(axis=1)
    return np.where(s > 0, err / np.where(s > 0, U * s, 1.0), np.where(err > 0, np.inf, 0.0))


def check(got, Cs, Ys, rows, what="", c=None):
    """Assert both bounds of the module's docstring per element for got = (clean, noisy) as (B, n) arrays, and that a copy
    row is the source bit for bit; prints the worst ratios first and returns the clean rows' worst.  c: a number or one
    per row; default the module's C."""
    c = np.broadcast_to(np.asarray(C if c is None else c, dtype=np.float64), (len(rows),))
    clean, noisy, s, d = reference(Cs, Ys, rows)
    gc, gy = (np.asarray(g, dtype=np.float64) for g in got)
    assert gc.shape == clean.shape and gy.shape == noisy.shape, (what, gc.shape, clean.shape)
    assert np.isfinite(gc).all() and np.isfinite(gy).all(), (what, "not finite")
    r = ratios(gc, clean, s)
    print(f"reverb {what}: worst |clean - ref| / (2^-24 s_b) per row = {np.array2string(r, precision=2)} (allowed "
          f"{np.array2string(c, precision=0)})")
    assert (r <= c).all(), (what, "clean", r.tolist())
    err = np.abs(gy - noisy).max(axis=1)
    allowed = (c + 1) * U * s + 2 * U * d
    print(f"reverb {what}: worst |noisy - ref| / allowed per row = "
          f"{np.array2string(err / np.where(allowed > 0, allowed, 1.0), precision=3)}")
    assert (err <= allowed).all(), (what, "noisy", (err / np.where(allowed > 0, allowed, 1.0)).tolist())
    for b, h in enumerate(rows):
        if h is None:
            assert np.array_equal(got[0][b], Cs[b]) and np.array_equal(got[1][b], Ys[b]), (what, b, "the row is no copy")
    return float(r.max())


def pack(ids):
    """The int32 record table {rir, 0, 0, 0} of per-row ids."""
    out = np.zeros((len(ids), 4), dtype=np.int32)
    out[:, 0] = ids
    return out.reshape(-1)


# ---- the cases of test_reverb_gpu.py, shared with the measurement of C_CPU below ---------------------------------------
def rows(n, seed):
    """A (C, Y) pair of one row of n samples: Gaussian speech at 0.1, Y = C + Gaussian noise at 0.05."""
    rng = np.random.default_rng(seed)
    C = (0.1 * rng.standard_normal((1, n))).astype(np.float32)
    return C, (C + (0.05 * rng.standard_normal((1, n))).astype(np.float32)).astype(np.float32)


def case_signals(n, nb, seed):
    pairs = [rows(n, seed + b) for b in range(nb)]
    return np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])


def seam_cases():
    """[(name, n, ids, seed)]: for every response of ``bank()`` the seven lengths, each launch holding its row, the rows of
    two other responses and a row without one (-1), all n long."""
    cases = []
    for i, T in enumerate(TAPS):
        for n in LENGTHS:
            cases.append((f"T = {T} n = {n}", n, [i, (i + 1) % len(TAPS), (i + 3) % len(TAPS), -1], 1000 * i + n))
    return cases


IMPULSE_RIRS = [2, 4, 7]         # T = P - 1, P + 1 and T_MAX

# (name, n, ids, seed) of the other cases of test_reverb_gpu.py that meet the oracle
OTHER_CASES = {"forms": ("forms", P + 1, [4, 6, -1], 5), "bad ids": ("bad ids", 300, [-1, -1, -1, -1, 2], 12),
               "bad device table": ("bad device table", P + 9, [7, -1, 0, -1], 21),
               "composition": ("composition, the stage", 3500, [7, -1, 4, 2], 31)}


def impulse_case(r):
    """(n, ids, positions, C, Y, noise): four rows of response r, n = 3 P + 5, a unit impulse at 0, P - 1, P, n - 1 in the
    clean row; Y = C + noise with a known noise."""
    n = 3 * P + 5
    pos = [0, P - 1, P, n - 1]
    C = np.zeros((4, n), dtype=np.float32)
    C[np.arange(4), pos] = 1.0
    noise = (0.05 * np.random.default_rng(70 + r).standard_normal((4, n))).astype(np.float32)
    noise[np.arange(4), pos] = 0.0                       # (so that Y - C gives the noise back exactly)
    return n, [r] * 4, pos, C, (C + noise).astype(np.float32), noise


def partitioned_f32(x, h32, N=N):
    """One row filtered as the kernel does it, in float32 on pocketfft: the response in partitions of N / 2, each padded to
    N and transformed; input blocks [(j - 1) P, (j + 1) P); per output block the sum over k of X[m - k] H[k] in ascending
    k, one inverse, its second half kept."""
    import scipy.fft
    Ph, n, T = N // 2, x.shape[0], h32.shape[0]
    K, M = -(-T // Ph), -(-n // Ph)
    H = []
    for k in range(K):
        g = np.zeros(N, dtype=np.complex64)
        part = h32[k * Ph:(k + 1) * Ph]
        g[:part.shape[0]] = part
        H.append(scipy.fft.fft(g))
        assert H[-1].dtype == np.complex64
    xp = np.zeros((M + 1) * Ph, dtype=np.complex64)
    xp[Ph:Ph + n] = x.astype(np.float32)
    X = [scipy.fft.fft(xp[j * Ph:j * Ph + N]) for j in range(M)]
    out = np.zeros(M * Ph, dtype=np.float32)
    for m in range(M):
        acc = np.zeros(N, dtype=np.complex64)
        for k in range(min(K, m + 1)):
            acc = acc + X[m - k] * H[k]
        blk = scipy.fft.ifft(acc)
        assert blk.dtype == np.complex64
        out[m * Ph:(m + 1) * Ph] = blk.real[Ph:]
    return out[:n]


def measure_c_cpu():
    taps, worst = bank(), 0.0
    cases = [(name, ids, *case_signals(n, len(ids), seed)) for name, n, ids, seed in seam_cases() + list(OTHER_CASES.values())]
    for r in IMPULSE_RIRS:
        n, ids, _, Cs, Ys, _ = impulse_case(r)
        cases.append((f"impulses of response {r}", ids, Cs, Ys))
    for name, ids, Cs, Ys in cases:
        hs = [taps[r] if r >= 0 else None for r in ids]
        clean, _, s, _ = reference(Cs, Ys, hs)
        for b, h in enumerate(hs):
            if h is not None:
                got = partitioned_f32(Cs[b], h)
                worst = max(worst, np.abs(got - clean[b]).max() / (U * s[b]))
        print(f"{name}: worst so far {worst:.3f}")
    return worst


if __name__ == "__main__":
    print("C_CPU =", measure_c_cpu())
