"""The arithmetic of training/augment.py (include/cleanumamba_hip.h: cum_augment_pairs) restated in f64, for
test_augment_host.py and test_augment_gpu.py.

For every output element ``reference`` returns the value and M, the sum of the absolute values of all terms that entered
it.  The bound used throughout is

    |out - ref| <= (n_terms + 8) 2^-24 M,      n_terms = the row's tap count + N_OPS

-- the standard bound of a fixed-order f32 chain (n roundings of relative size 2^-24, each on a partial sum no larger
than M), derived, not tuned.  N_OPS = 8 counts the roundings outside the tap chain that an f32 implementation with fused
multiply-adds makes on the way to noisy': Y - C, n0 + rn, 1 - kappa, (1 - kappa) rc + ., kappa rc + c0, a itself (from
f64 sums: one rounding to f32), a n1 + c1, and the gain.  An implementation that rounds a product before adding it
spends at most one more per product; the "+ 8" holds that.  The oracle starts from the f32 / int32 values of the draws.
"""
import numpy as np

N_OPS = 8
U = 2.0 ** -24


def reference(C, Y, draws):
    """C, Y: float32 (B, L + S) arrays.  Returns a dict of f64 arrays: clean, noisy, M_clean, M_noisy (B, L); c1, n1 (B, L);
    a, n_terms (B,)."""
    C, Y = np.asarray(C, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    B, L = draws.batch, draws.length
    assert C.shape == Y.shape == (B, L + draws.shift)
    out = {k: np.zeros((B, L)) for k in ("clean", "noisy", "M_clean", "M_noisy", "c1", "n1")}
    out["a"], out["n_terms"] = np.ones(B), np.zeros(B)
    for b in range(B):
        p, oc, on = int(draws.perm[b]), int(draws.off_clean[b]), int(draws.off_noise[b])
        c0 = C[b, oc:oc + L]
        n0 = Y[p, on:on + L] - C[p, on:on + L]
        m_c0, m_n0 = np.abs(c0), np.abs(Y[p, on:on + L]) + np.abs(C[p, on:on + L])
        rc, rn, m_rc, m_rn = np.zeros(L), np.zeros(L), np.zeros(L), np.zeros(L)
        for k in range(int(draws.n_taps[b])):
            d, g = int(draws.delay[b, k]), float(draws.tap_gain[b, k])
            if 1 <= d < L:
                rc[d:] += g * c0[:L - d]
                rn[d:] += g * n0[:L - d]
                m_rc[d:] += abs(g) * m_c0[:L - d]
                m_rn[d:] += abs(g) * m_n0[:L - d]
        kappa, gain, snr = float(draws.kappa[b]), float(draws.gain[b]), float(draws.snr_db[b])
        c1 = c0 + kappa * rc
        n1 = n0 + rn + (1.0 - kappa) * rc
        m_c1 = m_c0 + abs(kappa) * m_rc
        m_n1 = m_n0 + m_rn + abs(1.0 - kappa) * m_rc
        ec, en = float(np.sum(c1 * c1)), float(np.sum(n1 * n1))
        a = 1.0
        if np.isfinite(snr) and ec > 0 and en > 0:
            a = np.sqrt(ec / (en * 10.0 ** (snr / 10.0)))
        out["c1"][b], out["n1"][b], out["a"][b] = c1, n1, a
        out["clean"][b], out["noisy"][b] = gain * c1, gain * (c1 + a * n1)
        out["M_clean"][b], out["M_noisy"][b] = abs(gain) * m_c1, abs(gain) * (m_c1 + a * m_n1)
        out["n_terms"][b] = int(draws.n_taps[b]) + N_OPS
    return out


def bounds(ref):
    """(bound of clean', bound of noisy') per element."""
    scale = (ref["n_terms"] + 8)[:, None] * U
    return scale * ref["M_clean"], scale * ref["M_noisy"]


def check(clean, noisy, ref, what=""):
    """Assert the per-element bound for (B, L) results; prints the worst ratio error / bound first."""
    clean, noisy = np.asarray(clean, dtype=np.float64), np.asarray(noisy, dtype=np.float64)
    worst = 0.0
    for name, got, want, bound in zip(("clean", "noisy"), (clean, noisy), (ref["clean"], ref["noisy"]), bounds(ref)):
        assert got.shape == want.shape, (what, name, got.shape, want.shape)
        assert np.isfinite(got).all(), (what, name, "not finite")
        err = np.abs(got - want)
        ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
        worst = max(worst, ratio)
        print(f"augment {what} {name}: worst |out - ref| / bound = {ratio:.4f}")
        assert (err <= bound).all(), (what, name, ratio)
    return worst


def signals(B, n, seed, silent_clean=(), silent_noise=()):
    """Speech-level float32 (C, Y) of shape (B, n): Y = C + noise; rows in silent_clean have C = 0, rows in silent_noise
    have Y = C."""
    rng = np.random.default_rng(seed)
    C = (0.1 * rng.standard_normal((B, n))).astype(np.float32)
    N = (0.05 * rng.standard_normal((B, n))).astype(np.float32)
    for b in silent_clean:
        C[b] = 0
    for b in silent_noise:
        N[b] = 0
    return C, (C + N).astype(np.float32)


def make_draws(L, S, perm, off_clean=None, off_noise=None, snr_db=None, gain=None, kappa=0.1, taps=None):
    """AugmentDraws from plain lists; taps: per row a list of (delay, gain)."""
    from cleanumamba_amd.training.augment import K_MAX, AugmentDraws
    B = len(perm)
    delay, tap_gain, n_taps = np.zeros((B, K_MAX), np.int32), np.zeros((B, K_MAX), np.float32), np.zeros(B, np.int32)
    for b, row in enumerate(taps or [[]] * B):
        n_taps[b] = len(row)
        if row:
            delay[b, :len(row)], tap_gain[b, :len(row)] = zip(*row)
    zeros = np.zeros(B, np.int32)
    return AugmentDraws(L, S, perm, zeros if off_clean is None else off_clean, zeros if off_noise is None else off_noise,
                        np.full(B, np.nan) if snr_db is None else snr_db, np.ones(B) if gain is None else gain,
                        np.full(B, kappa), n_taps, delay, tap_gain)


def snr_check(clean, noisy, ref, draws):
    """For rows with a finite drawn SNR: the achieved SNR of (noisy' - clean') against clean', in f64, equals the drawn
    one within what the per-element bounds allow: with x the reference and e <= bound the error of an element, the
    energy moves by at most sum(2 |x| e + e^2), and d(10 log10 E) = (10 / ln 10) dE / E."""
    clean, noisy = np.asarray(clean, dtype=np.float64), np.asarray(noisy, dtype=np.float64)
    b_clean, b_noisy = bounds(ref)
    rows = 0
    for b in range(draws.batch):
        snr = float(draws.snr_db[b])
        x_c, x_n = ref["clean"][b], ref["noisy"][b] - ref["clean"][b]
        e_c, e_n = float(np.sum(x_c ** 2)), float(np.sum(x_n ** 2))
        if not np.isfinite(snr) or e_c == 0 or e_n == 0:
            continue
        rows += 1
        got = 10 * np.log10(np.sum(clean[b] ** 2) / np.sum((noisy[b] - clean[b]) ** 2))
        d_c = np.sum(2 * np.abs(x_c) * b_clean[b] + b_clean[b] ** 2) / e_c
        eb = b_clean[b] + b_noisy[b]
        d_n = np.sum(2 * np.abs(x_n) * eb + eb ** 2) / e_n
        tol = 10 / np.log(10) * (d_c + d_n) + 1e-12 * max(1.0, abs(snr))        # (+ the f64 of this function itself)
        print(f"augment snr row {b}: drawn {snr:.6f} dB, achieved {got:.6f} dB, tolerance {tol:.3e}")
        assert abs(got - snr) <= tol, (b, snr, got, tol)
    return rows
