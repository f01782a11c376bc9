"""The mixing stage's arithmetic (include/cleanumamba_hip.h: cum_mix_pairs; training/mix.py) restated in NumPy, for
test_mix_host.py and test_mix_gpu.py: Python integers for the sums, f64 scalars, ``np.float32`` for the rest.

``fmaf(a, n, s)`` is written as an f64 multiply-add rounded once to f32.  The product of an f32 and a 16-bit value times
2^-15 is exact in f64; the sum with the 16-bit speech value is exact too unless a is below about 2^-13 of the values in
play, and then the f64 rounding can move the f32 result only where the exact sum lies within 2^-29 of an f32 tie."""
import math

import numpy as np

F32 = np.float32
TWO30 = 1073741824.0


def scalars(snr_db, level_db, activity_db):
    """(q, l, thr) as the host forms them, in double: 10^(snr / 10), 10^(level / 10) or NaN (keep), and
    floor(2^30 10^(activity / 10))."""
    q = 10.0 ** (float(snr_db) / 10.0)
    l = 10.0 ** (float(level_db) / 10.0) if math.isfinite(float(level_db)) else math.nan
    return q, l, int(math.floor(2.0 ** 30 * 10.0 ** (float(activity_db) / 10.0)))


def signals(speech, noise, n_speech, length):
    """S[t] = speech[t mod n_s], N[t] = noise[t], t < length, as int64 arrays."""
    n_s = min(max(int(n_speech), 1), length)
    t = np.arange(length)
    return np.asarray(speech)[t % n_s].astype(np.int64), np.asarray(noise)[:length].astype(np.int64)


def mixture(a32, S, N):
    """Step 6: m[t] = fmaf(a32, N[t] 2^-15, S[t] 2^-15), float32."""
    return (np.float64(F32(a32)) * (N.astype(np.float64) / 32768.0) + S.astype(np.float64) / 32768.0).astype(F32)


def outputs(a32, g32, S, N):
    """Step 8 from the two scalars: (clean, noisy), float32."""
    return F32(g32) * (S.astype(np.float64) / 32768.0).astype(F32), F32(g32) * mixture(a32, S, N)


def mix_row(speech, noise, n_speech, length, frame, thr, q, l, clip):
    """(clean, noisy, stats, facts) of one row.  stats: the 8 float32 of the ABI; facts: what the tests ask about the
    branches taken -- ``active_s`` / ``active_n`` (per-frame booleans), ``guard``, ``a``, ``g`` (the f64 values)."""
    length = int(length)
    frame = min(max(int(frame), 1), length)
    thr = min(max(int(thr), 0), 1 << 30)
    S, N = signals(speech, noise, n_speech, length)
    Ss = Snn = Ssn = 0
    act = {"s": [0, 0, []], "n": [0, 0, []]}             # sum of e_k, sum of m over the active frames; the flags
    for f0 in range(0, length, frame):
        f1 = min(f0 + frame, length)
        m = f1 - f0
        es = int((S[f0:f1] * S[f0:f1]).sum())
        en = int((N[f0:f1] * N[f0:f1]).sum())
        Ss, Snn, Ssn = Ss + es, Snn + en, Ssn + int((S[f0:f1] * N[f0:f1]).sum())
        for key, e in (("s", es), ("n", en)):
            active = e > thr * m
            act[key][2].append(active)
            if active:
                act[key][0] += e
                act[key][1] += m
    Ps = float(act["s"][0]) / float(act["s"][1]) if act["s"][1] > 0 else float(Ss) / float(length)
    Pn = float(act["n"][0]) / float(act["n"][1]) if act["n"][1] > 0 else float(Snn) / float(length)
    a = math.sqrt(Ps / (Pn * q)) if Ps > 0 and Pn > 0 and math.isfinite(q) and q > 0 else 1.0
    a32 = F32(a)
    A = float(a32)
    Em = (A * float(Snn) + 2.0 * float(Ssn)) * A + float(Ss)
    g = math.sqrt(l * float(length) * TWO30 / Em) if math.isfinite(l) and Em > 0 else 1.0
    g32 = F32(g)
    peak = F32(np.abs(mixture(a32, S, N)).max())
    guard = bool(F32(g32 * peak) > F32(clip))
    if guard:
        g32 = F32(F32(clip) / peak)
    clean, noisy = outputs(a32, g32, S, N)
    stats = np.array([a32, g32, Ps / TWO30, Pn / TWO30, peak, act["s"][1] / length, act["n"][1] / length,
                      1.0 if guard else 0.0], dtype=F32)
    facts = {"active_s": act["s"][2], "active_n": act["n"][2], "guard": guard, "a": a, "g": g,
             "n_s": min(max(int(n_speech), 1), length)}
    return clean, noisy, stats, facts


def mix_batch(speech, n_speech, noise, snr_db, level_db, activity_db=-50.0, frame=1600, clip=0.99):
    """Rows of (B, L) int16 arrays: (clean (B, L), noisy (B, L), stats (B, 8), [facts])."""
    speech, noise = np.asarray(speech), np.asarray(noise)
    rows = []
    for b in range(speech.shape[0]):
        q, l, thr = scalars(snr_db[b], level_db[b], activity_db)
        rows.append(mix_row(speech[b], noise[b], n_speech[b], speech.shape[1], frame, thr, q, l, clip))
    return (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows]),
            [r[3] for r in rows])
