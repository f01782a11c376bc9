"""Fixtures of the speech metrics (cleanumamba_amd/util/metrics.py).  BUILD MACHINE ONLY: it reads the reference checkout.

The reference's src/util/python_eval.py is imported unmodified, with ``sys.modules`` stand-ins for pesq, pystoi and
tqdm (neither pesq nor pystoi is installed; the functions used here never call them).  Writes tests/golden/metrics.npz:
int16 clean / processed pairs, the reference's per-frame ``wss``, ``llr`` and segmental ``snr`` outputs, and the per-clip
``wss_dist``, ``llr_mean`` and ``segSNR`` of eval_waveform's recipe (python_eval.py:86-104).
Usage: python tools/make_golden_metrics.py [reference root]
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "metrics.npz")


def load_python_eval(ref_root):
    for name, attr in (("pesq", "pesq"), ("pystoi", "stoi")):
        m = types.ModuleType(name)
        setattr(m, attr, lambda *a, **k: float("nan"))
        sys.modules.setdefault(name, m)
    tq = types.ModuleType("tqdm")
    tq.tqdm = lambda it, *a, **k: it
    sys.modules.setdefault("tqdm", tq)
    path = os.path.join(ref_root, "src", "util", "python_eval.py")
    spec = importlib.util.spec_from_file_location("ref_python_eval", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def voiced(n, rng, f0=140.0, rate=16000, amp=8000.0):
    """harmonic signal with a slow pitch glide and a syllable-rate envelope"""
    t = np.arange(n) / rate
    ph = 2 * np.pi * np.cumsum(f0 * (1 + 0.1 * np.sin(2 * np.pi * 0.7 * t))) / rate
    x = sum(np.sin(k * ph + rng.uniform(0, 2 * np.pi)) / k for k in range(1, 25))
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 3.1 * t + rng.uniform(0, 6))
    return amp * env * x / np.max(np.abs(x))


def q16(x):
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def make_pairs():
    rng = np.random.default_rng(20261016)
    pairs = []   # (name, clean, processed)
    for snr in (-5.0, 5.0, 20.0):
        c = voiced(48000, rng)
        noise = rng.standard_normal(c.size)
        noise *= np.sqrt(np.mean(c ** 2) / np.mean(noise ** 2) / 10 ** (snr / 10))
        pairs.append((f"voiced_snr{int(snr)}", q16(c), q16(c + noise)))
    c = q16(voiced(16000, rng, f0=210.0))
    pairs.append(("identical", c, c.copy()))
    c = voiced(16000, rng)
    c[4000:7000] = 0                                          # digital silence in the clean signal
    p = c + 300 * rng.standard_normal(c.size)
    p[9000:11000] = 0                                         # ... and in the processed one
    pairs.append(("silences", q16(c), q16(p)))
    c = voiced(16000, rng, amp=30000.0)
    c[2000:5000] = np.where(c[2000:5000] >= 0, 32767, -32767)   # full-scale stretches
    p = 1.4 * c + 500 * rng.standard_normal(c.size)
    pairs.append(("full_scale", q16(c), q16(p)))
    c = voiced(4099, rng, f0=95.0)
    pairs.append(("len4099", q16(c), q16(0.7 * c + 800 * rng.standard_normal(c.size))))
    c = voiced(599, rng)
    pairs.append(("len599", q16(c), q16(c + 200 * rng.standard_normal(c.size))))
    c = voiced(480, rng)
    pairs.append(("len480", q16(c), q16(c + 200 * rng.standard_normal(c.size))))
    return pairs


def main():
    sys.path.insert(0, ROOT)
    from oracle.reference_shim import REFERENCE_ROOT
    ref_root = sys.argv[1] if len(sys.argv) > 1 else REFERENCE_ROOT
    pe = load_python_eval(ref_root)
    out = {}
    names = []
    for i, (name, c, p) in enumerate(make_pairs()):
        names.append(name)
        w = pe.wss(c, p, 16000)
        l = pe.llr(c, p, 16000)
        _, s = pe.snr(c, p, 16000)
        ws = np.sort(w)
        wss_dist = np.mean(ws[0:round(np.size(ws) * 0.95)])
        ls = np.sort(l)[0:round(np.size(l) * 0.95)]
        llr_mean = np.mean(ls[~np.isnan(ls)])
        seg = np.mean(s)
        out[f"clean_{i}"], out[f"processed_{i}"] = c, p
        out[f"wss_{i}"], out[f"llr_{i}"], out[f"snr_{i}"] = w, l, s
        out[f"clip_{i}"] = np.array([wss_dist, llr_mean, seg])
        print(f"{name:16s} n={c.size:6d} frames={w.size:4d} wss_dist={wss_dist:.6f} llr_mean={llr_mean:.6f} "
              f"segSNR={seg:.6f} nan_llr={int(np.isnan(l).sum())}")
    out["__names__"] = np.frombuffer(json.dumps(names).encode(), np.uint8)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        main()
