"""Speech metrics (util/metrics.py) on the DNS validation shape: 150 clips x 10 s at 16 kHz, all four metrics (wss_dist,
llr_mean, segSNR, STOI) in one speech_metrics call, and the same batch with the five extended metrics added (estoi,
si_sdr, snr, cep_dist, fwsegSNR: nine in all), the two timed alternately in one run.  GPU box only.  Prints one JSON
line: each batch's wall time after a warm-up (device synchronised), per-clip times and the ratio nine / four.  Kernel
times come from a separate run of this script under ``rocprofv3 --kernel-trace --stats``.
Usage: python tools/bench_metrics.py [clips] [seconds] [repeats] [out.json]"""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from cleanumamba_amd.util import metrics as M

CLIPS = int(sys.argv[1]) if len(sys.argv) > 1 else 150
SECONDS = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
REPEATS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
OUT = sys.argv[4] if len(sys.argv) > 4 else None

rng = np.random.default_rng(0)
n = int(SECONDS * 16000)
t = np.arange(n) / 16000
clean, proc = [], []
for i in range(CLIPS):
    f0 = rng.uniform(90, 250)
    x = sum(np.sin(2 * np.pi * k * f0 * t + rng.uniform(0, 6)) / k for k in range(1, 20))
    x *= (0.55 + 0.45 * np.sin(2 * np.pi * 3.0 * t)) * 6000 / np.max(np.abs(x))
    y = x + rng.uniform(100, 3000) * rng.standard_normal(n)
    clean.append(np.clip(np.round(x), -32768, 32767).astype(np.int16))
    proc.append(np.clip(np.round(y), -32768, 32767).astype(np.int16))
dev = torch.device("cuda")
clean_d = [torch.from_numpy(c).to(dev) for c in clean]
proc_d = [torch.from_numpy(p).to(dev) for p in proc]

NINE = M.METRICS + M.EXT_METRICS


def timed(names):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = M.speech_metrics(clean_d, proc_d, metrics=names)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


timed(M.METRICS)                                              # warm-up (tables, library, allocator)
timed(NINE)
times, times9 = [], []
for _ in range(REPEATS):                                      # alternating: both see the same clocks and allocator state
    dt, r = timed(M.METRICS)
    times.append(dt)
    dt, r9 = timed(NINE)
    times9.append(dt)
res = {"clips": CLIPS, "seconds_per_clip": SECONDS, "frames": int(M.frame_counts([n] * CLIPS).sum()),
       "batch_ms_median": round(1e3 * float(np.median(times)), 2), "batch_ms_min": round(1e3 * min(times), 2),
       "per_clip_ms": round(1e3 * float(np.median(times)) / CLIPS, 3),
       "means": {k: round(float(v.mean()), 5) for k, v in r.items()},
       "nine": {"batch_ms_median": round(1e3 * float(np.median(times9)), 2), "batch_ms_min": round(1e3 * min(times9), 2),
                "per_clip_ms": round(1e3 * float(np.median(times9)) / CLIPS, 3),
                "ratio_to_four": round(float(np.median(times9) / np.median(times)), 3),
                "means": {k: round(float(v.mean()), 5) for k, v in r9.items()}}}
print(json.dumps(res))
if OUT:
    with open(OUT, "w") as f:
        json.dump(res, f)
