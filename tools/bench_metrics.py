"""Speech metrics (util/metrics.py) on the DNS validation shape: 150 clips x 10 s at 16 kHz, all four metrics (wss_dist,
llr_mean, segSNR, STOI) in one speech_metrics call.  GPU box only.  Prints one JSON line: the batch's wall time after a
warm-up (device synchronised), and per-clip times.  Kernel times come from a separate run of this script under
``rocprofv3 --kernel-trace --stats``.
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

r = M.speech_metrics(clean_d, proc_d)                         # warm-up (tables, library, allocator)
torch.cuda.synchronize()
times = []
for _ in range(REPEATS):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = M.speech_metrics(clean_d, proc_d)
    torch.cuda.synchronize()
    times.append(time.perf_counter() - t0)
res = {"clips": CLIPS, "seconds_per_clip": SECONDS, "frames": int(M.frame_counts([n] * CLIPS).sum()),
       "batch_ms_median": round(1e3 * float(np.median(times)), 2), "batch_ms_min": round(1e3 * min(times), 2),
       "per_clip_ms": round(1e3 * float(np.median(times)) / CLIPS, 3),
       "means": {k: round(float(v.mean()), 5) for k, v in r.items()}}
print(json.dumps(res))
if OUT:
    with open(OUT, "w") as f:
        json.dump(res, f)
