"""Stream pool (network/streampool.py) throughput on the pruned E8 model, beside tools/bench_streaming.py (lock-step
feed_batch).  GPU box only.  One JSON line per mode:
  lockstep  256 slots open together and fed 16-hop calls of 30 s of audio each, then closed: ms per hop, RTF;
  churn     seeded join / leave: streams of 2 - 20 s join at random calls into a 256-slot pool, each call brings every
            live slot 12 - 20 hops' worth of samples (ragged, off the hop grid), streams close when their audio ends;
  sparse    256 live slots; calls that name 8 of them (one hop each) against calls that name all 256.
Usage: python tools/bench_stream_pool.py [lockstep|churn|sparse|all] [checkpoint]"""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from cleanumamba_amd.network import CleanUMamba

MODE = sys.argv[1] if len(sys.argv) > 1 else "all"
CKPT = sys.argv[2] if len(sys.argv) > 2 else "pruned500k"
dev = torch.device("cuda")
with np.load(f"tests/golden/ckpt_{CKPT}.npz") as f:
    cfg = json.loads(bytes(f["__network_config__"]).decode())
    sd = {k: torch.from_numpy(f[k].astype(np.float32)) for k in f.files if k != "__network_config__"}
net = CleanUMamba(**cfg)
net.load_state_dict(sd) if CKPT == "442k" else net.load_pruned_state_dict(sd)
net = net.to(dev).eval()
hop, F, SR = net.total_stride, net.frame_length, 16000


def lockstep(S=256, seconds=30.0):
    n = int(seconds * SR)
    x = 0.05 * torch.randn(S, n, device=dev)
    pool = net.stream_pool(S)
    slots = pool.open(S)
    pool.feed(slots, x[:, :4 * hop + F])                     # warm-up (first frames, a close: its drain)
    pool.close(slots)
    torch.cuda.synchronize()
    slots = pool.open(S)
    t0 = time.time()
    for i in range(0, n, 16 * hop):
        pool.feed(slots, x[:, i:i + 16 * hop])
    pool.close(slots)
    torch.cuda.synchronize()
    dt = time.time() - t0
    return {"mode": "lockstep", "checkpoint": CKPT, "slots": S, "seconds_per_stream": seconds, "wall_s": round(dt, 3),
            "ms_per_hop": round(1e3 * dt / (n // hop), 3), "rtf_aggregate": round(S * seconds / dt, 1)}


def churn(capacity=256, calls=200, seed=0):
    rng = np.random.default_rng(seed)
    pool = net.stream_pool(capacity)
    left, audio, joins, closes = {}, 0, 0, 0
    src = 0.05 * torch.randn(capacity, 40 * hop, device=dev)
    torch.cuda.synchronize()
    t0 = time.time()
    for c in range(calls):
        free = capacity - len(pool.live)
        n_join = min(free, int(rng.integers(0, 12)) if c else capacity - 16)
        for s in pool.open(n_join):
            left[s] = int(rng.uniform(2.0, 20.0) * SR)
            joins += 1
        done = [s for s in pool.live if left[s] <= 0]
        if done:
            pool.close(done)
            closes += len(done)
        live = pool.live
        if live:
            lens = [min(left[s], int(rng.integers(12 * hop, 20 * hop))) for s in live]
            chunks = [src[s, :n] for s, n in zip(live, lens)]
            pool.feed(live, chunks)
            for s, n in zip(live, lens):
                left[s] -= n
            audio += sum(lens)
    torch.cuda.synchronize()
    dt = time.time() - t0
    return {"mode": "churn", "checkpoint": CKPT, "capacity": capacity, "calls": calls, "seed": seed, "joins": joins,
            "closes": closes, "wall_s": round(dt, 3), "audio_s": round(audio / SR, 1),
            "rtf_aggregate": round(audio / SR / dt, 1), "mean_live": round(audio / (calls * 16 * hop), 1),
            "ms_per_call": round(1e3 * dt / calls, 3), "ms_per_hop": round(1e3 * dt / calls / 16, 3)}


def sparse(S=256, reps=200):
    pool = net.stream_pool(S)
    slots = pool.open(S)
    x = 0.05 * torch.randn(S, 8 * hop + F, device=dev)
    pool.feed(slots, x[:, :4 * hop + F])
    out = {"mode": "sparse", "checkpoint": CKPT, "slots": S}
    for k in (8, S):
        named = slots[:k]
        chunk = x[:k, :hop]
        for _ in range(5):
            pool.feed(named, chunk)
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(reps):
            pool.feed(named, chunk)
        torch.cuda.synchronize()
        out[f"ms_per_call_{k}_slots_1_hop"] = round(1e3 * (time.time() - t0) / reps, 4)
    return out


with torch.no_grad():
    for mode, fn in (("lockstep", lockstep), ("churn", churn), ("sparse", sparse)):
        if MODE in (mode, "all"):
            print(json.dumps(fn()), flush=True)
