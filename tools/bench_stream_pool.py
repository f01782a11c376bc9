"""Stream pool (network/streampool.py) throughput, beside tools/bench_streaming.py (lock-step feed_batch).  GPU box only.
One JSON line per mode:
  lockstep  the slots open together and are fed 16-hop calls of audio each, then closed: ms per hop, RTF;
  churn     seeded join / leave: streams of 2 - 20 s join at random calls into the pool, each call brings every live slot
            12 - 20 hops' worth of samples (ragged, off the hop grid), streams close when their audio ends;
  sparse    all slots live; calls that name 8 of them (one hop each) against calls that name all.
Usage: python tools/bench_stream_pool.py [lockstep|churn|sparse|all] [checkpoint] [--backend kernel|layers]
           [--synthetic e6|e8] [--slots N] [--seconds S] [--calls N] [--reps N]
--synthetic: instead of a checkpoint, a model of the E6 (27 M) / E8 (41 M) configuration with seeded random weights
(no such checkpoint is shipped): the models only the "layers" backend pools.  On that backend lockstep alternates the
pool with lock-step feed_batch + flush_batch of the same model on the same audio (--reps times, medians reported) and
times the slot-row mover with hipEvents around its launches in one more, instrumented run; churn counts the mover's
launches and bytes."""
import argparse
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from cleanumamba_amd.network import CleanUMamba, layerpool

ap = argparse.ArgumentParser()
ap.add_argument("mode", nargs="?", default="all", choices=["lockstep", "churn", "sparse", "all"])
ap.add_argument("checkpoint", nargs="?", default="pruned500k")
ap.add_argument("--backend", default=None, choices=["kernel", "layers"])
ap.add_argument("--synthetic", default=None, choices=["e6", "e8"])
ap.add_argument("--slots", type=int, default=None)
ap.add_argument("--seconds", type=float, default=None)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
MODE, CKPT, BACKEND = args.mode, args.checkpoint, args.backend
dev = torch.device("cuda")
if args.synthetic:
    CKPT = "synthetic-" + args.synthetic
    torch.manual_seed(0)
    net = CleanUMamba(channels_input=1, channels_output=1, channels_H=64, max_H=768, kernel_size=4, stride=2,
                      encoder_n_layers=8 if args.synthetic == "e8" else 6, tsfm_n_layers=3, tsfm_n_head=8,
                      tsfm_d_model=512, tsfm_d_inner=2048)
else:
    with np.load(f"tests/golden/ckpt_{CKPT}.npz") as f:
        cfg = json.loads(bytes(f["__network_config__"]).decode())
        sd = {k: torch.from_numpy(f[k].astype(np.float32)) for k in f.files if k != "__network_config__"}
    net = CleanUMamba(**cfg)
    net.load_state_dict(sd) if CKPT == "442k" else net.load_pruned_state_dict(sd)
net = net.to(dev).eval()
hop, F, SR = net.total_stride, net.frame_length, 16000
SLOTS = args.slots or (64 if args.synthetic else 256)
SECONDS = args.seconds or (4.0 if args.synthetic else 30.0)


class MoverClock:
    """Counts the launches of cum_stream_slots_move and, when ``timed``, brackets each with hipEvents (the events cost
    host time: a run that reports wall time is not timed this way)."""

    def __init__(self, timed):
        self.timed, self.calls, self.bytes, self.events, self.inner = timed, 0, 0, [], layerpool.move

    def __enter__(self):
        def move(direction, store, slots, table, clears=None):
            self.calls += 1
            self.bytes += 2 * len(slots) * int(table.host[:, 3].sum())        # read + written
            if self.timed:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
            self.inner(direction, store, slots, table, clears)
            if self.timed:
                b.record()
                self.events.append((a, b))
        layerpool.move = move
        return self

    def __exit__(self, *exc):
        layerpool.move = self.inner

    def report(self):
        out = {"mover_calls": self.calls, "mover_bytes": self.bytes}
        if self.timed and self.events:
            torch.cuda.synchronize()
            ms = sum(a.elapsed_time(b) for a, b in self.events)
            out.update(mover_ms=round(ms, 3), mover_GBps=round(self.bytes / ms / 1e6, 1))
        return out


def lockstep(S=SLOTS, seconds=SECONDS):
    n = int(seconds * SR)
    x = 0.05 * torch.randn(S, n, device=dev)
    pool = net.stream_pool(S, backend=BACKEND)

    def run():
        slots = pool.open(S)
        t0 = time.time()
        for i in range(0, n, 16 * hop):
            pool.feed(slots, x[:, i:i + 16 * hop])
        pool.close(slots)
        torch.cuda.synchronize()
        return time.time() - t0

    def run_feed_batch():
        net.reset_stream()
        t0 = time.time()
        for i in range(0, n, 16 * hop):
            net.feed_batch(x[:, i:i + 16 * hop])
        net.flush_batch()
        torch.cuda.synchronize()
        return time.time() - t0

    def warm_up(feed, end):
        feed(x[:, :4 * hop + F])                             # first frames, then a close: its drain
        end()
        torch.cuda.synchronize()

    slots = pool.open(S)
    warm_up(lambda c: pool.feed(slots, c), lambda: pool.close(slots))
    per_hop = lambda dt: round(1e3 * dt / (n // hop), 3)
    if pool.backend != "layers":
        dt = run()
        return {"mode": "lockstep", "checkpoint": CKPT, "backend": pool.backend, "slots": S, "seconds_per_stream": seconds,
                "wall_s": round(dt, 3), "ms_per_hop": per_hop(dt), "rtf_aggregate": round(S * seconds / dt, 1)}
    # beside lock-step feed_batch + flush_batch of the same model on the same audio in the same 16-hop calls: the two
    # alternate, the medians are reported and every run is listed (the hop is host-bound: other work on the host shows)
    net.reset_stream()
    warm_up(net.feed_batch, net.flush_batch)
    runs = [(run(), run_feed_batch()) for _ in range(args.reps)]
    dt, ref = float(np.median([r[0] for r in runs])), float(np.median([r[1] for r in runs]))
    out = {"mode": "lockstep", "checkpoint": CKPT, "backend": pool.backend, "slots": S, "seconds_per_stream": seconds,
           "wall_s": round(dt, 3), "ms_per_hop": per_hop(dt), "rtf_aggregate": round(S * seconds / dt, 1),
           "feed_batch_ms_per_hop": per_hop(ref), "feed_batch_rtf": round(S * seconds / ref, 1),
           "runs_ms_per_hop": [[per_hop(a), per_hop(b)] for a, b in runs]}
    with MoverClock(True) as clock:
        run()
    out.update(clock.report())
    out["mover_ms_per_hop"] = round(out.get("mover_ms", 0.0) / (n // hop), 4)
    return out


def churn(capacity=SLOTS, calls=args.calls, seed=0):
    with MoverClock(False) as clock:
        out = _churn(capacity, calls, seed)
    if out["backend"] == "layers":
        out.update(clock.report())
    return out


def _churn(capacity, calls, seed):
    rng = np.random.default_rng(seed)
    pool = net.stream_pool(capacity, backend=BACKEND)
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
    return {"mode": "churn", "checkpoint": CKPT, "backend": pool.backend, "capacity": capacity, "calls": calls, "seed": seed, "joins": joins,
            "closes": closes, "wall_s": round(dt, 3), "audio_s": round(audio / SR, 1),
            "rtf_aggregate": round(audio / SR / dt, 1), "mean_live": round(audio / (calls * 16 * hop), 1),
            "ms_per_call": round(1e3 * dt / calls, 3), "ms_per_hop": round(1e3 * dt / calls / 16, 3)}


def sparse(S=SLOTS, reps=200):
    pool = net.stream_pool(S, backend=BACKEND)
    slots = pool.open(S)
    x = 0.05 * torch.randn(S, 8 * hop + F, device=dev)
    pool.feed(slots, x[:, :4 * hop + F])
    out = {"mode": "sparse", "checkpoint": CKPT, "backend": pool.backend, "slots": S}
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
