"""bench_mix.py -- what does mixing speech and noise on the device (training/mix.py, csrc/mix.hip) cost?

  python tools/bench_mix.py [--steps 30] [--warmup 8] [--rounds 2] [--skip-fed] [--out FILE]

Two measurements, the E8 batch of bench.py throughout (B = 16, 10 s crops = 160 000 samples):

  alone   on an idle device between two events, 200 launches each, in alternating windows A B A B (``--rounds`` of each):
            A  cum_pcm_batch_f32, the assembling kernel the stage takes the place of (one launch);
            B  cum_mix_pairs on the same int16 block (three launches), with a level drawn and the stats written.
          Bytes: A reads 2 B L int16 and writes 2 B L floats (12 B L); B reads the int16 rows three times and writes the
          same floats (20 B L); against the time, the fraction of the HBM rate (8 TB/s peak).
  fed     tools/bench_feeder.py's method: ONE captured train step, timed in one process in alternating windows of
          ``--steps`` steps between two device synchronisations:
            P  ``step(batch)`` on a feeder over a pair dataset -- the code path without this feature, the yardstick;
            X  ``step(batch)`` on a feeder over the same files taken as separate speech and noise, with ``mix=Mix()``.

The last line is the result as JSON.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--crop-seconds", type=float, default=10.0)
    ap.add_argument("--clip-seconds", type=float, default=12.0)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--dtype", default="f16", choices=["f16", "bf16", "f32"])
    ap.add_argument("--skip-fed", action="store_true", help="only the launches alone")
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args()

    assert torch.cuda.is_available(), "bench_mix.py needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    import bench_feeder as bf
    from cleanumamba_amd import hip
    from cleanumamba_amd.training import mix as M
    lib = hip.lib()
    B, L = args.batch, int(args.crop_seconds * bf.RATE)

    # ---- the launches alone
    def timed(fn, n=200):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n
    rng = np.random.default_rng(0)
    pitch = (L + 7) // 8 * 8
    rows = np.clip(np.round(0.05 * 32768.0 * rng.standard_normal((2 * B, pitch))), -32768, 32767).astype(np.int16)
    pcm = torch.from_numpy(rows).to(dev)
    src_len = torch.full((B,), L, dtype=torch.int32, device=dev)
    draws = M.Mix().draw(np.random.default_rng(1), B)
    recs = torch.from_numpy(draws.pack([L] * B)).to(dev)
    work, stats = M.workspace_for(B, L, dev), torch.empty(B, M.STATS, device=dev)
    clean, noisy = torch.empty(B, 1, L, device=dev), torch.empty(B, 1, L, device=dev)
    calls = {
        "A": lambda: hip.check(lib.cum_pcm_batch_f32(hip.ptr(pcm), pitch, hip.ptr(src_len), B, L, hip.ptr(clean), L,
                                                     hip.ptr(noisy), L, hip.stream_ptr())),
        "B": lambda: M.launch(pcm, pitch, recs, B, L, work, clean, L, noisy, L, stats),
    }
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    alone_windows = [{"mode": tag, "ms": round(timed(calls[tag]), 4)} for _ in range(args.rounds) for tag in ("A", "B")]
    moved = {"A": 12 * B * L, "B": 20 * B * L}
    alone = {}
    for tag, name, launches in (("A", "cum_pcm_batch_f32", 1), ("B", "cum_mix_pairs", 3)):
        ms = [w["ms"] for w in alone_windows if w["mode"] == tag]
        mean = sum(ms) / len(ms)
        alone[tag] = {"kernel": name, "launches": launches, "ms": round(mean, 4), "spread_ms": round(max(ms) - min(ms), 4),
                      "bytes": moved[tag], "TB_per_s": round(moved[tag] / (mean * 1e-3) / 1e12, 3),
                      "frac_of_hbm_peak": round(moved[tag] / (mean * 1e-3) / HBM_PEAK, 3)}
        print(f"alone {tag}: {alone[tag]}", flush=True)
    result = {"tool": "tools/bench_mix.py", "batch": B, "length": L, "alone_windows": alone_windows, "alone": alone,
              "B_over_A": round(alone["B"]["ms"] / alone["A"]["ms"], 3),
              "guard_rows": int(stats[:, 7].sum().item()), "workspace_KB": round(8 * work.numel() / 1e3, 1)}

    # ---- the fed step
    if not args.skip_fed:
        from cleanumamba_amd.network import Net
        from cleanumamba_amd.training.feeder import BatchFeeder
        from cleanumamba_amd.training.train_step import TrainStep
        from cleanumamba_amd.util.dataset import CleanNoisyPairDataset, SpeechNoiseDataset
        tmp = tempfile.TemporaryDirectory(prefix="mix_bench_")
        t0 = time.perf_counter()
        bf.write_tree(tmp.name, args.pairs, int(args.clip_seconds * bf.RATE))
        print(f"tree: {args.pairs} pairs x {args.clip_seconds:g} s written in {time.perf_counter() - t0:.1f} s", flush=True)
        ac = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": None}[args.dtype]
        torch.manual_seed(0)
        step = TrainStep(Net("CleanUMamba", bf.E8).to(dev).train(), autocast_dtype=ac)
        pairs = CleanNoisyPairDataset(root=tmp.name, subset="training", crop_length_sec=args.crop_seconds)
        sets = os.path.join(tmp.name, "training_set")          # the same files, as two unpaired corpora
        unpaired = SpeechNoiseDataset(os.path.join(sets, "clean"), os.path.join(sets, "noisy"), args.crop_seconds)
        feeders = {"P": BatchFeeder(pairs, B, dev, crop_length=L, seed=0),
                   "X": BatchFeeder(unpaired, B, dev, crop_length=L, seed=0, mix=M.Mix())}

        def batches(feeder):
            while True:
                for batch in feeder:
                    yield batch
        streams = {tag: batches(f) for tag, f in feeders.items()}

        def run(tag, n):
            for _ in range(n):
                step(next(streams[tag]))
        settle = 0
        if ac == torch.float16:          # let the dynamic loss scale back off before anything is timed (as bench.py does)
            clean_run, skipped = 0, 0.0
            while clean_run < 2 and settle < 24:
                run("P", 1)
                settle += 1
                now = float(step.optimizer.state_vec[9])
                clean_run = clean_run + 1 if now == skipped else 0
                skipped = now
        for tag in feeders:
            run(tag, args.warmup)
        torch.cuda.synchronize()
        assert step.graph_status == "captured", step.graph_status
        windows = []
        for _ in range(args.rounds):
            for tag in feeders:
                torch.cuda.synchronize()
                t = time.perf_counter()
                run(tag, args.steps)
                torch.cuda.synchronize()
                ms = 1e3 * (time.perf_counter() - t) / args.steps
                windows.append({"mode": tag, "ms_per_step": round(ms, 4)})
                print(f"{tag}: {ms:.3f} ms/step", flush=True)
        idle = {tag: round(f.idle_seconds, 4) for tag, f in feeders.items()}
        for f in feeders.values():
            f.close()
        tmp.cleanup()
        mean = {tag: sum(w["ms_per_step"] for w in windows if w["mode"] == tag) / args.rounds for tag in feeders}
        p = [w["ms_per_step"] for w in windows if w["mode"] == "P"]
        result.update(workload=f"CleanUMamba-E8 train step, B={B}, {args.crop_seconds:g} s crops, {args.dtype}, one hipGraph",
                      steps_per_window=args.steps, warmup=args.warmup, settle_steps=settle, windows=windows,
                      P_to_P_spread_ms=round(max(p) - min(p), 4), mean_ms={k: round(v, 4) for k, v in mean.items()},
                      X_minus_P_ms=round(mean["X"] - mean["P"], 4), X_minus_P_frac=round(mean["X"] / mean["P"] - 1, 5),
                      feeder_idle_s=idle)
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
