"""bench_feeder_rates.py -- what does the E8 train step pay when its batches come from files that are not at 16 kHz?

  python tools/bench_feeder_rates.py [--steps 40] [--warmup 10] [--rounds 2] [--out FILE] [--unrated-only]

In the manner of tools/bench_feeder.py: synthetic dataset trees (``--pairs`` pairs of 16-bit mono wav files of
``--clip-seconds`` s, seeded noise) in a temporary directory, ONE CleanUMamba-E8 train step (B = 16, 10 s crops, f16, the
bench.py configuration), every window ``--steps`` steps between two device synchronisations on the host clock, the
windows alternating ``--rounds`` times  A B C D A B C D ...:

  A  step(clean, noisy) on two fixed device tensors -- what bench.py measures;
  B  ``BatchFeeder(...)`` on 16 kHz files: the unrated feeder, cum_pcm_batch_f32;
  C  ``BatchFeeder(..., sample_rate=16000)`` on the SAME files: records instead of lengths, cum_pcm_batch_resample_f32's
     copy route;
  D  ``BatchFeeder(..., sample_rate=16000)`` on 48 kHz files: three times the bytes read and uploaded, the 219-tap chains
     of csrc/resample.hip in front of every step;

then E: the assembling launch alone on an idle device, timed with device events (20 launches each) -- unrated and rated
at 16 kHz, rated at 48 kHz and at 44.1 kHz (the per-lane table route).

For every feeder window: ``starved`` -- host time next() waited for the readers -- and ``held`` -- for the device (see
tools/bench_feeder.py); for D also where each upload ended on the device's clock relative to the end of the step before
the one that uses it.  ``--unrated-only`` times A and B alone and passes no ``sample_rate``: the same script on a
commit without rated feeders, for the unchanged path.  The last line is the result as JSON.
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

E8 = dict(channels_input=1, channels_output=1, channels_H=64, max_H=768, encoder_n_layers=8, kernel_size=4,
          stride=2, tsfm_n_layers=3, tsfm_n_head=8, tsfm_d_model=512, tsfm_d_inner=2048)
MODEL_RATE = 16000


def write_tree(root, pairs, seconds, rate, seed=0):
    """training_set/{clean,noisy}/fileid_{i}.wav at ``rate``: speech-level noise, the noisy file = clean + more noise."""
    from scipy.io import wavfile
    rng = np.random.default_rng(seed)
    samples = int(seconds * rate)
    for sub in ("clean", "noisy"):
        os.makedirs(os.path.join(root, "training_set", sub), exist_ok=True)
    for i in range(pairs):
        clean = 0.05 * rng.standard_normal(samples)
        noisy = clean + 0.05 * rng.standard_normal(samples)
        for sub, x in (("clean", clean), ("noisy", noisy)):
            pcm = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
            wavfile.write(os.path.join(root, "training_set", sub, f"fileid_{i}.wav"), rate, pcm)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--crop-seconds", type=float, default=10.0)
    ap.add_argument("--clip-seconds", type=float, default=12.0)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--dtype", default="f16", choices=["f16", "bf16", "f32"])
    ap.add_argument("--unrated-only", action="store_true", help="windows A and B alone; no sample_rate is passed")
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args()

    tmp = tempfile.TemporaryDirectory(prefix="feeder_rates_bench_")
    trees = {16000: os.path.join(tmp.name, "at16k")}
    if not args.unrated_only:
        trees.update({48000: os.path.join(tmp.name, "at48k"), 44100: os.path.join(tmp.name, "at44k")})
    t0 = time.perf_counter()
    for rate, root in trees.items():
        write_tree(root, args.batch if rate == 44100 else args.pairs, args.clip_seconds, rate)
    print(f"trees at {sorted(trees)} Hz written in {time.perf_counter() - t0:.1f} s", flush=True)

    assert torch.cuda.is_available(), "bench_feeder_rates.py needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from cleanumamba_amd import hip
    from cleanumamba_amd.network import Net
    from cleanumamba_amd.training.feeder import BatchFeeder
    from cleanumamba_amd.training.train_step import TrainStep
    from cleanumamba_amd.util.dataset import CleanNoisyPairDataset
    hip.lib()

    ac = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": None}[args.dtype]
    B, L = args.batch, int(args.crop_seconds * MODEL_RATE)
    torch.manual_seed(0)
    net = Net("CleanUMamba", E8).to(dev).train()
    step = TrainStep(net, autocast_dtype=ac)

    def feeder_of(rate, rated):
        ds = CleanNoisyPairDataset(root=trees[rate], subset="training", crop_length_sec=args.crop_seconds)
        kw = {"sample_rate": MODEL_RATE} if rated else {}
        return BatchFeeder(ds, B, dev, crop_length=L, seed=0, depth=args.depth, workers=args.workers, **kw)

    def batches(feeder):
        while True:
            for batch in feeder:
                yield batch

    feeders = {"B": feeder_of(16000, False)}
    if not args.unrated_only:
        feeders.update({"C": feeder_of(16000, True), "D": feeder_of(48000, True)})
    streams = {k: batches(f) for k, f in feeders.items()}
    clean, noisy = next(streams["B"]).tensors()                 # A's fixed inputs: a real batch, on the device

    def run_a(n):
        for _ in range(n):
            step(clean, noisy)

    def run_fed(tag):
        def run(n):
            for _ in range(n):
                step(next(streams[tag]))
        return run

    settle = 0
    if ac == torch.float16:         # let the dynamic loss scale back off before anything is timed (as bench.py does)
        clean_run, skipped = 0, 0.0
        while clean_run < 2 and settle < 24:
            run_a(1)
            settle += 1
            now = float(step.optimizer.state_vec[9])
            clean_run = clean_run + 1 if now == skipped else 0
            skipped = now
    run_a(args.warmup)
    for tag in feeders:
        run_fed(tag)(args.warmup)
    torch.cuda.synchronize()
    assert step.graph_status == "captured", step.graph_status

    def window(tag, run):
        f = feeders.get(tag)
        torch.cuda.synchronize()
        read0, up0, late0 = (f.wait_read_s, f.wait_upload_s, f.uploads_late) if f else (0.0, 0.0, 0)
        host0 = step.host_seconds
        t = time.perf_counter()
        run(args.steps)
        torch.cuda.synchronize()
        el = time.perf_counter() - t
        w = {"mode": tag, "ms_per_step": round(1e3 * el / args.steps, 4),
             "step_host_ms": round(1e3 * (step.host_seconds - host0) / args.steps, 4)}
        if f:
            w.update({"wait_read_s": round(f.wait_read_s - read0, 6), "wait_upload_s": round(f.wait_upload_s - up0, 6),
                      "starved_frac": round((f.wait_read_s - read0) / el, 6),
                      "held_frac": round((f.wait_upload_s - up0) / el, 6), "uploads_issued_late": f.uploads_late - late0})
        print(f"{tag}: {w['ms_per_step']:.3f} ms/step  " + ("" if not f else
              f"next() starved {100 * w['starved_frac']:.3f} %, held {100 * w['held_frac']:.2f} % of the window; "
              f"{w['uploads_issued_late']} uploads issued late"), flush=True)
        return w

    windows = []
    for _ in range(args.rounds):
        windows.append(window("A", run_a))
        for tag in feeders:
            windows.append(window(tag, run_fed(tag)))
    windows.append(window("A", run_a))                          # against drift

    # D's uploads on the device's clock: 12 steps with an event before and after each
    timeline = None
    if "D" in feeders:
        marks = []
        torch.cuda.synchronize()
        for _ in range(12):
            batch = next(streams["D"])
            before, after = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            before.record()
            step(batch)
            after.record()
            marks.append((batch.uploaded, before, after))
        torch.cuda.synchronize()
        timeline = [{"upload_end_minus_previous_step_end_ms": round(marks[k - 1][2].elapsed_time(marks[k][0]), 3),
                     "step_first_launch_to_end_ms": round(marks[k][1].elapsed_time(marks[k][2]), 3)}
                    for k in range(2, len(marks))]
        print("D: upload end - previous step's end (ms):", [t["upload_end_minus_previous_step_end_ms"] for t in timeline])
        print("D: step, first launch to end (ms):       ", [t["step_first_launch_to_end_ms"] for t in timeline], flush=True)

    # E: the assembling launch alone on an idle device
    def timed(fn, n=20):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return round(a.elapsed_time(b) / n, 4)

    c2, n2 = torch.empty_like(clean), torch.empty_like(noisy)
    alone, slot_bytes = {}, {}
    if not args.unrated_only:
        feeders["E44"] = feeder_of(44100, True)
        streams["E44"] = batches(feeders["E44"])
    for tag, name in (("B", "unrated_16k_cum_pcm_batch_f32"), ("C", "rated_16k_copy_route"), ("D", "rated_48k"),
                      ("E44", "rated_44k1")):
        if tag in feeders:
            batch = next(streams[tag])
            alone[name] = timed(lambda: batch.into(c2, n2))
            slot_bytes[name] = 2 * feeders[tag]._stage[0].flat.numel()
            print(f"E: {name}: {alone[name]:.4f} ms per launch; a slot is {slot_bytes[name]} bytes", flush=True)
    for f in feeders.values():
        f.close()

    def mean(tag):
        v = [w["ms_per_step"] for w in windows if w["mode"] == tag]
        return sum(v) / len(v) if v else None
    a = [w["ms_per_step"] for w in windows if w["mode"] == "A"]
    result = {"tool": "tools/bench_feeder_rates.py",
              "workload": f"CleanUMamba-E8 train step, B={B}, {args.crop_seconds:g} s crops, {args.dtype}, one hipGraph; "
                          f"{args.pairs} pairs of {args.clip_seconds:g} s per tree, in the page cache",
              "steps_per_window": args.steps, "warmup": args.warmup, "settle_steps": settle, "workers": args.workers,
              "depth": args.depth, "order": [w["mode"] for w in windows], "windows": windows, "A_ms": a,
              "A_to_A_spread_ms": round(max(a) - min(a), 4), "B_ms": [w["ms_per_step"] for w in windows if w["mode"] == "B"],
              "B_minus_A_ms": round(mean("B") - mean("A"), 4), "assemble_alone_ms": alone, "slot_bytes": slot_bytes,
              "float_batch_bytes": 2 * 4 * B * L}
    if not args.unrated_only:
        result.update({"C_ms": [w["ms_per_step"] for w in windows if w["mode"] == "C"],
                       "D_ms": [w["ms_per_step"] for w in windows if w["mode"] == "D"],
                       "C_minus_B_ms": round(mean("C") - mean("B"), 4), "D_minus_A_ms": round(mean("D") - mean("A"), 4),
                       "timeline_D": timeline})
    print("  ".join(f"{k} {result[k]}" for k in result if k.endswith("_ms") and not isinstance(result[k], dict)))
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
    tmp.cleanup()


if __name__ == "__main__":
    main()
