"""bench_feeder.py -- does the E8 train step keep its benched time when its batches come from files?

  python tools/bench_feeder.py [--steps 40] [--warmup 10] [--rounds 2] [--out FILE]

Writes a synthetic dataset tree (``--pairs`` pairs of 16-bit mono wav files of ``--clip-seconds`` s, seeded noise) into
a temporary directory, builds ONE CleanUMamba-E8 train step (B = 16, 10 s crops, the bench.py configuration) and times
it in one process, alternating, ``--rounds`` times  A B A B ...:

  A  step(clean, noisy) on two fixed device tensors -- what bench.py measures;
  B  ``for batch in BatchFeeder(...): step(batch)`` -- int16 crops read from the page cache by the feeder's threads,
     uploaded on its stream, assembled by cum_pcm_batch_f32 into the captured graph's inputs;

then once each, to say where a difference between A and B comes from:

  C  step(clean, noisy) on two float tensors in pageable HOST memory: the reference loop's route
     (src/training/train.py:259-260), two synchronous 10 MB copies in front of the graph;
  D  step(batch) on ONE batch kept alive, no next(): the assembling launch and its events, no reading, no upload;
  E  next() every step, its batch dropped, then step(clean, noisy): reading, uploads and next()'s waits, no assembling;
  G  step(clean_i, noisy_i) over eight different batches held on the device: A with inputs that change from step to
     step as B's do, and nothing of the feeder;
  A  again, against drift.

Every window is ``--steps`` steps between two device synchronisations on the host clock.  Two things are reported about
the feeder's waits, and they are different things: ``starved`` is the host time next() waited for the READERS (a batch
was not staged when asked for: the feeder is too slow); ``held`` is the time it waited for the device -- for the kernel
that last read a device block before the next upload into it is issued, and for an upload to leave its staging slot --
which in a loop that never synchronises is back-pressure: it is where such a loop is kept from running more than
depth + 1 steps ahead of the device.
The timeline places every upload on the device's clock: its end relative to the end of the step before the one that
consumes it (negative: it ran beside earlier steps, nothing of it is exposed).  The last line is the result as JSON.
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
RATE = 16000


def write_tree(root, pairs, samples, seed=0):
    """training_set/{clean,noisy}/fileid_{i}.wav: speech-level noise, the noisy file = clean + more noise."""
    from scipy.io import wavfile
    rng = np.random.default_rng(seed)
    for sub in ("clean", "noisy"):
        os.makedirs(os.path.join(root, "training_set", sub), exist_ok=True)
    for i in range(pairs):
        clean = 0.05 * rng.standard_normal(samples)
        noisy = clean + 0.05 * rng.standard_normal(samples)
        for sub, x in (("clean", clean), ("noisy", noisy)):
            pcm = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
            wavfile.write(os.path.join(root, "training_set", sub, f"fileid_{i}.wav"), RATE, pcm)


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
    ap.add_argument("--root", default=None, help="where to write the tree (default: a temporary directory)")
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args()

    tmp = None
    root = args.root
    if root is None:
        tmp = tempfile.TemporaryDirectory(prefix="feeder_bench_")
        root = tmp.name
    t0 = time.perf_counter()
    write_tree(root, args.pairs, int(args.clip_seconds * RATE))
    print(f"tree: {args.pairs} pairs x {args.clip_seconds:g} s written in {time.perf_counter() - t0:.1f} s", flush=True)

    assert torch.cuda.is_available(), "bench_feeder.py needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from cleanumamba_amd import hip
    from cleanumamba_amd.network import Net
    from cleanumamba_amd.training.feeder import BatchFeeder
    from cleanumamba_amd.training.train_step import TrainStep
    from cleanumamba_amd.util.dataset import CleanNoisyPairDataset
    hip.lib()

    ac = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": None}[args.dtype]
    B, L = args.batch, int(args.crop_seconds * RATE)
    torch.manual_seed(0)
    net = Net("CleanUMamba", E8).to(dev).train()
    step = TrainStep(net, autocast_dtype=ac)
    dataset = CleanNoisyPairDataset(root=root, subset="training", crop_length_sec=args.crop_seconds)
    feeder = BatchFeeder(dataset, B, dev, crop_length=L, seed=0, depth=args.depth, workers=args.workers)

    def batches():
        while True:
            for batch in feeder:
                yield batch
    stream_of_batches = batches()
    clean, noisy = next(stream_of_batches).tensors()            # A's fixed inputs: a real batch, on the device
    clean_host, noisy_host = clean.cpu(), noisy.cpu()           # C's: the same, pageable
    kept = []                                                   # D's batch

    def run_a(n):
        for _ in range(n):
            step(clean, noisy)

    def run_b(n):
        for _ in range(n):
            step(next(stream_of_batches))

    def run_c(n):
        for _ in range(n):
            step(clean_host, noisy_host)

    def run_d(n):
        for _ in range(n):
            step(kept[0])

    def run_e(n):
        for _ in range(n):
            next(stream_of_batches)
            step(clean, noisy)

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
    run_b(args.warmup)
    torch.cuda.synchronize()
    assert step.graph_status == "captured", step.graph_status

    def window(tag, run):
        torch.cuda.synchronize()
        read0, up0, late0, host0 = feeder.wait_read_s, feeder.wait_upload_s, feeder.uploads_late, step.host_seconds
        t = time.perf_counter()
        run(args.steps)
        torch.cuda.synchronize()
        el = time.perf_counter() - t
        w = {"mode": tag, "ms_per_step": round(1e3 * el / args.steps, 4),
             "step_host_ms": round(1e3 * (step.host_seconds - host0) / args.steps, 4),
             "starved_frac": round((feeder.wait_read_s - read0) / el, 6),
             "held_frac": round((feeder.wait_upload_s - up0) / el, 6),
             "uploads_issued_late": feeder.uploads_late - late0}
        print(f"{tag}: {w['ms_per_step']:.3f} ms/step   step() host {w['step_host_ms']:.3f} ms;  next() starved "
              f"{100 * w['starved_frac']:.3f} %, held {100 * w['held_frac']:.2f} % of the window; "
              f"{w['uploads_issued_late']} uploads issued late", flush=True)
        return w

    windows = []
    for _ in range(args.rounds):
        windows += [window("A", run_a), window("B", run_b)]
    run_c(3)
    extra = [window("C", run_c)]
    kept.append(next(stream_of_batches))
    run_d(3)
    extra.append(window("D", run_d))
    run_e(3)
    extra.append(window("E", run_e))
    pool = [next(stream_of_batches).tensors() for _ in range(8)]       # G's inputs: eight different batches, on the device
    turn = [0]

    def run_g(n):
        for _ in range(n):
            turn[0] += 1
            step(*pool[turn[0] % len(pool)])
    run_g(3)
    extra += [window("G", run_g), window("A", run_a)]

    # where each upload lands on the device's clock: 12 B steps with an event before and after each
    late0 = feeder.uploads_late
    marks = []
    torch.cuda.synchronize()
    for _ in range(12):
        batch = next(stream_of_batches)
        before, after = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        before.record()
        step(batch)
        after.record()
        marks.append((batch.uploaded, before, after))
    torch.cuda.synchronize()
    timeline = [{"upload_end_minus_previous_step_end_ms": round(marks[k - 1][2].elapsed_time(marks[k][0]), 3),
                 "step_first_launch_to_end_ms": round(marks[k][1].elapsed_time(marks[k][2]), 3)}
                for k in range(2, len(marks))]
    late = feeder.uploads_late - late0
    print("upload end - previous step's end (ms):", [t["upload_end_minus_previous_step_end_ms"] for t in timeline])
    print("step, first launch to end (ms):       ", [t["step_first_launch_to_end_ms"] for t in timeline],
          f"  uploads issued late: {late} of 12", flush=True)

    # the pieces alone on an idle device (events, 20 each): one upload of a staging slot, one assembling launch, the two
    # device-to-device copies A makes, the two pageable copies C makes
    slot_elems = 2 * B * feeder.pitch + 2 * B
    pinned = torch.zeros(slot_elems, dtype=torch.int16, pin_memory=True)
    on_dev = torch.zeros(slot_elems, dtype=torch.int16, device=dev)

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
    batch = next(stream_of_batches)
    alone = {"upload_one_slot_pinned_int16": timed(lambda: on_dev.copy_(pinned, non_blocking=True)),
             "assemble_launch_cum_pcm_batch_f32": timed(lambda: batch.into(c2, n2)),
             "two_device_float_copies": timed(lambda: (c2.copy_(clean), n2.copy_(noisy))),
             "two_pageable_float_copies": timed(lambda: (c2.copy_(clean_host), n2.copy_(noisy_host)), n=5)}
    feeder.close()

    a = [w["ms_per_step"] for w in windows if w["mode"] == "A"]
    b = [w["ms_per_step"] for w in windows if w["mode"] == "B"]
    spread, mean_a, mean_b = max(a) - min(a), sum(a) / len(a), sum(b) / len(b)
    result = {"tool": "tools/bench_feeder.py", "workload": f"CleanUMamba-E8 train step, B={B}, {args.crop_seconds:g} s crops, "
              f"{args.dtype}, one hipGraph; {args.pairs} pairs of {args.clip_seconds:g} s in the page cache",
              "steps_per_window": args.steps, "warmup": args.warmup, "settle_steps": settle, "workers": args.workers,
              "depth": args.depth, "order": [w["mode"] for w in windows + extra], "windows": windows + extra,
              "A_ms": a, "B_ms": b, "A_to_A_spread_ms": round(spread, 4), "B_minus_A_ms": round(mean_b - mean_a, 4),
              "B_within_A_spread": bool(abs(mean_b - mean_a) <= spread),
              "feeder_idle_frac_B": round(sum(w["starved_frac"] for w in windows if w["mode"] == "B") / len(b), 6),
              "held_frac_B": round(sum(w["held_frac"] for w in windows if w["mode"] == "B") / len(b), 6),
              "alone_on_idle_device_ms": alone, "timeline_B": timeline, "uploads_issued_late_in_timeline": late,
              "slot_bytes": 2 * slot_elems, "float_batch_bytes": 2 * 4 * B * L}
    print(f"A {a} ms  B {b} ms;  A-to-A spread {spread:.3f} ms, B - A {mean_b - mean_a:+.3f} ms "
          f"({100 * (mean_b - mean_a) / mean_a:+.2f} %), feeder idle (starved) {100 * result['feeder_idle_frac_B']:.3f} % of B's time")
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
