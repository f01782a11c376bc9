"""bench_denoise_folder.py -- is a folder of mixed-length files denoised faster in ragged batches than one file per forward?

  python tools/bench_denoise_folder.py [--files 64] [--rounds 2] [--out FILE]

Writes ``--files`` seeded 16-bit mono wav files of 2 - 12 s (16 kHz) into a temporary directory and denoises the folder
with two models -- the shipped 442k checkpoint in f32 and a full-width E8 model with synthetic weights under f16
autocast -- by two routes, alternating A B A B ... ``--rounds`` times in one process:

  A  one file per ``forward``: read the file, upload it, ``model(x)``, bring the result back -- the reference's route
     (src/examples/denoise.py:42-68, ``batch_size=1``) and the best the package offered before ``denoise_batch``;
  B  ``model.denoise_batch``: the files read as int16, grouped by ``plan_batches`` (its defaults), each batch uploaded
     once and run by ``forward_ragged``; the results brought back once per pass.

Every window is one pass over the folder between two device synchronisations on the host clock, reading included on both
routes (the files are in the page cache after the warm-up pass).  Reported: audio-seconds per second per route and
window, and for B the share of a pass spent in the launches the ragged route adds -- per-clip std, framing, un-framing
and the row masks (cum_rows_zero_tail) -- from device events around those launches in one extra, instrumented pass (the
masks inside cum_dech_fwd_ragged / cum_dec7_fwd_ragged are part of those kernels and cannot be told apart).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

E8 = dict(channels_input=1, channels_output=1, channels_H=64, max_H=768, encoder_n_layers=8, kernel_size=4,
          stride=2, tsfm_n_layers=3, tsfm_n_head=8, tsfm_d_model=512, tsfm_d_inner=2048)
RATE = 16000


def write_folder(root, files, seed=0):
    from scipy.io import wavfile
    rng = np.random.default_rng(seed)
    lengths = []
    for i in range(files):
        n = int(rng.integers(2 * RATE, 12 * RATE + 1))
        x = 0.05 * rng.standard_normal(n) + 0.05 * rng.standard_normal(n)
        wavfile.write(os.path.join(root, f"noisy_{i:03d}.wav"), RATE, np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16))
        lengths.append(n)
    return lengths


def models(dev):
    from conftest import load_ckpt
    from oracle import synth
    from cleanumamba_amd.network import CleanUMamba
    sd, cfg = load_ckpt("442k")
    small = CleanUMamba(**cfg)
    small.load_state_dict(sd, strict=True)
    big = CleanUMamba(**E8)
    big.load_state_dict(synth.fill_state_dict({k: tuple(v.shape) for k, v in big.state_dict().items()}, seed=0), strict=True)
    return [("442k_f32", small.to(dev).float().eval(), None), ("e8_synth_f16", big.to(dev).float().eval(), torch.float16)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_denoise_folder.py needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from cleanumamba_amd import hip
    from cleanumamba_amd.network import convstack as cs
    from cleanumamba_amd.network import ragged as rg
    from cleanumamba_amd.util.dataset import NosyOnlyDataset
    hip.lib()

    tmp = tempfile.TemporaryDirectory(prefix="denoise_folder_bench_")
    lengths = write_folder(tmp.name, args.files)
    audio_s = sum(lengths) / RATE
    ds = NosyOnlyDataset(folder=tmp.name)
    print(f"folder: {args.files} files, {audio_s:.1f} s of audio, {min(lengths) / RATE:.2f} - {max(lengths) / RATE:.2f} s", flush=True)

    results = []
    for name, model, ac in models(dev):
        amp = (lambda: torch.autocast("cuda", dtype=ac)) if ac is not None else (lambda: torch.autocast("cuda", enabled=False))
        plan = rg.plan_batches(lengths, model.valid_length)
        waste = [round(1 - sum(model.valid_length(lengths[i]) for i in b.indices)
                       / (len(b.indices) * model.valid_length(lengths[b.indices[0]])), 4) for b in plan]

        def run_a():
            outs = []
            for n in range(len(ds)):
                x = ds[n][1].to(dev, non_blocking=True)
                outs.append(model(x.view(1, 1, -1))[0, 0].cpu())
            return outs

        def run_b():
            clips = [torch.from_numpy(ds.read_pcm(n)) for n in range(len(ds))]
            outs = model.denoise_batch(clips)
            flat = torch.cat(outs).cpu()
            return list(flat.split([o.shape[0] for o in outs]))

        def window(tag, run):
            torch.cuda.synchronize()
            t = time.perf_counter()
            outs = run()
            torch.cuda.synchronize()
            el = time.perf_counter() - t
            w = {"mode": tag, "seconds": round(el, 4), "audio_s_per_s": round(audio_s / el, 1)}
            print(f"{name} {tag}: {el * 1e3:9.1f} ms per pass   {w['audio_s_per_s']:10.1f} audio-s / s", flush=True)
            return w, outs

        with torch.no_grad(), amp():
            (_, ya), (_, yb) = window("warm A", run_a), window("warm B", run_b)
            dev_ab = max(float((a.double() - b.double()).norm() / a.double().norm().clamp_min(1e-30)) for a, b in zip(ya, yb))
            windows = []
            for _ in range(args.rounds):
                windows += [window("A", run_a)[0], window("B", run_b)[0]]
            # one instrumented pass of B: events around the launches the ragged route adds
            spans = {"std": [], "frame": [], "unframe": [], "zero_tail": []}
            real = {"std": rg.clip_std_ragged, "frame": rg.frame_input_ragged, "unframe": rg.unframe_ragged,
                    "zero_tail": cs.rows_zero_tail}

            def timed(kind):
                def call(*a, **k):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out = real[kind](*a, **k)
                    e1.record()
                    spans[kind].append((e0, e1))
                    return out
                return call
            rg.clip_std_ragged, rg.frame_input_ragged, rg.unframe_ragged = timed("std"), timed("frame"), timed("unframe")
            cs.rows_zero_tail = timed("zero_tail")
            try:
                wi, _ = window("B instrumented", run_b)
            finally:
                rg.clip_std_ragged, rg.frame_input_ragged, rg.unframe_ragged = real["std"], real["frame"], real["unframe"]
                cs.rows_zero_tail = real["zero_tail"]
            routes = model.ragged_dispatch
        added_ms = {k: round(sum(a.elapsed_time(b) for a, b in v), 4) for k, v in spans.items()}
        a = [w["audio_s_per_s"] for w in windows if w["mode"] == "A"]
        b = [w["audio_s_per_s"] for w in windows if w["mode"] == "B"]
        res = {"model": name, "windows": windows, "A_audio_s_per_s": a, "B_audio_s_per_s": b,
               "B_over_A": round((sum(b) / len(b)) / (sum(a) / len(a)), 3), "B_at_least_A": bool(min(b) >= max(a)),
               "batches": [len(p.indices) for p in plan], "batch_waste": waste,
               "B_vs_A_rel_l2_worst_file": dev_ab, "decoder_routes_last_batch": routes,
               "instrumented_pass_seconds": wi["seconds"], "added_launch_ms": added_ms,
               "added_launch_counts": {k: len(v) for k, v in spans.items()},
               "added_launch_share_of_pass": round(sum(added_ms.values()) * 1e-3 / wi["seconds"], 5)}
        print(f"{name}: A {a}  B {b} audio-s / s;  B / A = {res['B_over_A']};  added launches {added_ms} ms = "
              f"{100 * res['added_launch_share_of_pass']:.2f} % of a pass;  worst file B vs A rel-L2 {dev_ab:.2e}", flush=True)
        results.append(res)
        del model
        torch.cuda.empty_cache()

    result = {"tool": "tools/bench_denoise_folder.py", "files": args.files, "audio_seconds": round(audio_s, 2),
              "clip_seconds": [round(min(lengths) / RATE, 2), round(max(lengths) / RATE, 2)], "rounds": args.rounds,
              "order": "warm A, warm B, then A B per round, then one instrumented B", "models": results}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
    tmp.cleanup()


if __name__ == "__main__":
    main()
