"""resample_probe.py -- what does sample-rate conversion cost, alone and in front of and behind the model?

  python tools/resample_probe.py [--clips 64] [--seconds 10] [--reps 20] [--out FILE]

1. ``resample_ragged`` (csrc/resample.hip, one launch) on ``--clips`` int16 clips of ``--seconds`` for 48 k -> 16 k,
   16 k -> 48 k (f32 in: the way back from the model) and 44.1 k -> 16 k: after a warm-up, device events around
   ``--reps`` launches.  Printed: the time of one launch, the bytes it has to move (input samples in, f32 samples out)
   per second, and that rate over the HBM peak (8.0 TB/s by specification; a float4 copy reaches 6.29 TB/s).  The fma
   count (K per output) is printed beside it: the kernel's other bound.
2. ``denoise_batch`` on the same clips at 48 kHz with ``rates=48000`` (convert, denoise, convert back, crop) against the
   same clips converted to 16 kHz beforehand and denoised without ``rates`` -- the route that exists without the
   resampler -- alternating A B, device events around every call, with the shipped 442k checkpoint in f32 and a
   full-width E8 model with synthetic weights under f16 autocast.

Every line printed goes to ``--out`` as well.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12          # bytes / s, specification
HBM_COPY = 6.29e12         # bytes / s, a float4 copy
E8 = dict(channels_input=1, channels_output=1, channels_H=64, max_H=768, encoder_n_layers=8, kernel_size=4,
          stride=2, tsfm_n_layers=3, tsfm_n_head=8, tsfm_d_model=512, tsfm_d_inner=2048)


def elapsed_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--model_reps", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "resample_probe.py needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from cleanumamba_amd import hip
    from cleanumamba_amd.util.resample import _launch, out_length, plan, resample_ragged
    hip.lib()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/resample_probe.py: {args.clips} clips of {args.seconds} s, {args.reps} launches per figure, "
        f"{torch.cuda.get_device_name(dev)}")
    g = torch.Generator().manual_seed(0)
    for rate_in, rate_out, dtype in ((48000, 16000, torch.int16), (16000, 48000, torch.float32), (44100, 16000, torch.int16)):
        p = plan(rate_in, rate_out)
        L = int(args.seconds * rate_in)
        x = (3000 * torch.randn(args.clips, L, generator=g)).clamp(-32768, 32767)
        x = (x.to(torch.int16) if dtype == torch.int16 else x / 32768.0).to(dev)
        lens = torch.full((args.clips,), L, dtype=torch.int32, device=dev)
        n = out_length(L, p.up, p.down)
        out = torch.empty(args.clips, -(-n // 8) * 8, dtype=torch.float32, device=dev)
        run = lambda: _launch(p, x, lens, None, True, out, n)          # the launch alone, as resample_ragged makes it
        for _ in range(3):
            run()
        ms = elapsed_ms(run, args.reps)
        nbytes = args.clips * (L * x.element_size() + n * 4)
        fma = args.clips * n * p.K
        rate = nbytes / (ms * 1e-3)
        say(f"resample_ragged {rate_in:>5} -> {rate_out:>5} ({p.up}/{p.down}, K {p.K}, {str(dtype)[6:]} in): {ms * 1e3:9.1f} us "
            f"per launch; {nbytes / 1e6:7.1f} MB in + out = {rate / 1e12:6.3f} TB/s = {rate / HBM_PEAK:6.3f} of the HBM peak "
            f"({rate / HBM_COPY:5.3f} of a copy's rate); {fma / 1e9:5.2f} Gfma = {fma / (ms * 1e-3) / 1e12:5.2f} Tfma/s")

    from conftest import load_ckpt
    from oracle import synth
    from cleanumamba_amd.network import CleanUMamba
    sd, cfg = load_ckpt("442k")
    small = CleanUMamba(**cfg)
    small.load_state_dict(sd, strict=True)
    big = CleanUMamba(**E8)
    big.load_state_dict(synth.fill_state_dict({k: tuple(v.shape) for k, v in big.state_dict().items()}, seed=0), strict=True)
    L48 = int(args.seconds * 48000)
    clips48 = [(3000 * torch.randn(L48, generator=g)).clamp(-32768, 32767).to(torch.int16).to(dev) for _ in range(args.clips)]
    y, n = resample_ragged(torch.stack(clips48), [L48] * args.clips, 48000, 16000)
    clips16 = [y[b, :n[b]].clone() for b in range(args.clips)]
    del y
    for name, model, ac in (("442k_f32", small, None), ("e8_synth_f16", big, torch.float16)):
        model = model.to(dev).float().eval()
        amp = torch.autocast("cuda", dtype=ac) if ac is not None else torch.autocast("cuda", enabled=False)
        with torch.no_grad(), amp:
            a = lambda: model.denoise_batch(clips48, rates=48000)
            b = lambda: model.denoise_batch(clips16)
            a(), b()
            ta, tb = [], []
            for _ in range(args.model_reps):
                ta.append(elapsed_ms(a, 1))
                tb.append(elapsed_ms(b, 1))
            # one instrumented pass of A: device events around what the rates add -- the two conversions (table lookup,
            # length table upload and the launch) and the stackings of clips into rows they need
            from cleanumamba_amd.network import ragged as rg
            from cleanumamba_amd.util import resample as rs
            spans = {"resample_ragged": [], "stack_clips": []}
            real = {"resample_ragged": rs.resample_ragged, "stack_clips": rg.stack_clips}

            def timed(kind):
                def call(*args_, **kw):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out = real[kind](*args_, **kw)
                    e1.record()
                    spans[kind].append((e0, e1))
                    return out
                return call
            rs.resample_ragged, rg.stack_clips = timed("resample_ragged"), timed("stack_clips")
            try:
                ti = elapsed_ms(a, 1)
            finally:
                rs.resample_ragged, rg.stack_clips = real["resample_ragged"], real["stack_clips"]
            parts = {k: (len(v), round(sum(e0.elapsed_time(e1) for e0, e1 in v), 3)) for k, v in spans.items()}
        ma, mb = float(np.median(ta)), float(np.median(tb))
        say(f"denoise_batch {name}: instrumented pass with rates {ti:.2f} ms: " + ", ".join(
            f"{k} {c} calls {ms} ms" for k, (c, ms) in parts.items()) + " (stack_clips: the calls of the two conversions "
            "and those of the batches both routes make)")
        say(f"denoise_batch {name}: 48 kHz with rates=48000 {[round(t, 2) for t in ta]} ms (median {ma:.2f}); the same clips "
            f"already at 16 kHz, no rates {[round(t, 2) for t in tb]} ms (median {mb:.2f}); with / without = {ma / mb:.4f}")
        del model
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
