"""bench_validate.py -- is ``validate(batching="ragged")`` at least as fast as the ``"length"`` route on a test set of
mixed lengths?

  python tools/bench_validate.py [--pairs 64] [--rounds 2] [--out profiles/validate_bench.json]

Writes a seeded VCTK-style test set (the same file name in ``clean/`` and ``noisy/``) of ``--pairs`` 16-bit mono pairs of
2 - 12 s into a temporary directory, once at 16 kHz and once at 48 kHz (scored with ``resample=True``), and runs
``validate`` on the shipped 442k checkpoint in f32 by two routes, A B A B ... ``--rounds`` times after one warm-up pass
of each, in one process:

  A  ``batching="length"``: clips of equal length share a forward (here practically none do), the result is quantised
     per group and brought to the host, and the host arrays are uploaded again for scoring -- the route before this tool;
  B  ``batching="ragged"``: clips of any lengths share forwards, quantised on the device into one flat int16 buffer and
     scored where they stand.

Every window is one whole ``validate`` call between two device synchronisations on the host clock, file reading included
on both routes (the files are in the page cache after the warm-up).  One more pass of each route, not timed, counts the
forwards and the bytes ``Tensor.to`` / ``Tensor.cpu`` move between host and device (tables built by ``torch.tensor(...,
device=...)`` are not seen: a few hundred bytes).  The last line is the result as JSON.
"""
import argparse
import json
import os
import sys
import tempfile
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

EXTRA = ("estoi", "si_sdr")


def write_set(root, pairs, rate, seed=0):
    from scipy.io import wavfile
    os.makedirs(os.path.join(root, "clean"))
    os.makedirs(os.path.join(root, "noisy"))
    rng = np.random.default_rng(seed)
    lengths = []
    for i in range(pairs):
        n = int(rng.integers(2 * rate, 12 * rate + 1))
        spec = np.fft.rfft(rng.standard_normal(n))
        f = np.fft.rfftfreq(n, 1.0 / rate)
        spec[(f < 300) | (f > 3400)] = 0
        x = np.fft.irfft(spec, n)
        env = np.repeat(rng.choice([0.15, 1.0], size=n // (rate // 10) + 1), rate // 10)[:n]
        clean = np.round(9000 * env * x / np.abs(x).max())
        noisy = np.clip(np.round(clean + 1200 * rng.standard_normal(n)), -32768, 32767)
        wavfile.write(os.path.join(root, "clean", f"p{i:03d}.wav"), rate, clean.astype(np.int16))
        wavfile.write(os.path.join(root, "noisy", f"p{i:03d}.wav"), rate, noisy.astype(np.int16))
        lengths.append(n)
    return lengths


class Traffic:
    """Counts what ``Tensor.to`` and ``Tensor.cpu`` carry across the host / device boundary while it is active."""

    def __enter__(self):
        self.h2d = self.d2h = 0
        self._to, self._cpu = torch.Tensor.to, torch.Tensor.cpu
        counter = self

        def to(t, *a, **k):
            out = counter._to(t, *a, **k)
            if out.is_cuda != t.is_cuda:
                nbytes = out.numel() * out.element_size()
                counter.h2d += nbytes if out.is_cuda else 0
                counter.d2h += 0 if out.is_cuda else nbytes
            return out

        def cpu(t, *a, **k):
            if t.is_cuda:
                counter.d2h += t.numel() * t.element_size()
            return counter._cpu(t, *a, **k)
        torch.Tensor.to, torch.Tensor.cpu = to, cpu
        return self

    def __exit__(self, *exc):
        torch.Tensor.to, torch.Tensor.cpu = self._to, self._cpu


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_validate.py needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from conftest import load_ckpt
    from cleanumamba_amd import hip
    from cleanumamba_amd.network import CleanUMamba, blockdenoise
    from cleanumamba_amd.network import ragged as rg
    from cleanumamba_amd.util.denoise_eval import validate
    hip.lib()
    sd, cfg = load_ckpt("442k")
    net = CleanUMamba(**cfg)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).float().eval()

    forwards = {"n": 0}
    net.register_forward_hook(lambda *a: forwards.__setitem__("n", forwards["n"] + 1))     # route A: net(x)
    real_ragged, real_long = rg.forward_ragged, blockdenoise.denoise_long

    def counted(fn):
        def call(*a, **k):
            forwards["n"] += 1
            return fn(*a, **k)
        return call
    rg.forward_ragged, blockdenoise.denoise_long = counted(real_ragged), counted(real_long)    # route B

    variants = []
    warnings.simplefilter("ignore")
    for rate, kw in ((16000, {}), (48000, {"resample": True})):
        tmp = tempfile.TemporaryDirectory(prefix="validate_bench_")
        lengths = write_set(tmp.name, args.pairs, rate)
        audio_s = sum(lengths) / rate
        print(f"{rate} Hz: {args.pairs} pairs, {audio_s:.1f} s of audio", flush=True)

        def window(tag, batching):
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = validate(net, tmp.name, VCTK_DEMAND=True, extra_metrics=EXTRA, batching=batching, **kw)
            torch.cuda.synchronize()
            el = time.perf_counter() - t
            print(f"{rate} Hz {tag}: {el * 1e3:9.1f} ms per pass   {args.pairs / el:8.1f} clips / s", flush=True)
            return {"mode": tag, "seconds": round(el, 4), "clips_per_s": round(args.pairs / el, 2)}, res

        (_, ra), (_, rb) = window("warm A", "length"), window("warm B", "ragged")
        windows = []
        for _ in range(args.rounds):
            windows += [window("A", "length")[0], window("B", "ragged")[0]]
        counts = {}
        for tag, batching in (("A", "length"), ("B", "ragged")):
            forwards["n"] = 0
            with Traffic() as tr:
                window(tag + " counted", batching)
            counts[tag] = {"forwards": forwards["n"], "host_to_device_bytes": tr.h2d, "device_to_host_bytes": tr.d2h}
        a = [w["seconds"] for w in windows if w["mode"] == "A"]
        b = [w["seconds"] for w in windows if w["mode"] == "B"]
        diff = {k: float(np.float64(rb[k]) - np.float64(ra[k])) for k in sorted(ra)}
        variants.append({"rate": rate, "resample": bool(kw), "pairs": args.pairs, "audio_seconds": round(audio_s, 2),
                         "windows": windows, "A_seconds": a, "B_seconds": b,
                         "A_clips_per_s": [round(args.pairs / s, 2) for s in a],
                         "B_clips_per_s": [round(args.pairs / s, 2) for s in b],
                         "A_over_B_time": round((sum(a) / len(a)) / (sum(b) / len(b)), 3),
                         "B_not_slower_than_A": bool(max(b) <= min(a)), "counts": counts,
                         "ragged_minus_length_sums": diff,
                         "ragged_minus_length_means": {k: v / ra["Test/count"] for k, v in diff.items()}})
        print(f"{rate} Hz: A {a} s  B {b} s;  A / B = {variants[-1]['A_over_B_time']};  {counts}", flush=True)
        tmp.cleanup()

    result = {"tool": "tools/bench_validate.py", "model": "442k_f32", "extra_metrics": list(EXTRA), "rounds": args.rounds,
              "order": "warm A, warm B, then A B per round, then one counted pass of each", "variants": variants}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
