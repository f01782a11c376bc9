"""Long-recording denoising on the GPU: whole-signal forward against model.denoise_long against feed + flush.

E8, batch 1, 16 kHz, f32 and f16 autocast, 60 s and 600 s of audio (seeded noise).  Per route: seconds of audio per second
of wall clock (host clock around work that ends in a device synchronise; every shape is run once before it is timed) and
torch.cuda.max_memory_allocated over the call, weights excluded.  denoise_long gets a HOST tensor and returns one, as a
file denoiser would call it; forward gets a device tensor (its input and output are part of what it needs resident).
feed + flush is the f32 streaming algorithm (running per-frame std): it has no autocast mode, so it is listed once per
length, under f32.

    python tools/bench_block_denoise.py [--seconds 60 600] [--out profiles/block_denoise.json]

Writes one JSON document.  A route that does not fit is recorded as {"error": ...}, not skipped silently."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                    # noqa: E402  (the E8 configuration)
from cleanumamba_amd.network import Net                         # noqa: E402

SR = 16000


def measure(fn, reps):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    return dt, torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, nargs="+", default=[60, 600])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_denoise.json"))
    ap.add_argument("--feed-chunk", type=int, default=16000, help="samples per feed() call")
    ap.add_argument("--feed-budget", type=float, default=150.0, help="skip a feed + flush run projected to take longer (s)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_block_denoise needs a GPU")
    dev = torch.device("cuda")
    torch.manual_seed(0)
    net = Net("CleanUMamba", bench.E8).to(dev).eval()
    hop = net.total_stride
    res = {"model": "E8", "batch": 1, "sample_rate": SR, "block_samples": 625 * hop, "device": torch.cuda.get_device_name(0),
           "runs": []}
    feed_rate = None
    for secs in args.seconds:
        L = secs * SR
        x_host = 0.05 * torch.randn(1, 1, L, generator=torch.Generator().manual_seed(secs))
        reps = 3 if secs <= 60 else 1
        for dtype in ("f32", "f16"):
            def cast():
                return torch.autocast("cuda", dtype=torch.float16, enabled=dtype == "f16")
            row = {"seconds_of_audio": secs, "dtype": dtype}

            def whole():
                with torch.no_grad(), cast():
                    return net(x_dev)

            def blocks():
                with cast():
                    return net.denoise_long(x_host)
            try:
                x_dev = x_host.to(dev)
                whole()                                      # warm-up of this shape
                dt, peak = measure(whole, reps)
                row["forward"] = {"audio_s_per_s": secs / dt, "seconds": dt, "peak_bytes": peak}
                ref = whole().cpu()
            except torch.OutOfMemoryError as e:
                row["forward"] = {"error": "out of memory: " + str(e).split("\n")[0]}
                ref = None
            x_dev = None
            torch.cuda.empty_cache()
            blocks()
            dt, peak = measure(blocks, reps)
            row["denoise_long"] = {"audio_s_per_s": secs / dt, "seconds": dt, "peak_bytes": peak}
            if ref is not None:
                out = blocks()
                row["denoise_long"]["rel_l2_to_forward"] = ((out - ref).norm() / ref.norm()).item()
                row["denoise_long"]["cost_vs_forward"] = row["denoise_long"]["seconds"] / row["forward"]["seconds"]
                del out, ref
            if dtype == "f32":
                def stream():
                    with torch.no_grad():
                        net.reset_stream()
                        for i in range(0, L, args.feed_chunk):
                            net.feed(x_feed[:, i:i + args.feed_chunk])
                        net.flush()
                if feed_rate is not None and secs / feed_rate > args.feed_budget:
                    row["feed_flush"] = {"skipped": f"projected {secs / feed_rate:.0f} s at the measured "
                                                    f"{feed_rate:.1f} s of audio per second (memory does not depend on length)"}
                else:
                    x_feed = x_host[0].to(dev)
                    with torch.no_grad():                    # warm-up: one second of hops (captures the hop graph)
                        net.reset_stream()
                        net.feed(x_feed[:, :SR])
                        net.flush()
                    dt, peak = measure(stream, 1)
                    feed_rate = secs / dt
                    row["feed_flush"] = {"audio_s_per_s": feed_rate, "seconds": dt, "peak_bytes": peak}
                    del x_feed
            print(json.dumps(row), flush=True)
            res["runs"].append(row)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
