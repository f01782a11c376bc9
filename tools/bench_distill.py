"""bench_distill.py -- what does fine-tuning against a teacher (training/distill.py, csrc/distill.hip) cost?

  python tools/bench_distill.py [--steps 10] [--warmup 6] [--rounds 2] [--skip-steps] [--out FILE]

The E8 batch of bench.py throughout (B = 16, 10 s crops = 160 000 samples, f16 autocast):

  alone   the three passes on features of the E8 model's nine shapes (row buffers of the conv stack, f16), on an idle
          device between two events, in alternating windows; each pass against a device copy (``Tensor.copy_``) that moves
          the same number of bytes, timed by the same loop:
            stats  reads e and t                 (2 N bytes)
            loss   reads e and t                 (2 N bytes)
            bwd    reads e and t, writes d/de    (3 N bytes)         N = bytes of all e
  steps   ONE process, alternating windows of ``--steps`` steps between two device synchronisations:
            P  TrainStep(student)                             -- the step without a teacher, the yardstick
            K  TrainStep(student, distill=(teacher, adapters)) on the kernels
            F  the same on the torch fallback (training.distill.kernel_route forced off)
          with the peak of the allocator over each mode's warm-up (eager steps and the capture).  The student is the E8
          model with a few channels of two groups pruned, the teacher the E8 model.

The last line is the result as JSON.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def feature_shapes(net, B, L):
    """[(B, C, T)] of forward(x, return_skip_connections=True) for an input of L samples."""
    from cleanumamba_amd.training.distill import feature_channels
    T, ts = net.valid_length(L), []
    for _ in range(net.encoder_n_layers):
        T = (T - net.kernel_size) // net.stride + 1
        ts.append(T)
    ts = ts[::-1] + [ts[-1]]
    return [(B, c, t) for c, t in zip(feature_channels(net), ts)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--crop-seconds", type=float, default=10.0)
    ap.add_argument("--skip-steps", action="store_true", help="only the passes alone")
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args()

    assert torch.cuda.is_available(), "bench_distill.py needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    import bench_feeder as bf
    from cleanumamba_amd import hip
    from cleanumamba_amd.network import Net, convstack as cs
    from cleanumamba_amd.training import distill as D
    lib = hip.lib()
    B, L = args.batch, int(args.crop_seconds * bf.RATE)
    torch.manual_seed(0)
    teacher = Net("CleanUMamba", bf.E8).to(dev)

    # ---- the passes alone
    def timed(fn, n=20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n
    shapes = feature_shapes(teacher, B, L)
    n = len(shapes)
    recs, keep, n_bytes = (hip.DistillLayer * n)(), [], 0
    for i, (b_, c, t) in enumerate(shapes):
        geo = cs.Geo(b_, t, c)
        bufs = [torch.zeros(geo.R, geo.Cp, dtype=torch.float16, device=dev) for _ in range(3)]
        for buf in bufs[:2]:
            geo.rows(buf)[:, :t, :c] = torch.randn(b_, t, c, device=dev).to(torch.float16)
        e, tt, de = (cs.from_rows(buf, geo).transpose(1, 2) for buf in bufs)
        recs[i] = D._layer_record(e, tt, de, None, None, 1e-4, 0.1)
        keep.append(bufs)
        n_bytes += 2 * b_ * t * geo.Cp
    sizes = (hip.c_i64 * 3)()
    hip.check(lib.cum_distill_sizes(recs, n, sizes))
    part = torch.empty(max(int(sizes[0]), 4), dtype=torch.float32, device=dev)
    cst = torch.empty(int(sizes[1]) * 8, dtype=torch.float32, device=dev)
    csum = torch.empty(int(sizes[1]) * 2, dtype=torch.float64, device=dev)
    s4 = torch.empty(int(sizes[2]), dtype=torch.float32, device=dev)
    Dv, Lv = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    G = torch.full((n,), 1024.0 / n, device=dev)

    def fwd(passes):
        hip.check(lib.cum_distill_fwd(recs, n, 1.0, passes, hip.ptr(part), hip.ptr(cst), hip.ptr(csum), hip.ptr(s4),
                                      hip.ptr(Dv), hip.ptr(Lv), hip.stream_ptr()))
    moved = {"stats": 2 * n_bytes, "loss": 2 * n_bytes, "bwd": 3 * n_bytes}
    copies = {k: (torch.empty(v // 2, dtype=torch.uint8, device=dev), torch.empty(v // 2, dtype=torch.uint8, device=dev))
              for k, v in moved.items() if k != "loss"}
    copies["loss"] = copies["stats"]
    calls = {"stats": lambda: fwd(1), "loss": lambda: fwd(2),
             "bwd": lambda: hip.check(lib.cum_distill_bwd(recs, n, 1.0, hip.ptr(cst), hip.ptr(csum), hip.ptr(Dv), hip.ptr(G),
                                                          hip.stream_ptr()))}
    for k in ("stats", "loss", "bwd"):
        calls[k]()
        copies[k][0].copy_(copies[k][1])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(Lv).all()), Lv
    alone = {}
    for k in ("stats", "loss", "bwd"):
        ms, ms_copy = [], []
        for _ in range(args.rounds):
            ms.append(timed(calls[k]))
            ms_copy.append(timed(lambda: copies[k][0].copy_(copies[k][1])))
        m, mc = sum(ms) / len(ms), sum(ms_copy) / len(ms_copy)
        alone[k] = {"ms": round(m, 4), "spread_ms": round(max(ms) - min(ms), 4), "bytes": moved[k],
                    "GB_per_s": round(moved[k] / (m * 1e-3) / 1e9, 1), "copy_ms": round(mc, 4),
                    "copy_GB_per_s": round(moved[k] / (mc * 1e-3) / 1e9, 1), "frac_of_copy": round(mc / m, 3)}
        print(f"alone {k}: {alone[k]}", flush=True)
    result = {"tool": "tools/bench_distill.py", "batch": B, "length": L, "layers": [list(s) for s in shapes],
              "feature_bytes_per_side": n_bytes, "alone": alone,
              "workspace_MB": round((4 * part.numel() + 4 * cst.numel() + 8 * csum.numel() + 4 * s4.numel()) / 1e6, 2)}
    del keep, copies, part
    torch.cuda.empty_cache()

    # ---- the steps
    if not args.skip_steps:
        from cleanumamba_amd.pruning import CleanUMambaPrunableChannels, prune
        from cleanumamba_amd.training.train_step import TrainStep
        from oracle import synth
        real_route = D.kernel_route
        state = {k: v.detach().clone() for k, v in teacher.state_dict().items()}

        def student():
            net = Net("CleanUMamba", bf.E8).to(dev).train()
            net.load_state_dict(state)
            groups = CleanUMambaPrunableChannels(net)
            prune(groups, {groups[0]: [1, 29], groups[3]: [1, 61]}, None)
            return net
        steps, force = {}, {"P": None, "K": real_route, "F": lambda *a: False}
        for tag in ("P", "K", "F"):
            net = student()
            distill = None if tag == "P" else (teacher, D.make_adapters(net, teacher))
            steps[tag] = TrainStep(net, autocast_dtype=torch.float16, loss_config={"kd_p": 1}, distill=distill)
        clean, noisy = (x.to(dev) for x in synth.waveform(B, L, seed=1))

        def run(tag, k):
            D.kernel_route = force[tag] or real_route
            try:
                for _ in range(k):
                    steps[tag](clean, noisy)
            finally:
                D.kernel_route = real_route
        windows, peak = [], {}
        for tag in steps:                 # warm-up: three eager steps, the capture, replays -- and the mode's peak memory
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            run(tag, args.warmup)
            torch.cuda.synchronize()
            peak[tag] = torch.cuda.max_memory_allocated() - base
        for _ in range(args.rounds):
            for tag in steps:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(tag, args.steps)
                torch.cuda.synchronize()
                ms = 1e3 * (time.perf_counter() - t0) / args.steps
                windows.append({"mode": tag, "ms_per_step": round(ms, 3)})
                print(f"{tag}: {ms:.3f} ms/step, graph {steps[tag].graph_status}", flush=True)
        mean = {tag: sum(w["ms_per_step"] for w in windows if w["mode"] == tag) / args.rounds for tag in steps}
        result.update(workload=f"CleanUMamba-E8 train step, B={B}, {args.crop_seconds:g} s crops, f16 autocast",
                      steps_per_window=args.steps, warmup=args.warmup, windows=windows,
                      graph_status={tag: s.graph_status for tag, s in steps.items()},
                      mean_ms={k: round(v, 3) for k, v in mean.items()},
                      peak_allocated_GB={k: round(v / 1e9, 3) for k, v in peak.items()},
                      note="peak_allocated: the allocator's peak over a mode's warm-up (eager steps, capture, replays) above "
                           "what was allocated before it: activations, the graph's pool and the optimizer state",
                      K_minus_P_ms=round(mean["K"] - mean["P"], 3), F_minus_K_ms=round(mean["F"] - mean["K"], 3))
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
