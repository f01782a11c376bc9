"""Cost of channel pruning on the E8 model (41.4 M parameters) held by a TrainStep: importances of all groups (one
cum_prune_importance launch) against the same five sums as per-module torch expressions (the reference's form), one
compaction of the four flat buffers (cum_prune_gather) with its share of the HBM peak -- kernel times from the profiler,
warm, averaged over --reps calls --, and the TrainStep calls after a prune (eager until the graph is recaptured three
steps later) beside the first calls of the unpruned model, with the host functions that dominate them.
Usage: python tools/bench_prune.py [--out profiles/prune_bench.json]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # MI355X HBM3E, bytes / s


def torch_sums(groups):
    """The reference's per-module expressions (src/pruning/pruninggroup.py channel_importances) on the GPU."""
    out = []
    for g in groups:
        for pm in g.modules:
            p = pm.param()
            w, gr = p.data, p.grad
            if pm.dim == 1:
                w, gr = w.transpose(1, 0), gr.transpose(1, 0)
            w = w.flatten(1) if w.dim() > 2 else (w.unsqueeze(1) if w.dim() == 1 else w)
            gr = gr.flatten(1) if gr.dim() > 2 else (gr.unsqueeze(1) if gr.dim() == 1 else gr)
            n = g.n_channels * pm.n_heads
            w = w[pm.channel_offset:pm.channel_offset + n].reshape(g.n_channels, -1)
            gr = gr[pm.channel_offset:pm.channel_offset + n].reshape(g.n_channels, -1)
            wg = w * gr
            out += [w.abs().pow(2).sum(1), gr.abs().pow(2).sum(1), wg.abs().sum(1), wg.pow(2).sum(1), wg.sum(1).abs()]
    return out


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


USE_TORCH_PROFILER = True      # off (--no-torch-profiler) under an external tracer such as rocprofv3 --kernel-trace


def kernel_ms(fn, name, reps):
    """Mean device time (ms) of the kernels whose name contains ``name`` over ``reps`` warm calls of ``fn`` (None with
    the profiler off: the calls still run, for an external tracer to time)."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    if not USE_TORCH_PROFILER:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return None
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    total, n = 0.0, 0
    for e in prof.events():
        if name in e.name and e.device_type == torch.autograd.DeviceType.CUDA:
            total += e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total
            n += 1
    return round(total / n / 1e3, 4) if n else None


def step_times(step, clean, noisy, n, profile_first=0):
    """Wall ms of ``n`` TrainStep calls, each synchronised; with ``profile_first`` the first calls also run under cProfile
    and the ten functions with the most own time are returned beside."""
    import cProfile
    import pstats
    times, prof = [], cProfile.Profile()
    for i in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if i < profile_first:
            prof.enable()
        step(clean, noisy)
        torch.cuda.synchronize()
        if i < profile_first:
            prof.disable()
        times.append(round(1e3 * (time.perf_counter() - t0), 3))
    if not profile_first:
        return times
    st = pstats.Stats(prof)
    top = sorted(st.stats.items(), key=lambda kv: -kv[1][2])[:10]
    return times, [{"function": f"{os.path.basename(k[0])}:{k[1]}:{k[2]}", "calls": v[1], "own_ms": round(1e3 * v[2], 2),
                    "cumulative_ms": round(1e3 * v[3], 2)} for k, v in top]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prune_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-torch-profiler", action="store_true")
    args = ap.parse_args()
    global USE_TORCH_PROFILER
    USE_TORCH_PROFILER = not args.no_torch_profiler
    from cleanumamba_amd import hip
    from cleanumamba_amd.network import CleanUMamba
    from cleanumamba_amd.pruning import CleanUMambaPrunableChannels, get_prune_channels, prune
    from cleanumamba_amd.pruning import device as D
    from cleanumamba_amd.training.train_step import TrainStep
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = CleanUMamba(channels_H=64, max_H=768, encoder_n_layers=8, tsfm_n_layers=3, tsfm_n_head=8, tsfm_d_model=512,
                      tsfm_d_inner=2048).to(dev).train()
    n_params = sum(p.numel() for p in net.parameters())
    step = TrainStep(net)
    g = torch.Generator().manual_seed(1)
    clean = (0.1 * torch.randn(4, 1, 32000, generator=g)).to(dev)
    noisy = clean + 0.05 * torch.randn(clean.shape, generator=g).to(dev)
    res = {"model": "E8", "parameters": n_params}
    res["train_step_ms_initial"] = step_times(step, clean, noisy, 5)
    groups = CleanUMambaPrunableChannels(net)
    res.update(groups=len(groups), channels=sum(x.n_channels for x in groups))
    items = [(pm, x.n_channels) for x in groups for pm in x.modules]
    res["importances_hip_call_ms"] = round(timed(lambda: D._launch(items), args.reps), 4)
    res["importances_hip_kernel_ms"] = kernel_ms(lambda: D._launch(items), "prune_importance_kernel", args.reps)
    res["importances_torch_per_module_ms"] = round(timed(lambda: torch_sums(groups), args.reps), 4)
    res["importances_read_bytes"] = sum(2 * 4 * pm.param().numel() for pm, _ in items)
    if res["importances_hip_kernel_ms"]:
        res["importances_kernel_tb_per_s"] = round(res["importances_read_bytes"] / res["importances_hip_kernel_ms"] / 1e9, 3)

    # one compaction inside prune(); its arguments are kept, with the old buffers alive, to time the kernel alone, warm,
    # by repeating the same gather (it rewrites the live new buffers with the values they already hold)
    flat, opt = step.buckets.flat, step.optimizer
    chosen, _, _ = get_prune_channels(groups, "taylor_squared_individual*n_filters/n_parameters", None, 0.01, 8)
    old_numel = flat.numel
    old_buffers = (flat.data, flat.grad, opt.exp_avg, opt.exp_avg_sq)
    lib = hip.lib()
    orig = lib.cum_prune_gather
    captured = []

    def gather(*a):
        captured.append(a)
        return orig(*a)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lib.cum_prune_gather = gather
    try:
        prune(groups, chosen, opt)
    finally:
        lib.cum_prune_gather = orig
    torch.cuda.synchronize()
    res["prune_call_total_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
    a = list(captured[0])
    ws = torch.empty(int(a[15]), dtype=torch.uint8, device=dev)
    a[14] = hip.ptr(ws)

    def regather():
        a[16] = hip.stream_ptr()
        hip.check(orig(*a))
    gms = kernel_ms(regather, "prune_gather_kernel", args.reps)
    descs = a[0]
    elem_path = sum(d.n_new for d in descs[:a[1]]
                    if not ((d.keep[d.ndim - 1] < 0 and d.new_dims[d.ndim - 1] % 4 == 0) or max(d.keep) < 0))
    moved = 4 * 4 * 2 * flat.numel                      # four buffers: read kept + write new, f32
    del old_buffers
    res.update(channels_pruned=len(chosen), flat_elements_before=old_numel, flat_elements_after=flat.numel,
               gather_elements_on_element_path=elem_path, compaction_kernel_ms=gms, compaction_bytes=moved)
    if gms:
        res.update(compaction_tb_per_s=round(moved / gms / 1e9, 3),
                   compaction_share_of_hbm_peak=round(moved / gms / 1e9 / (HBM_PEAK / 1e12), 3))

    # TrainStep calls after the prune: eager (the graph is recaptured at the fourth); the host functions that dominate
    # the first two are recorded
    res["train_step_ms_after_prune"], res["after_prune_host_top"] = step_times(step, clean, noisy, 5, profile_first=2)
    res["graph_status"] = step.graph_status
    res["steady_step_ms"] = round(timed(lambda: step(clean, noisy), args.reps), 3)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
