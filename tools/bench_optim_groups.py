"""Cost of parameter groups in the flat optimizer's update on the E8 model (41.4 M elements, the real 103-tensor layout):
cum_optim_adam (one group; A) against cum_optim_adam_groups with the reference's two AdamW groups, decoupled decay (B), in
one process, alternating A B A B.  Each repetition times ``--launches`` back-to-back launches between two device events;
every repetition is recorded.  The verdict asked of B: its median may exceed A's by no more than the spread of A's own
repetitions (max - min).
Usage: python tools/bench_optim_groups.py [--out profiles/optim_groups.json] [--reps 10] [--launches 200]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES_PER_ELEMENT = 28         # p, g, m, v read; p, m, v written (f32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_groups.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from cleanumamba_amd import hip
    from cleanumamba_amd.network import CleanUMamba
    from cleanumamba_amd.training.flat_optim import FlatAdam, FlatParams
    from cleanumamba_amd.training.train_step import decay_groups
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim_groups: needs a GPU (a CPU run says nothing about the kernels)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = CleanUMamba(channels_H=64, max_H=768, encoder_n_layers=8, tsfm_n_layers=3, tsfm_n_head=8, tsfm_d_model=512,
                      tsfm_d_inner=2048).to(dev).train()
    flat = FlatParams(net)
    lib = hip.lib()
    opt_a = FlatAdam(flat, lr=1e-6, weight_decay=0.01, max_grad_norm=10)
    opt_b = FlatAdam(flat, lr=1e-6, max_grad_norm=10, groups=decay_groups(net, 0.01), decoupled_weight_decay=True)
    flat.grad.normal_(0.0, 1e-3, generator=torch.Generator(device=dev).manual_seed(1))
    for p, o in zip(flat.params, flat.offsets):                    # the alignment padding stays zero
        end = o + (p.numel() + 3) // 4 * 4
        flat.grad[o + p.numel():end].zero_()
    opt_a.step()                                                   # a valid state vector (step 1, no inf) for each
    opt_b.step()
    torch.cuda.synchronize()
    st = hip.stream_ptr()
    g = opt_a.param_groups[0]

    def launch_a():
        hip.check(lib.cum_optim_adam(hip.ptr(flat.data), hip.ptr(flat.grad), hip.ptr(opt_a.exp_avg),
                                     hip.ptr(opt_a.exp_avg_sq), flat.numel, hip.ptr(opt_a.state_vec), g["betas"][0],
                                     g["betas"][1], g["eps"], g["weight_decay"], st))

    def launch_b():
        hip.check(lib.cum_optim_adam_groups(hip.ptr(flat.data), hip.ptr(flat.grad), hip.ptr(opt_b.exp_avg),
                                            hip.ptr(opt_b.exp_avg_sq), flat.numel, hip.ptr(opt_b.state_vec),
                                            g["betas"][0], g["betas"][1], g["eps"], 1, hip.ptr(opt_b.group_hyper), 2,
                                            hip.ptr(opt_b.tile_group), hip.ptr(opt_b.seg_end), hip.ptr(opt_b.seg_group),
                                            opt_b.seg_end.numel(), st))

    def timed(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(args.launches):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / args.launches

    for fn in (launch_a, launch_b):
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    reps = {"A": [], "B": []}
    for _ in range(args.reps):
        reps["A"].append(round(timed(launch_a), 5))
        reps["B"].append(round(timed(launch_b), 5))
    med = {k: statistics.median(v) for k, v in reps.items()}
    spread_a = max(reps["A"]) - min(reps["A"])
    decayed = sum(p.numel() for p in opt_b.param_groups[0]["params"])
    res = {"model": "E8", "elements": flat.numel, "parameters": len(flat.params), "decayed_elements": decayed,
           "tile_elements": lib.cum_optim_group_tile_elems(), "tiles": opt_b.tile_group.numel(),
           "mixed_tiles": int((opt_b.tile_group < 0).sum()), "segments": opt_b.seg_end.numel(),
           "table_bytes": 4 * (opt_b.tile_group.numel() + 2 * opt_b.seg_end.numel()) + 16 * 2,
           "launches_per_repetition": args.launches, "warmup_launches": args.warmup,
           "A": "cum_optim_adam, one group, L2 decay 0.01", "B": "cum_optim_adam_groups, two groups, decoupled decay 0.01 / 0",
           "ms_per_launch": reps, "median_ms": {k: round(v, 5) for k, v in med.items()},
           "A_spread_ms": round(spread_a, 5), "B_over_A": round(med["B"] / med["A"], 4),
           "B_minus_A_ms": round(med["B"] - med["A"], 5), "B_within_A_spread": bool(med["B"] - med["A"] <= spread_a),
           "tb_per_s": {k: round(BYTES_PER_ELEMENT * flat.numel / v / 1e9, 3) for k, v in med.items()}}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
