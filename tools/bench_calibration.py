"""Wall time of one layer-wise calibration gather on E8 (cleanumamba_amd/pruning/layerwise_calibration.py).

A seeded model of the E8 configuration (41.4 M parameters), 128 synthetic clips of 10 s at batch 16 (8 batches), the
one-point calibration that ``calibrator.gather`` runs.  Two forms in the same process, each after a warm-up gather:
  * masked: the trials zero the selection in place (cum_prune_mask) and run on the model itself; d_model is pruned
    physically on a scratch copy;
  * copy: every trial on a scratch copy pruned through prune() (the reference's deepcopy + group.prune route).
Host wall times per phase (the phase boundaries synchronise the device) and the loss changes of both forms.
Usage: python tools/bench_calibration.py [--out profiles/calibration_bench.json] [--clips 128] [--batch 16]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calibration_bench.json"))
    ap.add_argument("--clips", type=int, default=128)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--skip-copy", action="store_true")
    args = ap.parse_args()
    from cleanumamba_amd.network import CleanUMamba
    from cleanumamba_amd.pruning import CleanUMambaPrunableChannels
    from cleanumamba_amd.pruning.layerwise_calibration import calibrate_prune_groups
    from cleanumamba_amd.util.util import loss_fn
    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    net = CleanUMamba(channels_H=64, max_H=768, encoder_n_layers=8, tsfm_n_layers=3, tsfm_n_head=8, tsfm_d_model=512,
                      tsfm_d_inner=2048).to(dev).train()
    L = int(args.seconds * 16000)
    g = torch.Generator(device=dev).manual_seed(11)
    data = []
    for _ in range(args.clips // args.batch):
        clean = 0.05 * torch.randn(args.batch, 1, L, generator=g, device=dev)
        data.append((clean, clean + 0.05 * torch.randn(args.batch, 1, L, generator=g, device=dev)))
    groups = CleanUMambaPrunableChannels(net)
    metric = "n_parameters*taylor_squared_individual"
    out = {"model": "E8 (seeded)", "clips": args.clips, "batch": args.batch, "seconds_per_clip": args.seconds,
           "groups": len(groups), "device": torch.cuda.get_device_name(dev)}

    def run(physical, tag):
        t = {}
        net.zero_grad()
        t0 = time.perf_counter()
        rows = calibrate_prune_groups(net, groups, [0.2], loss_fn, metric, data, loss_samples=args.clips,
                                      batch_size=args.batch, physical=physical, timings=t)
        torch.cuda.synchronize()
        t["total"] = time.perf_counter() - t0
        t["trials"] = len(rows)
        t["masked_trial_count"] = 0 if physical else sum(r["group"] != "d_model" for r in rows)
        print(tag, json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in t.items()}), flush=True)
        return t, rows

    run(False, "warm-up")
    t_mask, rows_mask = run(False, "masked")
    out["masked"] = t_mask
    if not args.skip_copy:
        t_copy, rows_copy = run(True, "copy")
        out["copy"] = t_copy
        out["speedup_total"] = t_copy["total"] / t_mask["total"]
        out["loss_change"] = {r["group"]: [r["loss_change"], q["loss_change"]] for r, q in zip(rows_mask, rows_copy)}
        out["max_rel_trial_loss_diff_masked_groups"] = max(
            abs(r["loss_change"] - q["loss_change"]) / abs(q["loss_change"] + t_copy["baseline_loss"])
            for r, q in zip(rows_mask, rows_copy) if r["group"] != "d_model")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "loss_change"}, indent=1))


if __name__ == "__main__":
    main()
