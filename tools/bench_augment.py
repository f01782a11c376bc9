"""bench_augment.py -- what does training augmentation (training/augment.py, csrc/augment.hip) cost the E8 train step?

  python tools/bench_augment.py [--steps 30] [--warmup 8] [--rounds 2] [--shift 8000] [--out FILE]

Two measurements, the E8 batch of bench.py throughout (B = 16, 10 s crops = 160 000 samples):

  alone   the launches ``PcmBatch.into`` adds, on an idle device between two events (20 each), from float sources of
          L + shift samples:  echo off with the SNR re-drawn (two launches);  echo off, SNR kept (one launch);  and a full
          list of 435 taps on every row (the worst case of the default ``Echo``), SNR re-drawn.  For the echo-off case the
          bytes moved -- three source rows read, c1 / n1 written, read back and written again -- against the time give the
          fraction of the HBM rate (8 TB/s peak).
  fed     tools/bench_feeder.py's method: ONE captured train step, timed in one process in alternating windows of
          ``--steps`` steps between two device synchronisations:
            P  ``step(batch)`` on a feeder without augmentation -- the code path of a build without this feature, the
               yardstick;
            Q  the same with remix + shift + SNR + gain;
            R  the same plus the default echo.

With ``--band`` the same two measurements for the band-mask stage (csrc/bandmask.hip) instead:

  alone   cum_band_mask_pairs (two launches) on L + shift samples per row, every row at the lowest band (W = 800, the
          longest default filter) and at a mid band (edges 60 and 80, W = 17).  Bytes: per signal n read, the halo
          re-reads 2 W / V of n, n written; against the time, the fraction of the HBM rate.
  fed     P and Q as above and M: Q plus the default ``BandMask``.

With ``--reverb`` the same two measurements for the reverb stage (csrc/reverb.hip) instead:

  alone   cum_reverb_pairs (three launches, the best of three runs of 20) on L + shift samples per row, every row with
          a response of T = 2048, 8192 and 16 384 taps (K = T / P partitions, P = N / 2), and with no row reverberant
          (the copy path).  Bytes by the
          design's own count, per row of n samples: the input blocks read C twice (8 n), their spectra are written (16 n),
          every output block reads K block spectra and K partition spectra (32 K n; fewer in the row's first K blocks),
          C and Y are read again and both outputs written (16 n); a copied row moves 16 n.
  fed     P and Q as above, V: nothing but ``Reverb(proba=1)`` at T = 8192, and W: Q plus that reverb.

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
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_PEAK = 8.0e12


def full_draws(nb, length, shift, taps, snr):
    """Draws with ``taps`` taps on every row, spread like the default echo's worst case (3 trains, 161-sample steps)."""
    from cleanumamba_amd.training.augment import K_MAX, AugmentDraws
    rng = np.random.default_rng(0)
    delay, gain = np.zeros((nb, K_MAX), np.int32), np.zeros((nb, K_MAX), np.float32)
    per = max(1, -(-taps // 3))
    d = np.concatenate([161 * (1 + np.arange(per)) + r for r in range(3)])[:taps]
    delay[:, :taps] = d
    gain[:, :taps] = 0.3 * 0.953 ** (np.arange(taps) % per)
    return AugmentDraws(length, shift, rng.permutation(nb), rng.integers(0, shift + 1, nb), rng.integers(0, shift + 1, nb),
                        np.full(nb, 5.0 if snr else np.nan), np.full(nb, 0.8), np.full(nb, 0.1), np.full(nb, taps), delay, gain)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--crop-seconds", type=float, default=10.0)
    ap.add_argument("--clip-seconds", type=float, default=12.0)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--shift", type=int, default=8000)
    ap.add_argument("--dtype", default="f16", choices=["f16", "bf16", "f32"])
    ap.add_argument("--skip-fed", action="store_true", help="only the launches alone")
    ap.add_argument("--band", action="store_true", help="measure the band-mask stage instead of the echo")
    ap.add_argument("--reverb", action="store_true", help="measure the reverb stage instead of the echo")
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args()
    assert not (args.band and args.reverb), "--band or --reverb, not both"

    assert torch.cuda.is_available(), "bench_augment.py needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    import bench_feeder as bf
    from cleanumamba_amd import hip
    from cleanumamba_amd.training import augment as A
    hip.lib()
    B, L, S = args.batch, int(args.crop_seconds * bf.RATE), args.shift

    # ---- the launches alone
    def timed(fn, n=20, runs=1):
        fn()
        torch.cuda.synchronize()
        best = float("inf")
        for _ in range(runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                fn()
            b.record()
            torch.cuda.synchronize()
            best = min(best, a.elapsed_time(b) / n)
        return best
    g = torch.Generator(device=dev).manual_seed(0)
    C = 0.05 * torch.randn(B, L + S, device=dev, generator=g)
    Y = C + 0.05 * torch.randn(B, L + S, device=dev, generator=g)
    clean, noisy = torch.empty(B, 1, L, device=dev), torch.empty(B, 1, L, device=dev)
    work = A.workspace_for(B, L, dev)
    alone = {}
    if args.band:
        n, N, edges = L + S, hip.lib().cum_band_mask_block(), A.mel_edges()
        out_c, out_y = torch.empty(B, n, device=dev), torch.empty(B, n, device=dev)
        band_work = A.band_workspace_for(B, dev)
        for tag, lo, hi in (("band_0_23", 0, 23), ("band_60_80", 60, 80)):
            W = int(2.0 / float(edges[lo]))
            draws = full_draws(B, L, S, 0, False)
            draws = A.AugmentDraws(L, S, draws.perm, draws.off_clean, draws.off_noise, draws.snr_db, draws.gain, draws.kappa,
                                   draws.n_taps, draws.delay, draws.tap_gain, np.full(B, W), np.full(B, edges[lo]),
                                   np.full(B, edges[hi]))
            recs = torch.from_numpy(draws.pack_band()).to(dev)
            ms = timed(lambda: A.launch_band(C, n, Y, n, B, n, recs, band_work, out_c, n, out_y, n))
            moved = int(4 * B * n * 2 * (2 + 2 * W / (N - 2 * W)))
            alone[tag] = {"ms": round(ms, 4), "launches": 2, "W": W, "block": N, "valid_per_block": N - 2 * W, "bytes": moved,
                          "TB_per_s": round(moved / (ms * 1e-3) / 1e12, 3),
                          "frac_of_hbm_peak": round(moved / (ms * 1e-3) / HBM_PEAK, 3)}
            print(f"alone {tag}: {alone[tag]}", flush=True)
    def rooms(T, proba=1.0):
        """Four synthetic responses of exactly T taps: decaying Gaussian noise, the direct path first."""
        raw = []
        for i in range(4):
            h = np.random.default_rng(900 + i).standard_normal(T) * 10.0 ** (-3.0 * np.arange(T) / T)
            h[0] = 1.5 * max(1.0, np.abs(h).max())
            raw.append(h)
        rv = A.Reverb(raw, proba=proba, decay_db=400.0)          # (every tap stays)
        assert all(h.shape[0] == T for h in rv.taps)
        return rv
    if args.reverb:
        n, N = L + S, hip.lib().cum_reverb_block()
        out_c, out_y = torch.empty(B, n, device=dev), torch.empty(B, n, device=dev)
        rev_work = A.reverb_workspace_for(B, n, dev)
        for tag, T in (("taps_2048", 2048), ("taps_8192", 8192), ("taps_16384", 16384), ("copy", 0)):
            bank = rooms(T or 2048).bank(dev)
            ids = np.arange(B) % len(bank) if T else np.full(B, -1)
            recs = np.zeros((B, A.REVERB_INTS), dtype=np.int32)
            recs[:, 0] = ids
            recs = torch.from_numpy(recs.reshape(-1)).to(dev)
            ms = timed(lambda: A.launch_reverb(C, n, Y, n, B, n, recs, bank, rev_work, out_c, n, out_y, n), runs=3)
            K = -(-T // (N // 2))
            moved = int(4 * B * n * (10 + 8 * K)) if T else 16 * B * n
            alone[tag] = {"ms": round(ms, 4), "launches": 3, "taps": T, "block": N, "partitions": K, "bytes": moved,
                          "TB_per_s": round(moved / (ms * 1e-3) / 1e12, 3),
                          "frac_of_hbm_peak": round(moved / (ms * 1e-3) / HBM_PEAK, 3)}
            print(f"alone {tag}: {alone[tag]}", flush=True)
        alone["workspace_MB_per_block"] = round(4 * rev_work.numel() / 1e6, 1)
    for tag, taps, snr in (() if args.band or args.reverb else
                           (("echo_off_snr", 0, True), ("echo_off_keep", 0, False), ("echo_435_taps_snr", 435, True))):
        draws = full_draws(B, L, S, taps, snr)
        k = draws.columns()
        table = torch.from_numpy(draws.pack(k)).to(dev)
        ms = timed(lambda: A.launch(C, L + S, Y, L + S, B, L, L + S, table, k, work if snr else None, clean, L, noisy, L))
        alone[tag] = {"ms": round(ms, 4), "launches": 2 if snr else 1}
        if not taps:
            moved = 4 * B * L * (3 + 2 + (4 if snr else 0))
            alone[tag].update(bytes=moved, TB_per_s=round(moved / (ms * 1e-3) / 1e12, 3),
                              frac_of_hbm_peak=round(moved / (ms * 1e-3) / HBM_PEAK, 3))
        print(f"alone {tag}: {alone[tag]}", flush=True)
    result = {"tool": "tools/bench_augment.py", "batch": B, "length": L, "shift": S, "alone": alone}

    # ---- the fed step
    if not args.skip_fed:
        from cleanumamba_amd.network import Net
        from cleanumamba_amd.training.feeder import BatchFeeder
        from cleanumamba_amd.training.train_step import TrainStep
        from cleanumamba_amd.util.dataset import CleanNoisyPairDataset
        tmp = tempfile.TemporaryDirectory(prefix="augment_bench_")
        t0 = time.perf_counter()
        bf.write_tree(tmp.name, args.pairs, int(args.clip_seconds * bf.RATE))
        print(f"tree: {args.pairs} pairs x {args.clip_seconds:g} s written in {time.perf_counter() - t0:.1f} s", flush=True)
        ac = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": None}[args.dtype]
        torch.manual_seed(0)
        step = TrainStep(Net("CleanUMamba", bf.E8).to(dev).train(), autocast_dtype=ac)
        dataset = CleanNoisyPairDataset(root=tmp.name, subset="training", crop_length_sec=args.crop_seconds)
        base = dict(remix=True, shift=S, snr_db=(-5.0, 15.0), gain_db=(-6.0, 3.0))
        third = "M" if args.band else "W" if args.reverb else "R"
        configs = {"P": None, "Q": A.Augment(**base)}
        if args.reverb:
            room = rooms(8192)
            configs["V"] = A.Augment(reverb=room)
            configs["W"] = A.Augment(reverb=room, **base)
        else:
            configs[third] = A.Augment(band_mask=A.BandMask(), **base) if args.band else A.Augment(echo=A.Echo(), **base)
        feeders = {tag: BatchFeeder(dataset, B, dev, crop_length=L, seed=0, augment=cfg) for tag, cfg in configs.items()}

        def batches(feeder):
            while True:
                for batch in feeder:
                    yield batch
        streams = {tag: batches(f) for tag, f in feeders.items()}

        def run(tag, n):
            for _ in range(n):
                step(next(streams[tag]))
        settle = 0
        if ac == torch.float16:          # let the dynamic loss scale back off before anything is timed (as bench.py does)
            clean_run, skipped = 0, 0.0
            while clean_run < 2 and settle < 24:
                run("P", 1)
                settle += 1
                now = float(step.optimizer.state_vec[9])
                clean_run = clean_run + 1 if now == skipped else 0
                skipped = now
        for tag in feeders:
            run(tag, args.warmup)
        torch.cuda.synchronize()
        assert step.graph_status == "captured", step.graph_status
        windows = []
        for _ in range(args.rounds):
            for tag in configs:
                torch.cuda.synchronize()
                t = time.perf_counter()
                run(tag, args.steps)
                torch.cuda.synchronize()
                ms = 1e3 * (time.perf_counter() - t) / args.steps
                windows.append({"mode": tag, "ms_per_step": round(ms, 4)})
                print(f"{tag}: {ms:.3f} ms/step", flush=True)
        last = [next(streams[third]).draws for _ in range(4)]
        for f in feeders.values():
            f.close()
        tmp.cleanup()
        mean = {tag: sum(w["ms_per_step"] for w in windows if w["mode"] == tag) / args.rounds for tag in configs}
        p = [w["ms_per_step"] for w in windows if w["mode"] == "P"]
        result.update(workload=f"CleanUMamba-E8 train step, B={B}, {args.crop_seconds:g} s crops, {args.dtype}, one hipGraph",
                      steps_per_window=args.steps, warmup=args.warmup, settle_steps=settle, windows=windows,
                      P_to_P_spread_ms=round(max(p) - min(p), 4), mean_ms={k: round(v, 4) for k, v in mean.items()},
                      Q_minus_P_ms=round(mean["Q"] - mean["P"], 4), Q_minus_P_frac=round(mean["Q"] / mean["P"] - 1, 5))
        result.update({f"{third}_minus_P_ms": round(mean[third] - mean["P"], 4),
                       f"{third}_minus_P_frac": round(mean[third] / mean["P"] - 1, 5)})
        if args.reverb:
            result.update(W_minus_Q_ms=round(mean["W"] - mean["Q"], 4), V_minus_P_ms=round(mean["V"] - mean["P"], 4),
                          reverberant_rows_W=[int((d.rir >= 0).sum()) for d in last])
        elif args.band:
            result.update(M_minus_Q_ms=round(mean["M"] - mean["Q"], 4), band_half_M=[int(d.band_half[0]) for d in last])
        else:
            result.update(mean_taps_per_row_R=[int(d.n_taps.mean()) for d in last])
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
