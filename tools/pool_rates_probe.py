"""pool_rates_probe.py -- what does it cost to run pool slots at their own sample rate?

  python tools/pool_rates_probe.py [--slots 256] [--ms 20] [--calls 25] [--rounds 7] [--only a] [--out FILE]

The pruned 492K model of the bench's streaming row (tests/golden/ckpt_pruned500k.npz), ``--slots`` pool slots, every call
feeds each slot ``--ms`` of audio at the slot's rate.  Timed per call:

  a  all slots at the model's rate (16 kHz): today's pool, no conversion;
  b  all slots at 48 kHz;
  c  a quarter of the slots each at 8, 16, 44.1 and 48 kHz;
  d  the hand-made chain of c: two ``StreamResampler`` objects per rated slot around an unrated pool.

After ``--warmup`` calls (every slot past its first frame), ``--rounds`` rounds; a round times ``--calls`` calls of each
variant between two device events, the variants in an order that rotates from round to round.  Printed per variant: the
median over the rounds of the time of one call, the lowest and highest round (the spread), the host's share (wall time
with no wait on the device), and the real-time factor the median implies (slots x ms / time of a call).  ``--only a``
restricts the run to the variants named, which is how a commit that has no rated slots is measured with the same code.

Every line printed goes to ``--out`` as well.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODEL_RATE = 16000
MIX = [8000, None, 44100, 48000]


class Chain:
    """Variant d: what a caller had to write before slots had rates."""

    def __init__(self, pool, slots, rates, dev):
        from cleanumamba_amd.util.resample import StreamResampler
        self.pool, self.slots = pool, slots
        self.rin = [StreamResampler(1, r, MODEL_RATE, dev) if r else None for r in rates]
        self.rout = [StreamResampler(1, MODEL_RATE, r, dev) if r else None for r in rates]

    def feed(self, chunks):
        mid = [r.push(c[None])[0] if r else c for r, c in zip(self.rin, chunks)]
        return [r.push(y[None])[0] if r else y for r, y in zip(self.rout, self.pool.feed(self.slots, mid))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--ms", type=float, default=20.0)
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--only", default="abcd")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pool_rates_probe.py needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from cleanumamba_amd.network import CleanUMamba
    import json
    with np.load(os.path.join(ROOT, "tests", "golden", "ckpt_pruned500k.npz")) as f:
        cfg = json.loads(bytes(f["__network_config__"]).decode())
        sd = {k: torch.from_numpy(f[k].astype(np.float32)) for k in f.files if k != "__network_config__"}
    net = CleanUMamba(**cfg)
    net.load_pruned_state_dict(sd)
    net = net.to(dev).float().eval()
    S = args.slots
    g = torch.Generator().manual_seed(1)

    def variant(kind):
        """-> a function that makes one call."""
        pool = net.stream_pool(S)
        rates = {"a": [None] * S, "b": [48000] * S, "c": [MIX[i % 4] for i in range(S)], "d": [MIX[i % 4] for i in range(S)]}[kind]
        size = [int((r or MODEL_RATE) * args.ms / 1000) for r in rates]
        if kind == "d":
            chain = Chain(pool, pool.open(S), rates, dev)
            chunks = [(0.1 * torch.randn(n, generator=g)).to(dev) for n in size]
            return lambda: chain.feed(chunks)
        if kind == "a":
            slots = pool.open(S)
        else:
            slots = [pool.open(1, rate=r)[0] for r in rates]
        if len(set(size)) == 1:
            x = (0.1 * torch.randn(S, size[0], generator=g)).to(dev)
        else:
            x = [(0.1 * torch.randn(n, generator=g)).to(dev) for n in size]
        return lambda: pool.feed(slots, x)

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    kinds = [k for k in "abcd" if k in args.only]
    dev_ms, host_ms = {k: [] for k in kinds}, {k: [] for k in kinds}
    with torch.no_grad():
        call = {k: variant(k) for k in kinds}
        for k in kinds:
            for _ in range(args.warmup):
                call[k]()
        torch.cuda.synchronize()
        for r in range(args.rounds):
            for k in kinds[r % len(kinds):] + kinds[:r % len(kinds)]:
                n = max(args.calls // 5, 2) if k == "d" else args.calls
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                for _ in range(n):
                    call[k]()
                e1.record()
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                dev_ms[k].append(e0.elapsed_time(e1) / n)
                host_ms[k].append((t1 - t0) * 1e3 / n)
    say(f"pool_rates_probe: {torch.cuda.get_device_name(0)}, pruned 492K model, {S} slots, {args.ms:g} ms per slot and call, "
        f"{args.rounds} rounds of {args.calls} calls (d: {max(args.calls // 5, 2)})")
    names = {"a": "a  all slots at 16 kHz (no conversion)", "b": "b  all slots at 48 kHz",
             "c": "c  8 / 16 / 44.1 / 48 kHz, a quarter each", "d": "d  the hand-made chain of c"}
    med = {}
    for k in kinds:
        v = np.asarray(dev_ms[k])
        med[k] = float(np.median(v))
        say(f"  {names[k]:44s} {med[k]:8.3f} ms / call  (rounds {v.min():.3f} .. {v.max():.3f}; host {np.median(host_ms[k]):.3f} ms)"
            f"  {S * args.ms / med[k]:9.0f} x real time")
    if "a" in med:
        for k in kinds:
            if k != "a":
                say(f"  {k} over a: {med[k] - med['a']:+.3f} ms / call ({med[k] / med['a']:.2f} x)")
    if "c" in med and "d" in med:
        say(f"  c against d: {med['d'] / med['c']:.1f} x faster")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
