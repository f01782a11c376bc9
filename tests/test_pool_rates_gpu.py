"""Rated pool slots on the GPU (network/streampool.py, csrc/resample.hip cum_resample_slots): the slotted conversion
kernel alone against ``cum_resample_ragged`` on history ++ chunk, and the pool against the hand-made chain -- a
``StreamResampler`` per rated slot and direction around an unrated pool -- bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_ckpt

pytestmark = pytest.mark.gpu

RATES = [8000, 22050, 32000, 44100, 48000]
PAIRS = [(r, 16000) for r in RATES] + [(16000, r) for r in RATES]
SENTINEL = -77.25


def _bits(t):
    return t.contiguous().view(torch.int32)


def _slot_cases():
    """One record per (pair, history count, chunk length, ended): a stream in a state ``stream_step`` reaches.
    History counts 0 and 1 are the first samples of a signal; K - 1 (= history_bound, the most a stream keeps) is a
    stream far into its signal -- every fourth of them beyond 2^33 samples.  Chunk lengths 0, 1, 2, K - 1, K, K + 1 and
    the shortest that give 767, 768 and 769 outputs (where one input makes several outputs, 16 k -> 48 k, the count asked
    for is capped at the target: the tile edge is what counts)."""
    from cleanumamba_amd.util.resample import final_outputs, history_bound, plan, stream_step
    cases = []
    for pid, pair in enumerate(PAIRS):
        p = plan(*pair)
        up, down, H, K = p.up, p.down, p.H, p.K
        assert history_bound(K) == K - 1
        for n_hist in (0, 1, K - 1):
            far = (1 << 33) + 12345 if len(cases) % 4 == 0 else 5000 + 7 * pid
            received = n_hist if n_hist < 2 else far
            emitted = final_outputs(received, up, down, H)
            base = received - n_hist
            assert base == 0 or (emitted * down + H) // up - (K - 1) >= base
            for ends in (False, True):
                lens = [(0, None), (1, None), (2, None), (K - 1, None), (K, None), (K + 1, None)]
                for target in (767, 768, 769):
                    n = 0
                    while stream_step(received, emitted, base, n, up, down, H, K, ends)[0] < target:
                        n += 1
                    lens.append((n, target))
                for n_new, target in lens:
                    count, start = stream_step(received, emitted, base, n_new, up, down, H, K, ends)
                    assert target is None or count == target or (up > down and count < target + up)
                    cases.append(dict(pid=pid, p=p, n_hist=n_hist, n_new=n_new, ends=ends, in0=base, out0=emitted,
                                      n_out=count if target is None else target, keep=received + n_new - start))
    return cases


def test_slots_kernel_against_resample_ragged(cuda):
    from cleanumamba_amd import hip
    from cleanumamba_amd.util import resample as rs
    cases = _slot_cases()
    n = len(cases)
    plans = [c["p"] for c in cases[::len(cases) // len(PAIRS)]]
    assert len(plans) == len(PAIRS) and [p for p in plans] == [rs.plan(*pair) for pair in PAIRS]
    pitch = -(-max(p.K - 1 for p in plans) // 4) * 4
    g = torch.Generator().manual_seed(5)
    lmax = max(c["n_new"] for c in cases)
    wmax = max(c["n_out"] for c in cases)
    nan = float("nan")
    # host images: NaN behind every chunk's length and every history's count, a sentinel behind every output row's count,
    # in the history row a record writes and in a guard row behind the last slot
    x = torch.full((n, lmax + 5), nan)
    hist = torch.full((n + 1, 2, pitch), SENTINEL)
    y = torch.full((n, wmax + 9), SENTINEL)
    rec = np.zeros((n, 16), dtype=np.int32)
    signals = []
    for i, c in enumerate(cases):
        sig = torch.randn(c["n_hist"] + c["n_new"], generator=g)
        signals.append(sig)
        parity = i % 2
        hist[i, parity] = nan
        hist[i, parity, :c["n_hist"]] = sig[:c["n_hist"]]
        x[i, :c["n_new"]] = sig[c["n_hist"]:]
        slot = (i * 7) % n                                  # 7 and n are coprime: every slot once, not in table order
        c["slot"], c["parity"] = slot, parity
        rec[i, :11] = [slot, c["pid"], c["n_hist"], i, c["n_new"], c["n_out"], i, c["ends"], c["keep"], parity, 3]
        rec[i].view(np.int64)[6:] = [c["in0"], c["out0"]]
    assert n % 7 != 0
    by_slot = torch.full((n + 1, 2, pitch), SENTINEL)
    for i, c in enumerate(cases):
        by_slot[c["slot"]] = hist[i]
    ints = np.zeros((len(plans), 8), dtype=np.int32)
    off = 0
    for k, p in enumerate(plans):
        ints[k, :6] = (p.up, p.down, len(p.taps), p.K, p.pitch, off)
        off += p.up * p.pitch
    tables = torch.cat([p.host_table().reshape(-1) for p in plans]).to(cuda)
    d_x, d_plans, d_rec = x.to(cuda), torch.from_numpy(ints).to(cuda), torch.from_numpy(rec).to(cuda)
    lib = hip.lib()

    def run():
        d_hist, d_y = by_slot.to(cuda), y.to(cuda)
        with torch.cuda.device(cuda):
            hip.check(lib.cum_resample_slots(
                hip.ptr(d_hist), pitch, n, ctypes.c_void_p(ints.ctypes.data), hip.ptr(d_plans), len(plans),
                hip.ptr(tables), tables.numel(), ctypes.c_void_p(rec.ctypes.data), hip.ptr(d_rec), n, hip.ptr(d_x), n,
                d_x.stride(0), hip.ptr(d_y), n, d_y.stride(0), hip.stream_ptr()))
        torch.cuda.synchronize()
        return d_hist.cpu(), d_y.cpu()

    got_hist, got_y = run()
    # the reference: cum_resample_ragged on history ++ chunk, one launch per pair and state
    want = [None] * n
    for pid, p in enumerate(plans):
        for ends in (False, True):
            idx = [i for i, c in enumerate(cases) if c["pid"] == pid and c["ends"] == ends]
            rows = torch.nn.utils.rnn.pad_sequence([signals[i] for i in idx], batch_first=True, padding_value=nan)
            rows = torch.cat([rows, torch.full((len(idx), 4), nan)], 1).to(cuda)
            lens = torch.tensor([signals[i].numel() for i in idx], dtype=torch.int32).to(cuda)
            origin = torch.tensor([[cases[i]["in0"], cases[i]["out0"]] for i in idx], dtype=torch.int64).to(cuda)
            ref = torch.full((len(idx), wmax + 8), SENTINEL, device=cuda)
            rs._launch(p, rows, lens, origin, ends, ref, wmax + 4)
            ref = ref.cpu()
            for j, i in enumerate(idx):
                want[i] = ref[j]
    for i, c in enumerate(cases):
        tag = (PAIRS[c["pid"]], c["n_hist"], c["n_new"], c["ends"], c["n_out"])
        m = c["n_out"]
        assert not torch.isnan(want[i][:m]).any() and (want[i][:m] != SENTINEL).all(), tag
        assert torch.equal(got_y[i, 3:3 + m], want[i][:m]), tag
        assert (got_y[i, :3] == SENTINEL).all() and (got_y[i, 3 + m:] == SENTINEL).all(), tag
        rows = got_hist[c["slot"]]
        sig, keep = signals[i], c["keep"]
        assert torch.equal(rows[1 - c["parity"], :keep], sig[sig.numel() - keep:]), tag
        assert (rows[1 - c["parity"], keep:] == SENTINEL).all(), tag
        assert torch.equal(_bits(rows[c["parity"]]), _bits(by_slot[c["slot"], c["parity"]])), tag      # the row read
    assert (got_hist[n] == SENTINEL).all()
    again_hist, again_y = run()
    assert torch.equal(_bits(again_y), _bits(got_y)) and torch.equal(_bits(again_hist), _bits(got_hist))


# ------------------------------------------------------------------------------------------- the pool against the chain
def _net(name, cuda):
    from cleanumamba_amd.network import CleanUMamba
    sd, cfg = load_ckpt(name)
    net = CleanUMamba(**cfg)
    (net.load_state_dict if name == "442k" else net.load_pruned_state_dict)(sd)
    return net.to(cuda).float().eval()


class Chain:
    """The definition: a StreamResampler(1, rate, 16000) per rated slot, its pushes fed into an unrated pool with the
    same slot sets per call, that pool's outputs pushed into a StreamResampler(1, 16000, rate); at the end finish(), a
    last feed, close, finish(), and the crop to the samples the slot was fed."""

    def __init__(self, net, capacity, dev):
        self.pool, self.dev = net.stream_pool(capacity), dev
        self.rin, self.rout, self.fed, self.given = {}, {}, {}, {}

    def open(self, n=1, rate=None):
        from cleanumamba_amd.util.resample import StreamResampler
        slots = self.pool.open(n)
        for s in slots:
            if rate not in (None, 16000):
                self.rin[s] = StreamResampler(1, rate, 16000, self.dev)
                self.rout[s] = StreamResampler(1, 16000, rate, self.dev)
                self.fed[s] = self.given[s] = 0
        return slots

    def feed(self, slots, chunks):
        mid = [self.rin[s].push(c[None])[0] if s in self.rin else c for s, c in zip(slots, chunks)]
        outs = [self.rout[s].push(y[None])[0] if s in self.rout else y for s, y in zip(slots, self.pool.feed(slots, mid))]
        for s, c, y in zip(slots, chunks, outs):
            if s in self.rin:
                self.fed[s] += c.numel()
                self.given[s] += y.numel()
        return outs

    def close(self, slots):
        none = torch.zeros(0, device=self.dev)
        heads = self.pool.feed(slots, [self.rin[s].finish()[0] if s in self.rin else none for s in slots])
        tails = self.pool.close(slots)
        outs = []
        for s, h, t in zip(slots, heads, tails):
            if s not in self.rin:
                outs.append(t)
                continue
            r = self.rout.pop(s)
            y = torch.cat([r.push(h[None])[0], r.push(t[None])[0], r.finish()[0]])
            outs.append(y[:self.fed[s] - self.given[s]])
            del self.rin[s]
        return outs


def _script(dev):
    """The calls of one run: ('open', key, rate), ('feed', [keys], [chunks]), ('close', [keys]).  Six streams at 8000,
    16000 (explicit), None, 32000, 44100 and 48000 join in different calls; ragged list-form chunks with an empty one, a
    1-sample one and one shorter than the delay; calls that name part of the live streams; closes at different times; the
    first id that closes is opened again at 22050."""
    rng = np.random.default_rng(21)
    g = torch.Generator().manual_seed(3)
    rates = {"a": 8000, "b": 16000, "c": None, "d": 32000, "e": 44100, "f": 48000, "g": 22050}
    joins = {0: ["a", "b"], 2: ["c", "d"], 3: ["e", "f"], 12: ["g"]}
    leaves = {10: ["a"], 15: ["c", "e"], 17: ["b", "f", "g"], 19: ["d"]}
    special = {(4, "f"): 0, (5, "f"): 1, (6, "f"): 50, (4, "a"): 1, (7, "e"): 0, (13, "g"): 30, (5, "c"): 0}
    calls, live = [], []
    for call in range(20):
        for k in leaves.get(call, []):
            live.remove(k)
        if call in leaves:
            calls.append(("close", list(leaves[call])))
        for k in joins.get(call, []):
            calls.append(("open", k, rates[k]))
            live.append(k)
        named = [k for k in live if call % 4 != 1 or rng.random() < 0.6 or (call, k) in special]
        if named:
            chunks = []
            for k in named:
                ms = float(rng.uniform(8, 45))
                m = special.get((call, k), int((rates[k] or 16000) * ms / 1000))
                chunks.append((0.1 * torch.randn(m, generator=g)).to(dev))
            calls.append(("feed", named, chunks))
    assert not live
    return calls


def _drive(pool, calls, count=None):
    slot, outs, fed = {}, {}, {}
    for c in calls:
        before = len(count) if count is not None else 0
        if c[0] == "open":
            slot[c[1]] = pool.open(1, rate=c[2])[0]
            outs[c[1]], fed[c[1]] = [], 0
        elif c[0] == "feed":
            for k, x, y in zip(c[1], c[2], pool.feed([slot[k] for k in c[1]], c[2])):
                outs[k].append(y)
                fed[k] += x.numel()
        else:
            for k, y in zip(c[1], pool.close([slot[k] for k in c[1]])):
                outs[k].append(y)
        if count is not None:
            c_calls = count[before:]
            rated = c[0] != "open" and any(pool_rate not in (None, 16000) for pool_rate in [RATE_OF[k] for k in c[1]])
            if not rated:
                assert c_calls == [], c[:2]               # a call of unrated slots never enters the conversion
            else:
                assert len(c_calls) <= 2 and len(set(c_calls)) == len(c_calls), c[:2]    # at most one per direction
    return {k: torch.cat(v) for k, v in outs.items()}, fed


RATE_OF = {"a": 8000, "b": 16000, "c": None, "d": 32000, "e": 44100, "f": 48000, "g": 22050}


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("name", ["pruned500k", "442k"])
def test_pool_is_the_chain_bit_for_bit(cuda, name, normalize, monkeypatch):
    from cleanumamba_amd import hip
    net = _net(name, cuda)
    net.normalize_input = normalize
    calls = _script(cuda)
    with torch.no_grad():
        want, fed = _drive(Chain(net, 6, cuda), calls)
        pool = net.stream_pool(6)
        lib, real, seen = hip.lib(), hip.lib().cum_resample_slots, []

        def counted(*args):
            seen.append(int(args[0].value != pool.rs_hist[0].data_ptr()))     # the history block: 0 in, 1 out
            return real(*args)
        monkeypatch.setattr(lib, "cum_resample_slots", counted, raising=False)
        got, fed2 = _drive(pool, calls, seen)
        monkeypatch.undo()
    assert len(seen) > 10 and set(seen) == {0, 1}
    assert set(got) == set(want) == set(RATE_OF) and fed == fed2
    for k in sorted(got):
        assert got[k].numel() == want[k].numel() == fed[k] > 0, (k, got[k].numel(), want[k].numel(), fed[k])
        assert torch.equal(got[k], want[k]), k
        assert float(got[k].abs().max()) > 0 and bool(torch.isfinite(got[k]).all())
    assert pool.live == [] and float(pool.state.abs().max()) == 0 and float(pool.hist.abs().max()) == 0
    assert float(pool.rs_hist.abs().max()) == 0
    assert not pool._rate.any() and not pool._rs_pos.any() and not pool._rs_par.any() and not pool._rs_parity.any()
    assert not pool._fed.any() and not pool._given.any()


def test_idle_rated_slots_leave_an_unrated_run_alone(cuda):
    """Unrated slots fed in a pool that also holds idle rated slots: bit-identical to the same run in a fresh pool."""
    net = _net("pruned500k", cuda)
    hop = net.total_stride
    g = torch.Generator().manual_seed(9)
    x = (0.1 * torch.randn(3, 9 * hop + 77, generator=g)).to(cuda)
    cuts = [0, 300, 301, 4 * hop + 5, 9 * hop + 77]
    outs = []
    with torch.no_grad():
        for idle in (False, True):
            pool = net.stream_pool(8)
            if idle:
                busy = pool.open(1, rate=48000) + pool.open(1, rate=44100)
                pool.feed(busy, [x[0, :700], x[1, :650]])  # (they hold conversion state)
            s = pool.open(3)
            ys = [pool.feed(s, x[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])] + [pool.close(s)]
            outs.append(torch.stack([torch.cat([y[i] for y in ys]) for i in range(3)]))
            if idle:
                assert pool.live == busy and pool.rate(busy) == [48000, 44100]
    assert outs[0].shape == x.shape and torch.equal(outs[0], outs[1])
