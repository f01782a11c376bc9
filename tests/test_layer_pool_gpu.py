"""The stream pool's "layers" backend on the GPU (network/streampool.py, network/layerpool.py, csrc/slotstate.hip): the
slot-row mover alone, bit for bit; the pool in lock-step against feed_batch / flush_batch on the per-layer hop, bit for
bit; slots that join, feed ragged chunks and leave on their own against forward and a lone feed / flush; the two backends
against each other; rated slots against the hand-made chain of two StreamResamplers around a lone stream."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_ckpt, record, rel_l2

pytestmark = pytest.mark.gpu

BIG = dict(channels_input=1, channels_output=1, channels_H=64, max_H=256, encoder_n_layers=8, kernel_size=4, stride=2,
           tsfm_d_model=256, tsfm_d_inner=1024, tsfm_n_head=8, tsfm_n_layers=3)
POISON = -77.25
_NETS = {}


def _net(name, cuda):
    """The fixtures and BIG (seeded random weights, really above hopplan.MAX_PARAMS), made once."""
    from cleanumamba_amd.network import CleanUMamba, hopplan
    if name not in _NETS:
        if name == "BIG":
            torch.manual_seed(1234)
            net = CleanUMamba(**BIG)
            assert sum(p.numel() for p in net.parameters()) > hopplan.MAX_PARAMS
            assert hopplan.unsupported_reason(net) == "weights too large to be re-read per stream"
        else:
            sd, cfg = load_ckpt(name)
            net = CleanUMamba(**cfg)
            (net.load_state_dict if name == "442k" else net.load_pruned_state_dict)(sd)
        _NETS[name] = net.to(cuda).float().eval()
    return _NETS[name]


# ------------------------------------------------------------------------------------------------- the mover alone
SEG_BYTES = [4, 12, 16, 20, 4092, 16388]
# dense side per segment: (bytes in front of stream 0 -- the "row 0" of a row buffer --, per-stream pitch, slack bytes
# behind the last stream, whether the buffer is a row buffer whose framing a gather clears).  Pitches 4, 12, 20 and
# 16392 leave every stream but the first off the 16-byte grid (dword path); 32 and 4096 keep the vector path, the
# 4092-byte segment with a short last piece.
DENSE = [(0, 4, 0, False), (0, 12, 0, False), (0, 32, 0, False), (0, 20, 0, False), (32, 4096, 96, True),
         (8, 16392, 40, True)]


@pytest.mark.parametrize("slots", [[3], [6, 0, 2], [0, 1, 2, 3, 4, 5, 6]])
def test_mover_gathers_and_scatters_exactly_the_named_rows(cuda, slots):
    from cleanumamba_amd import hip
    cap, n = 7, len(slots)
    offs, end = [], 24 * 4                                   # 96 bytes in front of the first segment belong to none
    for b in SEG_BYTES:
        offs.append(end)
        end = -(-(end + b) // 16) * 16 + 16                  # a 16-byte gap behind every segment
    stride = end // 4 + 4
    g = torch.Generator().manual_seed(17)
    store = torch.randn(cap, stride, generator=g).to(cuda)
    # each dense buffer holds `cap` streams; poisoned, with a guard of 64 floats at the end
    dense, recs, clears = [], [], []
    for (head, pitch, slack, is_rows), off, b in zip(DENSE, offs, SEG_BYTES):
        t = torch.full(((head + cap * pitch + slack) // 4 + 64,), POISON, device=cuda)
        dense.append(t)
        recs.append((t.data_ptr() + head, pitch, off, b))
        if is_rows:
            clears.append((t.data_ptr(), head, head + n * pitch, slack))
    before = [t.clone() for t in dense]
    h_slots = np.asarray(slots, dtype=np.int32)
    h_recs, h_clears = np.asarray(recs, dtype=np.int64), np.asarray(clears, dtype=np.int64)
    d_slots, d_recs, d_clears = (torch.from_numpy(x).to(cuda) for x in (h_slots, h_recs, h_clears))

    def move(direction, st):
        with torch.cuda.device(cuda):
            hip.check(hip.lib().cum_stream_slots_move(
                direction, hip.ptr(st), st.stride(0), cap, ctypes.c_void_p(h_slots.ctypes.data), hip.ptr(d_slots), n,
                ctypes.c_void_p(h_recs.ctypes.data), hip.ptr(d_recs), len(recs), ctypes.c_void_p(h_clears.ctypes.data),
                hip.ptr(d_clears), len(clears), hip.stream_ptr()))
        torch.cuda.synchronize()

    move(0, store)
    src = store.cpu().view(torch.int32)
    for (head, pitch, slack, is_rows), off, b, t, t0 in zip(DENSE, offs, SEG_BYTES, dense, before):
        want = t0.cpu().view(torch.int32).clone()
        for j, s in enumerate(slots):                       # stream j of the batch is slot slots[j]
            at = (head + j * pitch) // 4
            want[at:at + b // 4] = src[s, off // 4:(off + b) // 4]
        if is_rows:                                          # the framing of a batch of n: in front, and behind stream n - 1
            want[:head // 4] = 0
            want[(head + n * pitch) // 4:(head + n * pitch + slack) // 4] = 0
        assert torch.equal(t.cpu().view(torch.int32), want), (b, pitch)
    # ... and back, into a poisoned store: the named rows' segments, nothing else
    store2 = torch.full_like(store, POISON)
    move(1, store2)
    want = torch.full_like(store, POISON).cpu().view(torch.int32)
    for s in slots:
        for off, b in zip(offs, SEG_BYTES):
            want[s, off // 4:(off + b) // 4] = src[s, off // 4:(off + b) // 4]
    assert torch.equal(store2.cpu().view(torch.int32), want)
    assert torch.equal(store.cpu().view(torch.int32), src)              # (a gather leaves the store as it was)
    # a gather that names no slot only clears: the framing of a batch that shrank to n streams, its streams left in place
    for t in dense:
        t.fill_(POISON)
    with torch.cuda.device(cuda):
        hip.check(hip.lib().cum_stream_slots_move(
            0, hip.ptr(store), store.stride(0), cap, None, None, 0, ctypes.c_void_p(h_recs.ctypes.data), hip.ptr(d_recs),
            len(recs), ctypes.c_void_p(h_clears.ctypes.data), hip.ptr(d_clears), len(clears), hip.stream_ptr()))
    torch.cuda.synchronize()
    for (head, pitch, slack, is_rows), t in zip(DENSE, dense):
        want = torch.full_like(t, POISON).cpu()
        if is_rows:
            want[:head // 4] = 0
            want[(head + n * pitch) // 4:(head + n * pitch + slack) // 4] = 0
        assert torch.equal(t.cpu(), want)
    assert torch.equal(store.cpu().view(torch.int32), src)


# ------------------------------------------------------------------------------------------------- lock-step
@pytest.mark.parametrize("name", ["pruned500k", "442k", "BIG"])
def test_layers_pool_in_lock_step_is_bit_identical_to_feed_batch(cuda, name):
    """Five slots open together and get the same chunks: the pool's output, close included, is bit for bit what feed_batch
    + flush_batch give on the per-layer hop -- the same kernels at the same batch size, and the mover copies bits."""
    net = _net(name, cuda)
    net.normalize_input = False
    hop, F, S = net.total_stride, net.frame_length, 5
    sizes = [F - 40, 57, hop, 16 * hop + 3, 1, 5 * hop - 9, 2 * hop]
    x = (0.1 * torch.randn(S, sum(sizes), generator=torch.Generator().manual_seed(7))).to(cuda)
    x[2] *= 6.0
    net.use_hop_kernel = False                  # the reference on the per-layer hop too (BIG is there anyway)
    try:
        with torch.no_grad():
            net.reset_stream()
            ref, i = [], 0
            for n in sizes:
                ref.append(net.feed_batch(x[:, i:i + n]))
                i += n
            assert net.hop_kernel_status == "off"
            ref.append(net.flush_batch())
            ref = torch.cat(ref, 1)
    finally:
        del net.use_hop_kernel
    pool = net.stream_pool(8, backend=None if name == "BIG" else "layers")
    assert pool.backend == "layers"
    slots = pool.open(S)
    got, i = [[] for _ in range(S)], 0
    for n in sizes:
        for s, y in enumerate(pool.feed(slots, x[:, i:i + n])):
            assert y.dim() == 1 and y.numel() % hop == 0
            got[s].append(y)
        i += n
    assert float(pool.state.abs().max()) > 0
    for s, y in enumerate(pool.close(slots)):
        got[s].append(y)
    got = torch.stack([torch.cat(g) for g in got])
    assert got.shape == ref.shape == x.shape and float(ref.abs().max()) > 0
    assert torch.equal(got, ref)
    assert pool.live == [] and float(pool.state.abs().max()) == 0 and float(pool.hist.abs().max()) == 0


def test_layers_pool_weight_change_under_live_slots(cuda):
    """An in-place weight change while slots are live: the pool has no blob of its own, the fused hop re-packs through
    the model's pack plan, the slots keep their state -- bit for bit feed_batch on the per-layer hop through the same
    change (running std off: the pool multiplies by 1 / f where first_frame divides by f)."""
    net = _net("pruned500k", cuda)
    net.normalize_input = False
    hop, S = net.total_stride, 3
    x = (0.1 * torch.randn(S, 12 * hop, generator=torch.Generator().manual_seed(9))).to(cuda)
    w0 = net.decoder[3][0].weight.detach().clone()
    cuts = [(0, 5 * hop), (5 * hop, 8 * hop + 5), (8 * hop + 5, 12 * hop)]
    net.use_hop_kernel = False
    try:
        with torch.no_grad():
            net.reset_stream()
            pool = net.stream_pool(4, backend="layers")
            slots = pool.open(S)
            ref, got = [], [[] for _ in range(S)]
            for c, (i, j) in enumerate(cuts):
                if c == 1:
                    net.decoder[3][0].weight.mul_(1.5)          # in place: bumps the parameter's version counter
                ref.append(net.feed_batch(x[:, i:j]))
                for s, y in enumerate(pool.feed(slots, x[:, i:j])):
                    got[s].append(y)
            ref.append(net.flush_batch())
            for s, y in enumerate(pool.close(slots)):
                got[s].append(y)
    finally:
        del net.use_hop_kernel
        with torch.no_grad():
            net.decoder[3][0].weight.copy_(w0)
    ref = torch.cat(ref, 1)
    got = torch.stack([torch.cat(g) for g in got])
    assert got.shape == ref.shape and float(ref.abs().max()) > 0
    assert torch.equal(got, ref)


# ------------------------------------------------------------------------------------------------- staggered joins
def _staggered_run(net, signals, joins, capacity, rng_seed, backend):
    """Drive a pool through a churn schedule: stream k joins at call joins[k] and feeds its signal in ragged chunks
    (the list form of feed: a different length per slot); in some calls only part of the live slots is named; a stream
    closes in the call after its last sample.  Returns each stream's output, the largest number of slots that ran a hop
    in one call and whether a slot id was used twice."""
    rng = np.random.default_rng(rng_seed)
    hop = net.total_stride
    pool = net.stream_pool(capacity, backend=backend)
    slot_of, pos, outs, finished = {}, {}, {k: [] for k in range(len(signals))}, set()
    most, call, used, reused = 0, 0, set(), False
    while len(finished) < len(signals):
        for k in [k for k, c in enumerate(joins) if c == call]:
            slot_of[k], pos[k] = pool.open()[0], 0
            reused |= slot_of[k] in used
            used.add(slot_of[k])
        live = [k for k in slot_of if k not in finished]
        done = [k for k in live if pos[k] >= signals[k].numel()]
        if done:
            for k, y in zip(done, pool.close([slot_of[k] for k in done])):
                outs[k].append(y)
                finished.add(k)
        live = [k for k in live if k not in done]
        named = live if call % 4 != 2 else [k for k in live if rng.random() < 0.6]
        if named:
            chunks = []
            for k in named:
                # a running stream gets 1 - 3 hops' worth (so it runs a hop), a joining one an odd count (off the grid)
                n = int(rng.integers(hop, 3 * hop)) if pos[k] else int(rng.integers(hop // 2, 3 * hop)) | 1
                chunks.append(signals[k][pos[k]:pos[k] + n])
                pos[k] += chunks[-1].numel()
            ys = pool.feed([slot_of[k] for k in named], chunks)
            most = max(most, sum(1 for y in ys if y.numel() > 0))
            for k, y in zip(named, ys):
                outs[k].append(y)
        call += 1
        assert call < 10_000
    assert pool.live == [] and float(pool.state.abs().max()) == 0
    return [torch.cat(outs[k]) for k in range(len(signals))], most, reused


JOINS = [0] * 9 + [3] * 6 + [9] * 5


def _signals(net, cuda):
    """20 streams of 2 - 12 hops plus an offset off the hop grid, one of 3 samples."""
    hop = net.total_stride
    g = torch.Generator().manual_seed(11)
    rng = np.random.default_rng(5)
    lengths = [int(rng.integers(2, 13)) * hop + int(rng.integers(1, hop)) for _ in JOINS]
    lengths[5] = 3                                       # a stream that never reaches a frame
    return [(0.1 * float(1 + k % 5) * torch.randn(n, generator=g)).to(cuda) for k, n in enumerate(lengths)]


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("name", ["pruned500k", "BIG"])
def test_layers_pool_staggered_joins_ragged_chunks_and_reuse(cuda, name, normalize):
    """Streams join in calls 0, 3 and 9 (the last into the ids of streams that have left), at sample offsets off the hop
    grid, with ragged chunks, leaving at different times, so that the rounds of a call run cohorts of different sizes.
    Each stream's output: normalisation off, the parallel forward of its own signal (1e-4, the project's bound for a
    stream against forward); on, a lone feed / flush of it (5e-5, the bound of the same comparison on the kernel pool)."""
    net = _net(name, cuda)
    net.normalize_input = normalize
    signals = _signals(net, cuda)
    with torch.no_grad():
        outs, most, reused = _staggered_run(net, signals, JOINS, 14, 1, "layers")
    assert most > 4 and reused
    worst = 0.0
    with torch.no_grad():
        for k, sig in enumerate(signals):
            if not normalize:
                want = net(sig.view(1, 1, -1))[0, 0, :sig.numel()]
            else:
                net.reset_stream()
                want = torch.cat([net.feed(sig.view(1, -1)), net.flush()], 1)[0]
            assert outs[k].shape == want.shape == sig.shape
            if k != 5:
                assert float(want.abs().max()) > 0
            worst = max(worst, rel_l2(outs[k], want))
    record(f"layers_pool_staggered{'_norm' if normalize else ''}[{name}]", worst)
    print(f"layers pool staggered {name} normalize={normalize}: worst rel_l2 {worst:.3e}")
    assert worst < (5e-5 if normalize else 1e-4)


def test_both_backends_agree(cuda):
    """The same staggered schedule through a "kernel" pool and a "layers" pool of one model."""
    net = _net("pruned500k", cuda)
    net.normalize_input = False
    signals = _signals(net, cuda)
    with torch.no_grad():
        a, _, _ = _staggered_run(net, signals, JOINS, 14, 1, "kernel")
        b, _, _ = _staggered_run(net, signals, JOINS, 14, 1, "layers")
    worst = 0.0
    for k, (ya, yb) in enumerate(zip(a, b)):
        assert ya.shape == yb.shape == signals[k].shape
        if k != 5:
            assert float(ya.abs().max()) > 0 and float(yb.abs().max()) > 0
        worst = max(worst, rel_l2(yb, ya))
    record("layers_pool_against_kernel_pool[pruned500k]", worst)
    print(f"layers pool against kernel pool: worst rel_l2 {worst:.3e}")
    assert worst < 1e-4


def test_layers_pool_is_reproducible(cuda):
    """The same schedule twice on two fresh pools: equal bits (running std included)."""
    net = _net("pruned500k", cuda)
    net.normalize_input = True
    signals = _signals(net, cuda)
    with torch.no_grad():
        a, _, _ = _staggered_run(net, signals, JOINS, 14, 1, "layers")
        b, _, _ = _staggered_run(net, signals, JOINS, 14, 1, "layers")
    assert all(torch.equal(ya, yb) for ya, yb in zip(a, b)) and float(a[0].abs().max()) > 0


# ------------------------------------------------------------------------------------------------- rated slots
def test_rated_slots_on_a_large_model(cuda):
    """One BIG pool with a slot at 8 000, one at 48 000 and one at the model's rate, fed ragged chunks in the same calls and
    closed: each returns exactly as many samples as it was fed and agrees with two StreamResamplers around a lone feed /
    flush of the same model."""
    from cleanumamba_amd.util.resample import StreamResampler
    net = _net("BIG", cuda)
    net.normalize_input = True
    rates = [8000, 48000, 16000]
    g = torch.Generator().manual_seed(23)
    rng = np.random.default_rng(9)
    calls = [[(0.1 * torch.randn(int(r * rng.uniform(0.02, 0.06)), generator=g)).to(cuda) for r in rates]
             for _ in range(6)]
    with torch.no_grad():
        pool = net.stream_pool(4)
        assert pool.backend == "layers"
        slots = [pool.open(1, rate=r)[0] for r in rates]
        got = [[] for _ in rates]
        for chunks in calls:
            for i, y in enumerate(pool.feed(slots, chunks)):
                got[i].append(y)
        for i, y in enumerate(pool.close(slots)):
            got[i].append(y)
        got = [torch.cat(g_) for g_ in got]
        worst = 0.0
        for i, r in enumerate(rates):
            sig = torch.cat([c[i] for c in calls])
            assert got[i].numel() == sig.numel()
            net.reset_stream()
            if r == 16000:
                want = torch.cat([net.feed(sig[None]), net.flush()], 1)[0]
            else:
                rin, rout = StreamResampler(1, r, 16000, cuda), StreamResampler(1, 16000, r, cuda)
                ys = [rout.push(net.feed(rin.push(c[i][None]))) for c in calls]
                ys += [rout.push(net.feed(rin.finish())), rout.push(net.flush()), rout.finish()]
                want = torch.cat(ys, 1)[0, :sig.numel()]
            assert want.numel() == sig.numel() and float(want.abs().max()) > 0
            worst = max(worst, rel_l2(got[i], want))
    record("layers_pool_rated[BIG]", worst)
    print(f"layers pool rated slots: worst rel_l2 {worst:.3e}")
    assert worst < 5e-5
