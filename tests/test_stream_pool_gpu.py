"""Stream pool (cleanumamba_amd/network/streampool.py, csrc/hop.hip cum_stream_hop_slots / cum_stream_pool_stage) on
the GPU: slots that join, feed ragged chunks and leave on their own, against feed_batch / flush_batch, forward and a lone
feed / flush."""
import numpy as np
import pytest
import torch

from conftest import load_ckpt, record, rel_l2

pytestmark = pytest.mark.gpu

NAMES = ["pruned500k", "442k", "e6_pruned2m"]


def _net(name, cuda):
    from cleanumamba_amd.network import CleanUMamba
    sd, cfg = load_ckpt(name)
    net = CleanUMamba(**cfg)
    (net.load_state_dict if name == "442k" else net.load_pruned_state_dict)(sd)
    return net.to(cuda).float().eval()


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_pool_in_lock_step_is_bit_identical_to_feed_batch(cuda, name, normalize):
    """All slots open together and get the same chunks (a first chunk short of a frame, crumbs, many hops): the pool's
    output, close included, is bit for bit feed_batch + flush_batch's."""
    net = _net(name, cuda)
    net.normalize_input = normalize
    hop, F, S = net.total_stride, net.frame_length, 5
    sizes = [F - 40, 57, hop, 16 * hop + 3, 1, 5 * hop - 9, 2 * hop]
    x = (0.1 * torch.randn(S, sum(sizes), generator=torch.Generator().manual_seed(7))).to(cuda)
    x[2] *= 6.0
    with torch.no_grad():
        net.reset_stream()
        ref, i = [], 0
        for n in sizes:
            ref.append(net.feed_batch(x[:, i:i + n]))
            i += n
        ref.append(net.flush_batch())
        ref = torch.cat(ref, 1)
    pool = net.stream_pool(8)
    slots = pool.open(S)
    got, i = [[] for _ in range(S)], 0
    for n in sizes:
        for s, y in enumerate(pool.feed(slots, x[:, i:i + n])):
            assert y.dim() == 1 and y.numel() % hop == 0
            got[s].append(y)
        i += n
    for s, y in enumerate(pool.close(slots)):
        got[s].append(y)
    got = torch.stack([torch.cat(g) for g in got])
    assert got.shape == ref.shape == x.shape and float(ref.abs().max()) > 0
    assert torch.equal(got, ref)
    assert pool.live == [] and float(pool.state.abs().max()) == 0 and float(pool.hist.abs().max()) == 0


def _staggered_run(net, signals, joins, capacity, rng_seed):
    """Drive a pool through a churn schedule: stream k joins at call joins[k] and feeds its signal in ragged chunks
    (the list form of feed: a different length per slot); in some calls only part of the live slots is named; a stream
    closes in the call after its last sample.  Returns each stream's output and the largest number of slots one slotted
    launch ran."""
    rng = np.random.default_rng(rng_seed)
    hop = net.total_stride
    pool = net.stream_pool(capacity)
    slot_of, pos, outs, finished = {}, {}, {k: [] for k in range(len(signals))}, set()
    most, call = 0, 0
    while len(finished) < len(signals):
        for k in [k for k, c in enumerate(joins) if c == call]:
            slot_of[k], pos[k] = pool.open()[0], 0
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
    assert pool.live == []
    return [torch.cat(outs[k]) for k in range(len(signals))], most


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_pool_staggered_joins_ragged_chunks_and_reuse(cuda, name, normalize):
    """More slots than the chip has CUs: 220 streams join in call 0, 72 in call 3, 60 in call 17 (into the ids of streams
    that have left), at sample offsets off the hop grid, with ragged chunks, leaving at different times.  Each stream's
    output: normalisation off, the parallel forward of its own signal; on, a lone feed / flush of it."""
    net = _net(name, cuda)
    net.normalize_input = normalize
    hop = net.total_stride
    g = torch.Generator().manual_seed(11)
    rng = np.random.default_rng(5)
    joins = [0] * 220 + [3] * 72 + [17] * 60
    lengths = [int(rng.integers(2, 9)) * hop + int(rng.integers(0, hop)) if k < 30 else
               int(rng.integers(20, 60)) * hop + int(rng.integers(0, hop)) for k in range(len(joins))]
    lengths[5] = 3                                       # a stream that never reaches a frame
    signals = [(0.1 * float(1 + k % 5) * torch.randn(n, generator=g)).to(cuda) for k, n in enumerate(lengths)]
    with torch.no_grad():
        outs, most = _staggered_run(net, signals, joins, 330, 1)
    assert most > 256
    worst = 0.0
    with torch.no_grad():
        if not normalize:
            for k, sig in enumerate(signals):
                par = net(sig.view(1, 1, -1))[0, 0, :sig.numel()]
                assert outs[k].shape == sig.shape
                worst = max(worst, rel_l2(outs[k], par))
            record(f"pool_staggered[{name}]", worst)
            assert worst < 1e-4
        else:
            for k in list(range(0, len(signals), 11)) + [5]:
                net.reset_stream()
                lone = torch.cat([net.feed(signals[k].view(1, -1)), net.flush()], 1)[0]
                assert outs[k].shape == lone.shape
                worst = max(worst, rel_l2(outs[k], lone))
            record(f"pool_staggered_norm[{name}]", worst)
            assert worst < 5e-5


@pytest.mark.parametrize("name", NAMES)
def test_pool_slots_are_isolated(cuda, name):
    """Group A's outputs are bit for bit the same whether or not group B joins (with a join offset of its own), feeds in
    the same calls and leaves during A's life."""
    net = _net(name, cuda)
    net.normalize_input = True
    hop = net.total_stride
    xa = (0.1 * torch.randn(4, 30 * hop, generator=torch.Generator().manual_seed(2))).to(cuda)
    xb = (0.3 * torch.randn(6, 30 * hop, generator=torch.Generator().manual_seed(3))).to(cuda)
    cuts = [0, net.frame_length + 3, 4 * hop, 9 * hop + 7, 13 * hop, 20 * hop + 1, 26 * hop, 30 * hop]
    results = []
    with torch.no_grad():
        for with_b in (False, True):
            pool = net.stream_pool(16)
            a = pool.open(4)
            outs = [[] for _ in a]
            b = None
            for c in range(len(cuts) - 1):
                chunk = xa[:, cuts[c]:cuts[c + 1]]
                if with_b and c == 2:
                    b = pool.open(6)
                    pool.feed(b, xb[:, :hop + 77])
                if b is not None and 2 < c < 5:
                    ys = pool.feed(a + b, torch.cat([chunk, xb[:, cuts[c]:cuts[c + 1]]]))[:4]
                else:
                    ys = pool.feed(a, chunk)
                if b is not None and c == 5:
                    pool.close(b)
                    b = None
                for s, y in enumerate(ys):
                    outs[s].append(y)
            for s, y in enumerate(pool.close(a)):
                outs[s].append(y)
            results.append(torch.stack([torch.cat(o) for o in outs]))
    assert results[0].shape == xa.shape and float(results[0].abs().max()) > 0
    assert torch.equal(results[0], results[1])


@pytest.mark.parametrize("name", NAMES)
def test_pool_calls_leave_other_slots_untouched(cuda, name):
    """The state rows and the history of slots a call does not name are bit-unchanged by it -- a feed, a join, a close."""
    net = _net(name, cuda)
    hop = net.total_stride
    x = (0.1 * torch.randn(8, 12 * hop, generator=torch.Generator().manual_seed(4))).to(cuda)
    with torch.no_grad():
        pool = net.stream_pool(12)
        a, b = pool.open(4), pool.open(4)
        pool.feed(a + b, x[:, :5 * hop + 33])
        rows = torch.tensor(b, device=cuda)
        st0, h0 = pool.state[rows].clone(), pool.hist[rows].clone()
        assert float(st0.abs().max()) > 0 and float(h0.abs().max()) > 0
        pool.feed(a, x[:4, 5 * hop + 33:9 * hop])                      # a feed
        c = pool.open(2)
        pool.feed(c + a[:1], x[:3, :net.frame_length + 5])              # a join
        pool.close(a[1:3])                                              # a close
        assert torch.equal(pool.state[rows], st0) and torch.equal(pool.hist[rows], h0)
        closed = torch.tensor(a[1:3], device=cuda)
        assert float(pool.state[closed].abs().max()) == 0 and float(pool.hist[closed].abs().max()) == 0


def test_pool_weight_change_and_the_models_own_stream(cuda):
    """An in-place weight change while the pool is live (the blob is re-packed, the slots keep their state) -- the
    model's own feed_batch / flush_batch stream runs on the same model between the pool's calls, through the same
    change, and the two agree bit for bit."""
    net = _net("pruned500k", cuda)
    hop, S = net.total_stride, 3
    x = (0.1 * torch.randn(S, 20 * hop, generator=torch.Generator().manual_seed(9))).to(cuda)
    w0 = net.decoder[3][0].weight.detach().clone()
    with torch.no_grad():
        net.reset_stream()
        pool = net.stream_pool(4)
        slots = pool.open(S)
        ref, got = [], [[] for _ in range(S)]
        for c, (i, j) in enumerate([(0, 8 * hop), (8 * hop, 13 * hop + 5), (13 * hop + 5, 20 * hop)]):
            if c == 1:
                net.decoder[3][0].weight.mul_(1.5)              # in place: bumps the parameter's version counter
            ref.append(net.feed_batch(x[:, i:j]))
            for s, y in enumerate(pool.feed(slots, x[:, i:j])):
                got[s].append(y)
        assert net.hop_kernel_status == "active"
        ref.append(net.flush_batch())
        for s, y in enumerate(pool.close(slots)):
            got[s].append(y)
        net.decoder[3][0].weight.copy_(w0)
    ref = torch.cat(ref, 1)
    got = torch.stack([torch.cat(g) for g in got])
    assert torch.equal(got, ref)
    assert rel_l2(ref[:, 10 * hop:], ref[:, :10 * hop].new_zeros(1)) > 0
