"""Stream pool (cleanumamba_amd/network/streampool.py) on the host: the per-call scheduler as a pure function, checked
against a per-slot restatement of feed_batch's loop, and the argument errors of the pool's interface.  (The kernels:
-m gpu, tests/test_stream_pool_gpu.py.)"""
import numpy as np
import pytest

from conftest import load_ckpt


def _net(name):
    from cleanumamba_amd.network import CleanUMamba
    sd, cfg = load_ckpt(name)
    net = CleanUMamba(**cfg)
    (net.load_state_dict if name == "442k" else net.load_pruned_state_dict)(sd)
    return net.eval()


def _lone_stream(pending, started, length, frame_len, hop):
    """CleanUMamba.feed_batch's loop for one stream: (first frame?, kernel hops, samples consumed)."""
    total, first, hops, consumed = pending + length, False, 0, 0
    while total - consumed >= frame_len:
        if not started and not first:
            first = True                        # per-layer path: one frame of whole windows
            consumed += hop
            continue
        n = (total - consumed - frame_len) // hop + 1      # the one-launch hop: every remaining hop at once
        hops += n
        consumed += n * hop
    return first, hops, consumed


def test_scheduler_matches_feed_batch_for_every_slot():
    from cleanumamba_amd.network.streampool import schedule
    frame_len, hop = 766, 256                    # the E8 models
    rng = np.random.default_rng(3)
    pending = rng.integers(0, frame_len, 400)
    started = rng.random(400) < 0.6
    pending[~started] = rng.integers(0, frame_len, int((~started).sum()))
    lengths = rng.choice([0, 1, 17, hop - 1, hop, hop + 1, 3 * hop + 5, 16 * hop, 40 * hop + 77], 400)
    sch = schedule(pending, started, lengths, frame_len, hop)
    for i in range(400):
        first, hops, consumed = _lone_stream(int(pending[i]), bool(started[i]), int(lengths[i]), frame_len, hop)
        assert bool(sch.first[i]) == first and int(sch.n_hops[i]) == hops and int(sch.consumed[i]) == consumed
        assert int(sch.offset[i]) == (hop if first else 0)
        assert int(sch.remainder[i]) == pending[i] + lengths[i] - consumed
        assert 0 <= sch.remainder[i] < frame_len                  # the history row holds frame_len - 1 samples
        assert sch.consumed[i] % hop == 0


def test_scheduler_joins_at_offsets_off_the_hop_grid():
    from cleanumamba_amd.network.streampool import schedule
    F, hop = 190, 64                              # an E6 model
    # slot 0 joins with a chunk short of a frame, 1 reaches its first frame exactly, 2 with a first frame and 2 hops,
    # 3 had 37 samples pending (an odd offset) and gets its first frame plus one hop, 4 is running and gets a crumb
    sch = schedule([0, 0, 0, 37, 150], [False, False, False, False, True], [189, 190, 190 + 2 * hop + 5, 153 + hop + 3, 39],
                   F, hop)
    assert sch.first.tolist() == [False, True, True, True, False]
    assert sch.n_hops.tolist() == [0, 0, 2, 1, 0]
    assert sch.offset.tolist() == [0, hop, hop, hop, 0]
    assert sch.consumed.tolist() == [0, hop, 3 * hop, 2 * hop, 0]
    assert sch.remainder.tolist() == [189, 190 - hop, 190 + 2 * hop + 5 - 3 * hop, 37 + 153 + hop + 3 - 2 * hop, 189]
    # after a first frame the slot holds frame_len - hop samples plus its offset in the hop grid
    assert sch.remainder[3] == F - hop + 3
    # one more sample makes the running slot's next hop
    assert schedule([189], [True], [1], F, hop).n_hops.tolist() == [1]


def test_pool_argument_errors():
    from cleanumamba_amd.network import hopplan
    net = _net("pruned500k")
    pool = net.stream_pool(4)
    assert pool.capacity == 4 and pool.live == []
    a = pool.open(3)
    assert a == [0, 1, 2] and pool.live == [0, 1, 2]
    with pytest.raises(ValueError, match="asked for"):
        pool.open(2)                                  # capacity exceeded: one slot left
    with pytest.raises(ValueError, match="twice"):
        pool.feed([0, 0], np.zeros((2, 10), np.float32))
    with pytest.raises(ValueError, match="not open"):
        pool.feed([3], np.zeros((1, 10), np.float32))
    with pytest.raises(ValueError, match="lie in"):
        pool.feed([4], np.zeros((1, 10), np.float32))
    assert pool.close([1])[0].numel() == 0            # never fed: nothing to emit
    assert pool.live == [0, 2]
    with pytest.raises(ValueError, match="not open"):
        pool.close([1])
    with pytest.raises(ValueError, match="not open"):
        pool.feed([0, 1], np.zeros((2, 10), np.float32))
    assert pool.open() == [1]                         # the lowest free id is reused
    pool.reset()
    assert pool.live == [] and pool.pending([]) == []
    with pytest.raises(ValueError):
        net.stream_pool(0)
    assert hopplan.unsupported_reason(net) is None


def test_pool_refuses_the_models_the_one_launch_hop_declines():
    from cleanumamba_amd.network import CleanUMamba, hopplan
    sd, cfg = load_ckpt("mamba2")
    m2 = CleanUMamba(**cfg)
    m2.load_pruned_state_dict(sd)
    why = hopplan.unsupported_reason(m2)
    assert "Mamba2" in why
    with pytest.raises(ValueError, match="Mamba2"):
        m2.stream_pool(8)
    half = _net("442k").half()
    with pytest.raises(ValueError, match="not f32"):
        half.stream_pool(8)


def test_entry_points_check_every_record_before_a_launch():
    """cum_stream_hop_slots / cum_stream_pool_stage read the host copy of their table and refuse a slot outside the pool,
    a record without a hop and rows that do not fit -- before anything is launched (no GPU needed)."""
    import ctypes
    from cleanumamba_amd import hip
    lib = hip.lib()
    fake = ctypes.c_void_p(1 << 20)                      # never dereferenced: every check runs before the launch

    def hop_rc(rec, capacity=4):
        t = np.asarray(rec, dtype=np.int32).reshape(-1, 8)
        p = ctypes.c_void_p(t.ctypes.data)
        return lib.cum_stream_hop_slots(fake, fake, fake, 64, capacity, p, fake, t.shape[0], fake, 100, fake, 100,
                                        1024, None)

    assert hop_rc([4, 1, 0, 0, 0, 0, 0, 0]) == -1 and b"slot" in lib.cum_last_error()
    assert hop_rc([-1, 1, 0, 0, 0, 0, 0, 0]) == -1
    assert hop_rc([0, 2, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0]) == -1 and b"n_hops" in lib.cum_last_error()
    assert hop_rc([0, 1, 0, -3, 0, 0, 0, 0]) == -1

    def stage_rc(rec, hist_stride=12, stage_stride=40):
        t = np.asarray(rec, dtype=np.int32).reshape(-1, 8)
        p = ctypes.c_void_p(t.ctypes.data)
        return lib.cum_stream_pool_stage(fake, hist_stride, 4, p, fake, t.shape[0], fake, 100, fake, stage_stride, None)

    assert stage_rc([7, 0, 10, 0, 0, 0, 0, 0]) == -1 and b"slot" in lib.cum_last_error()
    assert stage_rc([0, 13, 0, 0, 0, 0, 0, 0]) == -1                 # more pending than the history holds
    assert stage_rc([0, 10, 31, 0, 0, 0, 0, 0]) == -1                 # the row does not fit the stage row
    assert stage_rc([0, 10, 20, 5, 0, 0, 0, 0]) == -1                 # 25 samples left for a 12-sample history
    assert stage_rc([0, 10, 20, 31, 0, 0, 0, 0]) == -1                # consumes more than it has
