"""The stream pool's "layers" backend (network/streampool.py, network/layerpool.py, csrc/slotstate.hip) on the host: the
backend choice, the slot row's segment table as a pure function of the model, the checks cum_stream_slots_move makes
before a launch, and the pool's argument errors.  (The kernels: -m gpu, tests/test_layer_pool_gpu.py.)"""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_ckpt

BIG = dict(channels_input=1, channels_output=1, channels_H=64, max_H=256, encoder_n_layers=8, kernel_size=4, stride=2,
           tsfm_d_model=256, tsfm_d_inner=1024, tsfm_n_head=8, tsfm_n_layers=3)


def _net(name):
    from cleanumamba_amd.network import CleanUMamba
    sd, cfg = load_ckpt(name)
    net = CleanUMamba(**cfg)
    (net.load_state_dict if name == "442k" else net.load_pruned_state_dict)(sd)
    return net.eval()


def _big(**over):
    from cleanumamba_amd.network import CleanUMamba
    torch.manual_seed(1234)
    return CleanUMamba(**dict(BIG, **over)).eval()


def test_a_model_above_the_limit_gets_the_layers_backend():
    from cleanumamba_amd.network import hopplan
    big = _big()
    assert sum(p.numel() for p in big.parameters()) > hopplan.MAX_PARAMS
    assert hopplan.unsupported_reason(big) == "weights too large to be re-read per stream"
    assert hopplan.pool_backend(big) == "layers"
    pool = big.stream_pool(4)
    assert pool.backend == "layers" and pool.capacity == 4 and pool.live == []
    assert pool.state.shape == (4, pool.plan.state_stride) and pool.state.dtype == torch.float32
    with pytest.raises(ValueError, match="too large"):
        big.stream_pool(4, backend="kernel")
    with pytest.raises(ValueError, match="backend"):
        big.stream_pool(4, backend="graph")


def test_backend_of_a_small_model_and_forcing():
    from cleanumamba_amd.network import hopplan
    for name in ("pruned500k", "442k"):
        net = _net(name)
        assert hopplan.pool_backend(net) == "kernel" and hopplan.unsupported_reason(net) is None
        assert net.stream_pool(3).backend == "kernel"
        assert net.stream_pool(3, backend="kernel").backend == "kernel"
        forced = net.stream_pool(3, backend="layers")
        assert forced.backend == "layers" and forced.dense is not None
        assert forced.hop == net.total_stride and forced.frame_len == net.valid_length(1)


def test_obstacles_that_are_not_of_size_still_raise():
    """unsupported_reason checks size first, so a large Mamba2 / half model answers "too large" there: the backend choice
    looks at the other reasons on their own and keeps refusing, with the same text."""
    from cleanumamba_amd.network import hopplan
    m2 = _big(mamba_v2=True)
    assert hopplan.unsupported_reason(m2) == "weights too large to be re-read per stream"
    with pytest.raises(ValueError, match="Mamba2"):
        hopplan.pool_backend(m2)
    with pytest.raises(ValueError, match="Mamba2"):
        m2.stream_pool(4)
    with pytest.raises(ValueError, match="Mamba2"):
        m2.stream_pool(4, backend="layers")
    half = _big().half()
    assert hopplan.unsupported_reason(half) == "weights too large to be re-read per stream"
    with pytest.raises(ValueError, match="not f32"):
        half.stream_pool(4)
    bf = _big()
    bf.stream_bf16 = True
    with pytest.raises(ValueError, match="stream_bf16"):
        bf.stream_pool(4)
    small = _net("pruned500k")
    small.stream_bf16 = True
    with pytest.raises(ValueError, match="stream_bf16"):
        small.stream_pool(4, backend="layers")


def _expected_names(net):
    E, B = net.encoder_n_layers, len(net.tsfm_Mamba_layers)
    return (["std"] + [f"{k}{i}" for i in range(E) for k in ("encin", "enc")] + [f"dec{j}" for j in range(E)]
            + [f"{k}{b}" for b in range(B) for k in ("conv", "ssm")])


@pytest.mark.parametrize("name", ["pruned500k", "442k", "BIG"])
def test_segment_table(name):
    from cleanumamba_amd.network import convstack as cs, layerpool
    net = _big() if name == "BIG" else _net(name)
    segs, row_bytes = layerpool.segment_table(net)
    assert sorted(s[0] for s in segs) == sorted(_expected_names(net))           # exactly the state, no decbuf
    end = 0
    for seg_name, off, nbytes in segs:                                          # ascending, aligned, no overlap
        assert off % 16 == 0 and nbytes > 0 and nbytes % 4 == 0 and off >= end, seg_name
        end = off + nbytes
    assert row_bytes == cs.rup(end, 16)
    pool = net.stream_pool(2, backend="layers")
    assert pool.plan.state_stride * 4 == row_bytes and pool.state.shape[1] == pool.plan.state_stride
    size = dict((s[0], s[2]) for s in segs)
    # the sizes, from the shapes the fused hop gives its buffers: windows of all P = T + 2 rows, tails (2, Cp), Mamba states
    T, c_in, n_new = net.valid_length(1), 1, net.total_stride
    for i, enc in enumerate(net.encoder):
        T, n_new = (T - 4) // 2 + 1, n_new // 2
        assert size[f"encin{i}"] == (2 * n_new + 2 + 2) * cs.rup(c_in, 8) * 4
        c_in = enc[2].weight.shape[0] // 2
        assert size[f"enc{i}"] == (T + 2) * cs.rup(c_in, 8) * 4
    assert T == 1
    for j, dec in enumerate(net.decoder):
        assert size[f"dec{j}"] == 2 * cs.rup(dec[2].weight.shape[1], 8) * 4
    for b, blk in enumerate(net.tsfm_Mamba_layers):
        conv, ssm = blk.mixer.allocate_inference_cache(1, 1)
        assert size[f"conv{b}"] == conv.numel() * 4 and size[f"ssm{b}"] == ssm.numel() * 4
    assert size["std"] == 4
    # the dense scratch holds `capacity` streams of every segment, and decbuf besides
    assert pool.dense.table.streams == 2 and pool.dense.table.n == len(segs)
    assert sorted(set(pool.dense.layers) - set(size)) == [f"decbuf{j}" for j in range(net.encoder_n_layers - 1)]


def test_mover_checks_every_table_before_a_launch():
    from cleanumamba_amd import hip
    lib = hip.lib()
    fake = 1 << 20                                        # never dereferenced: every check runs before the launch
    fp = ctypes.c_void_p(fake)
    good = [[fake, 64, 0, 16], [fake, 64, 16, 20], [fake, 64, 48, 12]]

    def rc(slots, segs, direction=0, stride=16, capacity=4, clears=None, store=fp, dev_tables=fp):
        s = np.asarray(slots, dtype=np.int32)
        g = np.asarray(segs, dtype=np.int64).reshape(-1, 4)
        c = np.asarray(clears if clears is not None else [], dtype=np.int64).reshape(-1, 4)
        return lib.cum_stream_slots_move(direction, store, stride, capacity, ctypes.c_void_p(s.ctypes.data), dev_tables,
                                         s.size, ctypes.c_void_p(g.ctypes.data), dev_tables, g.shape[0],
                                         ctypes.c_void_p(c.ctypes.data) if c.size else None,
                                         dev_tables if c.size else None, c.shape[0], None)

    assert rc([], good) == 0                                                   # nothing named: nothing launched
    assert rc([4], good) == -1 and b"slot" in lib.cum_last_error()            # outside [0, capacity)
    assert rc([-1], good) == -1 and b"slot" in lib.cum_last_error()
    assert rc([1, 2, 1], good) == -1 and b"twice" in lib.cum_last_error()
    assert rc([0], [[fake, 64, 48, 20]]) == -1 and b"overruns" in lib.cum_last_error()       # 68 bytes in a 64-byte row
    assert rc([0], [[fake, 64, 0, 20], [fake, 64, 16, 16]]) == -1 and b"overlap" in lib.cum_last_error()
    assert rc([0], [[fake, 64, 16, 16], [fake, 64, 0, 20]]) == -1 and b"overlap" in lib.cum_last_error()
    assert rc([0], [[0, 64, 0, 16]]) == -1 and b"null" in lib.cum_last_error()
    assert rc([0], good, store=None) == -1 and b"null" in lib.cum_last_error()
    assert rc([0], good, dev_tables=None) == -1 and b"null" in lib.cum_last_error()
    assert rc([0], good, clears=[[0, 32, 64, 32]]) == -1 and b"null" in lib.cum_last_error()
    assert rc([], good, clears=[[0, 32, 64, 32]]) == -1 and b"null" in lib.cum_last_error()   # (no slot: it only clears)
    assert rc([], good, direction=1, clears=[[0, 32, 64, 32]]) == 0           # a scatter clears nothing
    assert rc([0], [[fake, 64, 0, 18]]) == -1                                 # not whole dwords
    assert rc([0, 1], [[fake, 8, 0, 16]]) == -1 and b"pitch" in lib.cum_last_error()        # dense streams would overlap
    assert rc([0], good, direction=2) == -1
    assert rc([0], [good[0]] * 257) == -1                                      # more segments than the kernel's table


def test_the_entry_point_is_declared_and_the_abi_version_stays():
    from cleanumamba_amd import hip
    assert hip.lib().cum_abi_version() == 16
    res, args = hip.SIGNATURES["cum_stream_slots_move"]
    with open(f"{ROOT}/include/cleanumamba_hip.h") as f:
        header = f.read()
    decl = re.search(r"int cum_stream_slots_move\(([^;]*)\);", header)
    assert decl is not None and len(decl.group(1).split(",")) == len(args) == 14
    assert "#define CUM_ABI_VERSION 16" in header


def test_pool_argument_errors_on_the_layers_backend():
    for net in (_net("pruned500k"), _big()):
        pool = net.stream_pool(4, backend="layers")
        assert pool.backend == "layers" and pool.capacity == 4 and pool.live == []
        a = pool.open(3)
        assert a == [0, 1, 2] and pool.live == [0, 1, 2]
        with pytest.raises(ValueError, match="asked for"):
            pool.open(2)
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
            net.stream_pool(0, backend="layers")


def test_relayout_rechooses_the_backend_unless_it_was_forced():
    """With no slot open, relayout() sizes the store to the model's shapes again; a pool whose backend was chosen follows
    the model across the size limit, a forced one stays."""
    from cleanumamba_amd.network import hopplan
    net = _net("pruned500k")
    chosen, forced = net.stream_pool(2), net.stream_pool(2, backend="layers")
    limit = hopplan.MAX_PARAMS
    try:
        hopplan.MAX_PARAMS = 1000
        chosen.relayout()
        forced.relayout()
        assert chosen.backend == "layers" and chosen.state.shape == forced.state.shape
    finally:
        hopplan.MAX_PARAMS = limit
    chosen.relayout()
    forced.relayout()
    assert chosen.backend == "kernel" and forced.backend == "layers"
    forced.open(1)
    with pytest.raises(RuntimeError, match="close the slots"):
        forced.relayout()
