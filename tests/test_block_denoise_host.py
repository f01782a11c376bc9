"""Block denoising, the parts that need no GPU: the window schedule (a pure function), the argument checks of the two
entering-state C entries (made before any launch), and util.sampling's plain route."""
import ctypes

import pytest
import torch


def _valid_length(length, E, K=4, S=2):
    """CleanUMamba.valid_length, restated."""
    import math
    for _ in range(E):
        length = 1 if length < K else 1 + math.ceil((length - K) / S)
    for _ in range(E):
        length = (length - 1) * S + K
    return int(length)


@pytest.mark.parametrize("block_hops", [2, 3, 7, 16, 61, 625])
@pytest.mark.parametrize("L", [1, 300, 767, 4099, 16000, 160000])
@pytest.mark.parametrize("E", [4, 8])
def test_window_schedule(E, L, block_hops):
    from cleanumamba_amd.network.blockdenoise import block_schedule, padded_length
    hop, F = 2 ** E, _valid_length(1, E)
    T0 = _valid_length(L, E)
    assert padded_length(L, F, hop) == T0
    sched = block_schedule(L, block_hops, F, hop)
    ncol = (T0 - F) // hop + 1
    pos, tau = 0, 0
    for i, w in enumerate(sched):
        # context is 0, then 2
        assert w.context == (0 if i == 0 else 2)
        # consecutive column ranges, at least two columns per block (a one-column signal has one block of one)
        assert w.tau0 == tau and w.tau1 > w.tau0
        assert w.tau1 - w.tau0 >= 2 or ncol == 1
        assert w.tau1 - w.tau0 <= block_hops + 1
        tau = w.tau1
        # the window starts `context` columns early, ends with the last column's frame, and is itself a valid_length
        assert w.win_lo == hop * (w.tau0 - w.context) >= 0
        assert w.win_hi == hop * (w.tau1 - 1) + F <= T0
        assert _valid_length(w.win_hi - w.win_lo, E) == w.win_hi - w.win_lo
        # emit ranges tile [0, T0) once, in order, inside the window's exact part
        assert w.emit_lo == pos == hop * w.tau0 and w.emit_hi > w.emit_lo
        assert w.win_lo <= w.emit_lo and w.emit_hi <= w.win_hi
        pos = w.emit_hi
    assert tau == ncol and pos == T0
    assert all(w.emit_hi == hop * w.tau1 for w in sched[:-1])


def test_schedule_refuses_one_column_blocks():
    from cleanumamba_amd.network.blockdenoise import block_schedule
    with pytest.raises(ValueError):
        block_schedule(16000, 1, 766, 256)


def test_entering_state_entries_check_arguments_before_any_launch():
    from cleanumamba_amd import hip
    lib = hip.lib()
    fake = lambda a: ctypes.c_void_p(a)               # never dereferenced: the checks come before any launch
    data = [fake(0x100000 + 0x10000 * i) for i in range(9)]
    s = hip.ScanShape()
    s.batch, s.dim, s.dstate, s.len = 2, 4, 200, 4
    assert lib.cum_selective_scan_fwd_from(ctypes.byref(s), *data, fake(0x900000), fake(0xa00000), None, None) == -1
    assert b"d_state" in lib.cum_last_error()
    s.dstate = 8
    st = 0x900000                                      # 2 * 4 * 8 floats = 256 bytes
    for off in (0, 4, 252, -252):
        rc = lib.cum_selective_scan_fwd_from(ctypes.byref(s), *data, fake(st), fake(st + off), None, None)
        assert rc == -1 and b"overlap" in lib.cum_last_error(), off
    c = hip.ConvShape()
    c.batch, c.dim, c.len, c.width = 2, 4, 4, 9
    assert lib.cum_causal_conv1d_fwd_from(ctypes.byref(c), *data[:4], fake(st), fake(st + 0x1000), None) == -1
    assert b"width" in lib.cum_last_error()
    c.width = 4                                        # 2 * 4 * 4 floats = 128 bytes
    for off in (0, 4, 124, -124):
        rc = lib.cum_causal_conv1d_fwd_from(ctypes.byref(c), *data[:4], fake(st), fake(st + off), None)
        assert rc == -1 and b"overlap" in lib.cum_last_error(), off


def test_sampling_without_split_calls_the_net_once_under_no_grad():
    from cleanumamba_amd.util.util import sampling
    calls = []

    class Net(torch.nn.Module):
        def forward(self, x):
            calls.append((x.shape, torch.is_grad_enabled()))
            return x * 2

        def denoise_long(self, x, block_size):
            calls.append(("long", block_size))
            return x

    x = torch.randn(2, 1, 100, requires_grad=True)
    y = sampling(Net(), x)
    assert calls == [((2, 1, 100), False)] and not y.requires_grad and torch.equal(y, x.detach() * 2)
    sampling(Net(), x, split_sampling=True, block_size=4096)
    assert calls[-1] == ("long", 4096) and len(calls) == 2
