"""Host side of rated pool slots (network/streampool.py, util/resample.py, csrc/resample.hip cum_resample_slots): the
per-stream bookkeeping against the definitions, ``open(rate=...)`` validation and every argument error of the C entry --
all of it before any launch, so without a GPU."""
import ctypes

import numpy as np
import pytest

from conftest import load_ckpt

RATES = [8000, 22050, 32000, 44100, 48000]
PAIRS = [(r, 16000) for r in RATES] + [(16000, r) for r in RATES]


@pytest.mark.parametrize("pair", PAIRS)
def test_stream_step_against_the_definitions(pair):
    """Whatever the cuts: the outputs declared final sum to final_outputs(received), after the end to out_length(total);
    the history never exceeds history_bound and always holds the oldest sample the next output reads."""
    from cleanumamba_amd.util.resample import final_outputs, history_bound, out_length, plan, stream_step
    up, down, H, K, _ = plan(*pair)
    rng = np.random.default_rng(sum(pair))
    longest = 0
    for trial in range(12):
        cuts = [0, 1, K - 1, K, K + 1] + [int(v) for v in rng.integers(0, 3, 6)] + [int(v) for v in rng.integers(0, 40, 10)]
        cuts += [int(v) for v in rng.integers(0, 3 * K, 10)] + [int(v) for v in rng.integers(0, 5000, 4)]
        cuts = [cuts[i] for i in rng.permutation(len(cuts))]
        if trial == 0:
            cuts = [0, 1, K - 1, K, K + 1] + cuts        # the named sizes first, from the start of the signal
        received = emitted = base = 0
        for n in cuts:
            count, start = stream_step(received, emitted, base, n, up, down, H, K)
            received += n
            emitted += count
            assert count >= 0 and emitted == final_outputs(received, up, down, H), (pair, cuts)
            assert base <= start <= received
            assert received - start <= history_bound(K)
            # output `emitted` reads inputs (emitted down + H) // up - (K - 1) ... (positions below 0 are zeros)
            assert start <= max((emitted * down + H) // up - (K - 1), 0)
            longest = max(longest, received - start)
            base = start
        # the array form is the scalar form, entry by entry
        many = stream_step(np.array([received, 0]), np.array([emitted, 0]), np.array([base, 0]), np.array([7, 3]),
                           np.array([up, up]), np.array([down, down]), np.array([H, H]), np.array([K, K]), False)
        for i, (r, e, b, n) in enumerate([(received, emitted, base, 7), (0, 0, 0, 3)]):
            one = stream_step(r, e, b, n, up, down, H, K)
            assert (int(many[0][i]), int(many[1][i])) == (int(one[0]), int(one[1]))
        count, start = stream_step(received, emitted, base, 0, up, down, H, K, ends=True)
        assert emitted + count == out_length(received, up, down) and base <= start <= received
        ended = stream_step(np.array([received]), np.array([emitted]), np.array([base]), np.array([0]), np.array([up]),
                            np.array([down]), np.array([H]), np.array([K]), True)
        assert (int(ended[0][0]), int(ended[1][0])) == (count, start)
    assert longest == history_bound(K) == K - 1            # the bound is reached: the rows are not sized too large


def test_stream_resampler_uses_the_same_bookkeeping():
    """``StreamResampler.push`` kept its arithmetic: the history start it used to compute is stream_step's."""
    from cleanumamba_amd.util.resample import final_outputs, plan, stream_step
    for pair in PAIRS:
        up, down, H, K, _ = plan(*pair)
        received = emitted = base = 0
        for n in (3, 0, 700, 1, 2 * K, 5):
            count, start = stream_step(received, emitted, base, n, up, down, H, K)
            received += n
            emitted = final_outputs(received, up, down, H)
            assert start == min(max((emitted * down + H) // up - (K - 1), base), received)
            base = start


def _net(name):
    from cleanumamba_amd.network import CleanUMamba
    sd, cfg = load_ckpt(name)
    net = CleanUMamba(**cfg)
    (net.load_state_dict if name == "442k" else net.load_pruned_state_dict)(sd)
    return net.float().eval()


def test_open_checks_the_rate_before_anything_else():
    net = _net("pruned500k")
    pool = net.stream_pool(6)
    assert pool.model_rate == 16000 and net.stream_pool(2, model_rate=8000).model_rate == 8000
    for bad in (44100.5, 0, -48000, "48k", True):
        with pytest.raises(ValueError, match="positive integer"):
            pool.open(1, rate=bad)
    for bad in (16001, 1, 48001):                          # 16001/16000, 16000/1, 48001/16000: factors above 1024
        with pytest.raises(ValueError, match=str(bad)):
            pool.open(1, rate=bad)
    with pytest.raises(ValueError, match="768000.*LDS"):   # 1/48 reduces, but a tile's input span is too long
        pool.open(1, rate=768000)
    assert pool.live == [] and pool.rs_hist is None        # nothing was opened, nothing allocated
    with pytest.raises(ValueError):
        net.stream_pool(2, model_rate=0)
    a = pool.open(2, rate=16000)
    b = pool.open(1)
    c = pool.open(1, rate=16000.0)
    assert pool.rate(a + b + c) == [16000] * 4 and pool.rs_hist is None and not pool._rate.any()   # unrated slots
    d = pool.open(2, rate=48000)
    assert pool.rate(d) == [48000, 48000] and pool.live == [0, 1, 2, 3, 4, 5] and pool.pending(d) == [0, 0]
    with pytest.raises(ValueError):
        pool.rate([7])
    pool.reset()
    assert pool.live == [] and not pool._rate.any() and float(pool.rs_hist.abs().max()) == 0
    assert pool.open(1, rate=44100) == [0] and pool.rate([0]) == [44100]
    from cleanumamba_amd.util.resample import history_bound, plan
    assert pool.rs_hist.shape[:3] == (2, 6, 2) and pool.rs_hist.shape[3] >= history_bound(plan(48000, 16000).K)


# ---------------------------------------------------------------------------------- the C entry's argument checks
P = ctypes.c_void_p
PLAN_48_16 = [1, 3, 219, 219, 220, 0, 0, 0]
PLAN_16_441 = [441, 160, 31947, 73, 76, 220, 0, 0]
TABLE_FLOATS = 220 + 441 * 76


def _rec(slot=0, plan=0, n_hist=218, x_row=0, n_new=960, n_out=320, y_row=0, ends=0, keep=218, parity=0, y_col=0,
         in0=1000 - 218, out0=None):
    if out0 is None:                                       # a stream 1000 samples in: what was final is out
        up, down, n_taps = (PLAN_48_16 if plan == 0 else PLAN_16_441)[:3]
        out0 = max(0, -(-(1000 * up - (n_taps - 1) // 2) // down))
    r = np.zeros(16, dtype=np.int32)
    r[:11] = [slot, plan, n_hist, x_row, n_new, n_out, y_row, ends, keep, parity, y_col]
    r.view(np.int64)[6:] = [in0, out0]
    return r


def _call(lib, records, plan_rows=(PLAN_48_16, PLAN_16_441), **over):
    plans = np.asarray(plan_rows, dtype=np.int32).reshape(-1, 8)
    recs = np.ascontiguousarray(np.stack(records)) if len(records) else np.zeros((0, 16), dtype=np.int32)
    a = dict(hist=P(0x10000), hist_pitch=220, capacity=4, plans_host=P(plans.ctypes.data), plans=P(0x20000),
             n_plans=plans.shape[0], tables=P(0x30000), table_floats=TABLE_FLOATS, recs_host=P(recs.ctypes.data),
             recs=P(0x40000), n_recs=recs.shape[0], x=P(0x50000), x_rows=2, x_pitch=1000, y=P(0x60000), y_rows=2,
             y_pitch=400)
    a.update(over)
    return lib.cum_resample_slots(*a.values(), None)


def test_slots_entry_refuses_bad_arguments_before_any_launch():
    from cleanumamba_amd import hip
    lib = hip.lib()
    assert "cum_resample_slots" in hip.SIGNATURES and lib.cum_abi_version() == 16

    def refused(text, records=None, **over):
        rc = _call(lib, [_rec()] if records is None else records, **over)
        assert rc == -1, (text, over)
        assert text in lib.cum_last_error(), (text, over, lib.cum_last_error())

    # no records: the plans are checked, nothing is launched
    assert _call(lib, []) == 0
    # pointers
    for name in ("hist", "plans_host", "plans", "tables", "recs_host", "recs", "x", "y"):
        refused(b"null pointer", **{name: None})
    assert _call(lib, [], x=None, x_rows=0) == 0           # no chunk rows: x may be null
    refused(b"16-byte", tables=P(0x30004))
    for name in ("hist", "plans", "x", "y"):
        refused(b"misaligned", **{name: P(0x70002)})
    refused(b"misaligned", recs=P(0x40004))
    # shapes
    refused(b"capacity", capacity=0)
    refused(b"n_plans", n_plans=0)
    for name in ("hist_pitch", "table_floats", "x_rows", "x_pitch", "y_rows", "y_pitch"):
        refused(b"negative", **{name: -1})
    # plan fields: the limits of cum_resample_ragged, and the table inside the blob
    for field, value, text in [(0, 0, b"up and down"), (1, 0, b"up and down"), (1, -3, b"up and down"), (0, 1025, b"1024"),
                               (1, 1025, b"1024"), (2, 218, b"odd"), (2, 0, b"odd"), (3, 218, b"smaller than the tap count"),
                               (3, 0, b"smaller than the tap count"), (4, 216, b"table_pitch"), (4, 222, b"table_pitch"),
                               (5, -4, b"blob"), (5, 2, b"blob"), (5, TABLE_FLOATS, b"blob")]:
        bad = list(PLAN_48_16)
        bad[field] = value
        refused(text, plan_rows=(bad, PLAN_16_441))
    refused(b"LDS", plan_rows=([1, 48, 3477, 3477, 3480, 0, 0, 0],), table_floats=3480)
    refused(b"blob", table_floats=TABLE_FLOATS - 1)
    # records
    refused(b"slot outside", records=[_rec(slot=4)])
    refused(b"slot outside", records=[_rec(slot=-1)])
    refused(b"named twice", records=[_rec(slot=1), _rec(slot=2), _rec(slot=1)])
    refused(b"plan outside", records=[_rec(plan=2)])
    refused(b"plan outside", records=[_rec(plan=-1)])
    refused(b"parity", records=[_rec(parity=2)])
    refused(b"history count", records=[_rec(n_hist=221, in0=1000 - 221)])
    refused(b"history count", records=[_rec(n_hist=-1)])
    refused(b"chunk", records=[_rec(n_new=1001)])
    refused(b"chunk", records=[_rec(n_new=-1)])
    refused(b"chunk", records=[_rec(x_row=2)])
    refused(b"chunk", records=[_rec(x_row=-1)])
    refused(b"history to keep", records=[_rec(keep=221)])
    refused(b"history to keep", records=[_rec(keep=-1)])
    refused(b"history to keep", records=[_rec(n_hist=5, n_new=3, n_out=0, keep=9, in0=0, out0=0)])
    refused(b"outputs do not fit", records=[_rec(y_col=81)])
    refused(b"outputs do not fit", records=[_rec(y_col=-1)])
    refused(b"outputs do not fit", records=[_rec(n_out=-1)])
    refused(b"outputs do not fit", records=[_rec(y_row=2)])
    refused(b"outputs do not fit", records=[_rec(n_out=320)], y_pitch=319)
    refused(b"position", records=[_rec(in0=-1)])
    refused(b"position", records=[_rec(out0=-1)])
    refused(b"position", records=[_rec(in0=1 << 52)])
    refused(b"more outputs", records=[_rec(n_out=321)])     # 960 new samples at 3:1 make 320 outputs final
    refused(b"more outputs", records=[_rec(n_out=358, ends=1)], y_pitch=500)   # ... and the signal's end 37 more, not 38
    refused(b"oldest sample", records=[_rec(n_hist=217, in0=1000 - 217, keep=217)])
    # (a good record gets past every check only with a GPU: tests/test_pool_rates_gpu.py)
