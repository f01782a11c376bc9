"""Host side of the resampler (util/resample.py, csrc/resample.hip): the definition against scipy, the tap recipe, the
length and finality arithmetic, the C entry's argument checks (they run before any launch, so without a GPU) and the
``resample`` switch of examples/denoise.py."""
import ctypes
import os

import numpy as np
import pytest
import torch
from scipy import signal
from scipy.io import wavfile

import wavtree
from resample_ref import resample_ref

PAIRS = [(48000, 16000), (44100, 16000), (16000, 48000), (16000, 44100), (22050, 16000), (8000, 16000), (32000, 16000)]
TAPS_K = {(48000, 16000): (219, 219), (16000, 48000): (219, 73), (8000, 16000): (147, 74), (32000, 16000): (147, 147),
          (44100, 16000): (31947, 200), (22050, 16000): (31947, 100), (16000, 44100): (31947, 73)}


@pytest.mark.parametrize("pair", PAIRS)
def test_reference_is_scipy_resample_poly(pair):
    from cleanumamba_amd.util.resample import out_length, plan
    up, down, H, K, h = plan(*pair)
    rng = np.random.default_rng(sum(pair))
    for L in (1, 2, 1000, 2777):
        x = rng.standard_normal(L)
        y, A = resample_ref(x, h, up, down)
        want = signal.resample_poly(x, up, down, window=h / up)
        assert len(y) == len(want) == out_length(L, up, down)
        assert np.max(np.abs(y - want)) <= 1e-12, (pair, L)
        assert np.all(A >= np.abs(y) - 1e-12)
    part, _ = resample_ref(x, h, up, down, m0=5, m1=40)
    assert np.array_equal(part, y[5:40])


@pytest.mark.parametrize("pair", PAIRS)
def test_taps_are_odd_symmetric_and_sum_to_up(pair):
    from cleanumamba_amd.util.resample import plan
    p = plan(*pair)
    up, down, H, K, h = p
    assert (up, down) == (pair[1] // np.gcd(*pair), pair[0] // np.gcd(*pair))
    assert len(h) % 2 == 1 and len(h) == 2 * H + 1 and h.dtype == np.float64
    assert (len(h), K) == TAPS_K[pair] and K == -(-len(h) // up)
    assert np.max(np.abs(h - h[::-1])) <= 1e-15 * up
    assert abs(h.sum() - up) <= 1e-12 * up
    tab = p.host_table()
    assert tab.shape == (up, p.pitch) and p.pitch % 4 == 0 and p.pitch >= K and tab.dtype == torch.float32
    for r in (0, up // 2, up - 1):
        row = np.zeros(p.pitch)
        taps = h[r::up]
        row[:len(taps)] = taps
        assert np.array_equal(tab[r].numpy(), row.astype(np.float32))


def test_the_stoi_pair_gives_the_stoi_taps():
    from cleanumamba_amd.util import metrics
    from cleanumamba_amd.util.resample import plan
    p = plan(16000, 10000)
    assert (p.up, p.down) == (5, 8) and np.array_equal(p.taps, metrics.resample_taps())
    assert plan(16000, 10000) is p                       # cached per pair


@pytest.mark.parametrize("pair", PAIRS)
def test_lengths_and_final_outputs(pair):
    from cleanumamba_amd.util.resample import final_outputs, out_length, plan
    up, down, H, K, _ = plan(*pair)
    for L in range(1, 2001):
        n = out_length(L, up, down)
        assert n == -(-L * up // down) and (n - 1) * down < L * up <= n * down
        assert out_length(n, down, up) >= L              # a round trip never shortens a clip
    assert out_length(0, up, down) == 0
    # final_outputs from the definition: output m is final when the newest input it reads has arrived
    prev = 0
    for received in list(range(0, 700)) + [1999, 2000, 20000]:
        m, count = 0, 0
        while m < out_length(received, up, down) and (m * down + H) // up <= received - 1:
            m += 1
        count = m
        got = final_outputs(received, up, down, H)
        assert got == count, (pair, received)
        assert got >= prev
        prev = got
        if received > 0:
            assert got < out_length(received, up, down)  # the last outputs wait for finish()


def test_bad_rates_raise():
    from cleanumamba_amd.util.resample import plan
    for bad in ((16000, 16001), (16001, 16000), (0, 16000), (16000, 0), (-8000, 16000), (44100.5, 16000), ("48k", 16000),
                (True, 16000)):
        with pytest.raises(ValueError):
            plan(*bad)
    assert plan(44100, 48000).up == 160 and plan(16000.0, 16000).identity


def test_new_symbols_and_their_argument_errors_need_no_gpu():
    from cleanumamba_amd import hip
    lib = hip.lib()
    for name in ("cum_resample_tile", "cum_resample_ragged"):
        assert hasattr(lib, name) and name in hip.SIGNATURES
    assert lib.cum_abi_version() == 16
    T = lib.cum_resample_tile()
    assert T >= 64 and T % 64 == 0
    P = ctypes.c_void_p
    order = ["src", "x", "B", "lmax", "in_pitch", "len", "origin", "ends", "up", "down", "taps", "K", "table", "tp", "y",
             "out_pitch", "max_out"]
    ok = dict(src=1, x=P(0x1000), B=3, lmax=1000, in_pitch=1000, len=P(0x2000), origin=None, ends=1, up=1, down=3,
              taps=219, K=219, table=P(0x3000), tp=220, y=P(0x4000), out_pitch=336, max_out=334)
    bad = [("taps", 218, b"odd"), ("taps", 0, b"odd"), ("up", 0, b"up and down"), ("down", 0, b"up and down"),
           ("down", -3, b"up and down"), ("up", 1025, b"1024"), ("K", 218, b"smaller than the tap count"),
           ("K", 0, b"smaller than the tap count"), ("table", None, b"null table"), ("in_pitch", -1, b"negative"),
           ("out_pitch", -1, b"negative"), ("lmax", -1, b"negative"), ("max_out", -1, b"negative"),
           ("in_pitch", 999, b"smaller than its row"), ("out_pitch", 333, b"smaller than its row"),
           ("tp", 219, b"table_pitch"), ("tp", 216, b"table_pitch"), ("x", None, b"null pointer"),
           ("len", None, b"null pointer"), ("y", None, b"null pointer"), ("table", P(0x3004), b"16-byte"),
           ("x", P(0x1001), b"misaligned"), ("origin", P(0x5004), b"misaligned"), ("y", P(0x4002), b"misaligned"),
           ("B", 0, b"batch"), ("src", 2, b"src_i16")]
    for name, value, text in bad:
        args = dict(ok, **{name: value})
        rc = lib.cum_resample_ragged(*[args[k] for k in order], None)
        assert rc == -1, (name, value)
        assert text in lib.cum_last_error(), (name, value, lib.cum_last_error())
    # a ratio whose tile span cannot be staged (1/48: 256 * 48 + 3476 samples) is refused, not truncated
    far = dict(ok, down=48, taps=3477, K=3477, tp=3480)
    assert lib.cum_resample_ragged(*[far[k] for k in order], None) == -1 and b"LDS" in lib.cum_last_error()
    # nothing to write: accepted without a launch (and so without a GPU)
    none = dict(ok, max_out=0)
    assert lib.cum_resample_ragged(*[none[k] for k in order], None) == 0


def test_tile_span_is_the_c_sides_span_limit():
    """``tile_span`` / ``LDS_SPAN_FLOATS`` / ``RS_TILE`` mirror rs_span_cap / RS_LDS_SPAN_FLOATS / RS_TILE of
    csrc/resample.hip: a launch of nothing (max_out = 0 returns after every check) is accepted exactly when Python says
    the pair fits, so ``check_fits`` never passes a pair the entries then refuse."""
    from cleanumamba_amd import hip
    from cleanumamba_amd.util import resample as rs
    lib = hip.lib()
    assert rs.RS_TILE == lib.cum_resample_tile()
    P = ctypes.c_void_p

    def accepted(up, down, K):
        rc = lib.cum_resample_ragged(1, P(0x1000), 1, 8, 8, P(0x2000), None, 1, up, down, 1, K, P(0x3000), -(-K // 4) * 4,
                                     P(0x4000), 0, 0, None)
        assert rc == 0 or (rc == -1 and b"LDS" in lib.cum_last_error()), (up, down, K, lib.cum_last_error())
        return rc == 0

    # just inside and just outside the limit of 12288 floats
    for triple, span in (((1, 14, 1500), 12256), ((1, 16, 1), 12296), ((3, 48, 1), 12296), ((1, 16, 219), 12512)):
        assert rs.tile_span(*triple) == span and accepted(*triple) == (span <= rs.LDS_SPAN_FLOATS), triple
    fits = 0
    for up in (1, 2, 3, 4, 80, 147, 160, 441, 1024):
        for down in (1, 2, 3, 6, 12, 14, 15, 16, 17, 48, 147, 160, 441, 1024):
            for K in (1, 7, 73, 219, 640, 1500, 3477):
                want = rs.tile_span(up, down, K) <= rs.LDS_SPAN_FLOATS
                assert accepted(up, down, K) == want, (up, down, K)
                fits += want
    assert 0 < fits < 882                                # the sweep has pairs on both sides


def test_plan_table_layout_and_the_c_checker_accepts_it():
    from cleanumamba_amd import hip
    from cleanumamba_amd.util import resample as rs
    lib = hip.lib()
    t = rs.PlanTable("cpu")
    assert t.args() == (None, None, 0, None, 0) and t.host is None and t.plans == []
    plans = [rs.plan(48000, 16000), rs.plan(16000, 44100), rs.plan(44100, 16000)]
    assert [t.add(p) for p in plans] == [0, 1, 2]
    assert t.plans == plans and t.host.dtype == torch.int32 and tuple(t.host.shape) == (3, rs.PLAN_INTS)
    off = 0
    for row, p in zip(t.host.tolist(), plans):
        assert row == [p.up, p.down, len(p.taps), p.K, p.pitch, off, 0, 0] and off % 4 == 0
        off += p.up * p.pitch
    assert torch.equal(t.dev, t.host) and t.blob.dtype == torch.float32
    assert torch.equal(t.blob, torch.cat([p.host_table().reshape(-1) for p in plans])) and t.blob.numel() == off
    before = t.host
    assert t.add(rs.plan(16000, 44100)) == 1 and len(t.plans) == 3 and t.host is before     # known: nothing is rebuilt
    host, dev, n, blob, floats = t.args()
    assert (host.value, dev.value, n, blob.value, floats) == (t.host.data_ptr(), t.dev.data_ptr(), 3, t.blob.data_ptr(), off)
    P = ctypes.c_void_p
    # no record: cum_resample_slots checks every plan row and the blob, and launches nothing
    rc = lib.cum_resample_slots(P(0x10000), 220, 4, host, dev, n, blob, floats, P(0x40000), P(0x50000), 0, None, 0, 0,
                                P(0x60000), 1, 8, None)
    assert rc == 0, lib.cum_last_error()
    rc = lib.cum_resample_slots(P(0x10000), 220, 4, host, dev, n, blob, floats - 1, P(0x40000), P(0x50000), 0, None, 0, 0,
                                P(0x60000), 1, 8, None)
    assert rc == -1 and b"blob" in lib.cum_last_error()


def test_the_pool_and_the_feeder_each_hold_one_plan_table(tmp_path):
    from cleanumamba_amd.util import resample as rs
    from cleanumamba_amd.training.feeder import BatchFeeder
    from test_feeder_rates_host import MIXED, MODEL, _dataset, _plan_only_feeder, mixed_tree
    from test_pool_rates_host import _net
    pool = _net("pruned500k").stream_pool(2)
    pool.open(1, rate=48000)
    assert isinstance(pool._rs, rs.PlanTable) and pool._rs.plans == [rs.plan(48000, 16000), rs.plan(16000, 48000)]
    mixed_tree(str(tmp_path), MIXED)
    rates = [r for r, _ in MIXED]
    assert isinstance(_plan_only_feeder(_dataset(str(tmp_path)), rates)._rs, rs.PlanTable)
    # the feeder's own registration, from the files' headers (its table on the host: nothing here touches a GPU)
    f = BatchFeeder.__new__(BatchFeeder)
    f.dataset, f.sample_rate, f.crop_length, f.device = _dataset(str(tmp_path)), MODEL, 4000, torch.device("cpu")
    f._read_rates(True)
    seen = list(dict.fromkeys(r for r in rates if r != MODEL))              # in the order the pairs bring them
    assert f._rs.plans == [rs.plan(r, MODEL) for r in seen] and tuple(f._rs.host.shape) == (len(seen), rs.PLAN_INTS)
    assert f._rs_ids == {MODEL: -1, **{r: i for i, r in enumerate(seen)}}
    # the records' 64-bit positions stand where both packers and the C side read them: ints 12-13 and 14-15
    assert (rs.REC_IN0, rs.REC_OUT0, rs.REC_INTS) == (12, 14, 16) and rs.REC_IN0 % 2 == rs.REC_OUT0 % 2 == 0


def test_host_tensors_are_refused():
    from cleanumamba_amd.util.resample import StreamResampler, resample_ragged
    with pytest.raises(RuntimeError, match="GPU"):
        resample_ragged(torch.zeros(1, 100), [100], 48000, 16000)
    with pytest.raises(RuntimeError, match="GPU"):
        StreamResampler(1, 48000, 16000, "cpu")
    with pytest.raises(ValueError):
        resample_ragged(torch.zeros(100), [100], 48000, 16000)


class _PastTheRateCheck(Exception):
    pass


def test_resample_switch_skips_the_rate_check(tmp_path, monkeypatch):
    """With ``resample=True`` a folder of mixed rates gets as far as loading the checkpoint; without it the ValueError of
    test_ragged_host.py stands."""
    from cleanumamba_amd.examples import denoise as D
    folder = tmp_path / "noisy"
    folder.mkdir()
    wavfile.write(str(folder / "a_16k.wav"), 16000, wavtree.pcm(300, 1))
    wavfile.write(str(folder / "b_8k.wav"), 8000, wavtree.pcm(100, 2))
    wavfile.write(str(folder / "c_48k.wav"), 48000, wavtree.pcm(100, 3))

    def marker(*a, **k):
        raise _PastTheRateCheck()
    monkeypatch.setattr(D, "load_pretrained_CleanUMamba", marker)
    with pytest.raises(_PastTheRateCheck):
        D.denoise("no_such_checkpoint.pkl", str(folder), str(tmp_path / "out"), resample=True)
    with pytest.raises(ValueError, match="b_8k.wav"):
        D.denoise("no_such_checkpoint.pkl", str(folder), str(tmp_path / "out"))
    with pytest.raises(ValueError):                      # a rate the resampler cannot reduce is named before any GPU work
        wavfile.write(str(folder / "d_odd.wav"), 16001, wavtree.pcm(100, 4))
        D.denoise("no_such_checkpoint.pkl", str(folder), str(tmp_path / "out"), resample=True)
