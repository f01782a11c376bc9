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
