"""Extended speech metrics without a GPU: properties of the definitions (tests/metrics_ext_ref.py), the seeded inputs'
share of frames at a limit, argument checks of the Python surface and of the new C entries, header and bindings."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import metrics_ext_ref as R
from conftest import ROOT

NEW_ENTRIES = ("cum_metrics_sums", "cum_metrics_sums_workspace_bytes", "cum_metrics_frames_ext", "cum_metrics_stoi_ex",
               "cum_metrics_clip_nanmean")


@pytest.fixture(scope="module")
def pairs():
    return R.speech_like_pairs()


@pytest.fixture(scope="module")
def x():
    return R.q16(R.voiced(32000, np.random.default_rng(3)))


def test_estoi_properties(x):
    xf = x.astype(np.float64)
    assert R.estoi(x, x, 16000) == pytest.approx(1.0, abs=1e-12)
    assert R.estoi(xf, 3 * xf, 16000) == pytest.approx(1.0, abs=1e-12)
    rng = np.random.default_rng(1)
    noise = rng.standard_normal(x.size) * np.std(xf)
    scores = [R.estoi(xf, xf + g * noise, 16000) for g in (0.05, 0.3, 1.0, 3.0)]
    assert all(a > b for a, b in zip(scores, scores[1:])), scores
    x10 = R.voiced(20000, np.random.default_rng(4), rate=10000)
    assert R.estoi(x10, x10, 10000) == pytest.approx(1.0, abs=1e-12)
    short = R.voiced(3500, np.random.default_rng(5), rate=10000)
    assert R.estoi(short, short, 10000) == 1e-5              # fewer than 30 STFT frames, as STOI


def test_cep_and_fwseg_of_identical_clips(x):
    c = x[:4440]
    assert np.all(R.cep_frames(c, c) == 0.0)
    assert np.all(R.fwseg_frames(c, c) == 35.0)
    z = np.zeros(1200, np.int16)
    assert np.isnan(R.cep_frames(z, c[:1200])).all() and np.isnan(R.cep_frames(c[:1200], z)).all()
    assert np.isnan(R.fwseg_frames(z, c[:1200])).all()       # silent clean frame: NaN
    quiet = R.fwseg_frames(c[:1200], z)                       # silent processed frame: near 0 dB, not NaN
    assert np.all(np.abs(quiet) < 1e-6)


def test_si_sdr_and_snr_properties(x):
    rng = np.random.default_rng(2)
    c = x[:8000]
    y = R.q16(c * 0.4 + 300 * rng.standard_normal(c.size))
    assert R.si_sdr(c, 2 * y.astype(np.int64)) == R.si_sdr(c, y)            # exactly scale invariant
    assert R.si_sdr(c, 3 * c.astype(np.int64)) == math.inf                  # f64 gets Sxx Syy - Sxy^2 wrong here
    z = np.zeros_like(c)
    assert math.isnan(R.si_sdr(z, c)) and math.isnan(R.snr(z, c))
    assert R.si_sdr(c, z) == -math.inf
    assert R.snr(c, c) == math.inf
    cf = c.astype(np.float64)
    n = rng.standard_normal(c.size)
    n = np.round(n * np.sqrt(np.mean(cf ** 2) / np.mean(n ** 2) / 10 ** 1.2))   # integer noise 12 dB down
    want = 10 * np.log10(np.sum(cf ** 2) / np.sum(n ** 2))
    assert R.snr(c, (cf + n).astype(np.int64)) == pytest.approx(want, abs=1e-9)
    assert abs(want - 12.0) < 0.01
    from cleanumamba_amd.util import metrics as M                           # the host half of the GPU path
    for a, b in ((c, y), (c, 3 * c.astype(np.int64)), (z, c), (c, z), (c, c)):
        s = R.sums(a, b)
        for got, ref in ((M.si_sdr_from_sums(*s), R.si_sdr(a, b)), (M.snr_from_sums(*s), R.snr(a, b))):
            assert got == ref or (math.isnan(got) and math.isnan(ref))


def test_seeded_pairs_are_not_clamped(pairs):
    """at most 5 % of the frames of either series sit at a limit, so the GPU comparison cannot pass on clamped values"""
    assert [p[0] for p in pairs] == ["coloured_snr10", "coloured_snr25", "tilt"]
    for name, c, p in pairs:
        assert c.size == p.size == 24000 and c.dtype == p.dtype == np.int16
        cep, fw = R.cep_frames(c, p), R.fwseg_frames(c, p)
        assert cep.size == fw.size == 196 and not np.isnan(cep).any() and not np.isnan(fw).any()
        assert np.mean((cep <= 0.0) | (cep >= 10.0)) <= 0.05, name
        assert np.mean((fw <= -10.0) | (fw >= 35.0)) <= 0.05, name


def test_argument_errors_raise_before_any_launch():
    from cleanumamba_amd.util import metrics as M
    from cleanumamba_amd.util import python_eval as PE
    assert M.METRICS == ("wss_dist", "llr_mean", "segSNR", "stoi")
    assert M.EXT_METRICS == ("estoi", "si_sdr", "snr", "cep_dist", "fwsegSNR")
    x = np.zeros(16000, np.int16)
    with pytest.raises(ValueError, match="unknown metric"):
        M.speech_metrics([x], [x], metrics=("pesq",))
    with pytest.raises(ValueError, match="unknown metric"):
        M.speech_metrics([x], [x], metrics=("si_sdr", "sdr"))
    with pytest.raises(ValueError, match="not supported"):
        M.speech_metrics([x], [x], rate=22050, metrics=("estoi",))
    with pytest.raises(ValueError, match="not supported"):
        M.stoi(x, x, 22050, extended=True)
    with pytest.raises(ValueError, match="not supported"):
        M.speech_metrics([x], [x], rate=10000, metrics=("cep_dist",))
    with pytest.raises(ValueError, match="not supported"):
        M.speech_metrics([x], [x], rate=10000, metrics=("estoi", "fwsegSNR"))
    with pytest.raises(ValueError, match="not supported"):
        M.speech_metrics([x], [x], rate=0, metrics=("si_sdr",))
    with pytest.raises(ValueError, match="16 kHz"):
        PE.cepstrum_distance(x, x, 8000)
    with pytest.raises(ValueError, match="16 kHz"):
        PE.fwsegsnr(x, x, 10000)
    with pytest.raises(ValueError, match="same length"):
        PE.si_sdr(x, x[:-1])
    with pytest.raises(ValueError, match="unknown extra metric"):
        PE.eval_waveforms([x], [x], 16000, extra=("pesq",))
    from cleanumamba_amd.util.denoise_eval import validate
    with pytest.raises(ValueError, match="unknown extra metric"):
        validate(None, "/nonexistent", extra_metrics=("stoi",))
    # si_sdr at 8 kHz passes every argument check: what stops it here is the missing GPU (there it runs)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            M.speech_metrics([x], [x], rate=8000, metrics=("si_sdr", "snr"))


def test_new_c_entries_check_their_arguments():
    from cleanumamba_amd import hip
    L = hip.lib()
    arr = lambda *v: (ctypes.c_int64 * len(v))(*v)
    ext = lambda n, off, ln, k, rate: L.cum_metrics_frames_ext(None, None, n, off, ln, k, rate, *([None] * 5), 0, None,
                                                                None, 0, None)
    assert ext(1000, arr(0), arr(1000), 1, 8000) == -1
    assert b"16 kHz" in L.cum_last_error()
    assert ext(1000, arr(0), arr(479), 1, 16000) == -1
    assert b"fewer than one window" in L.cum_last_error()
    assert ext(1000, arr(600), arr(480), 1, 16000) == -1
    assert b"outside the sample buffer" in L.cum_last_error()
    assert ext(0, arr(), arr(), 0, 16000) == -1
    assert b"1 to 65535 clips" in L.cum_last_error()

    stoi = lambda n, off, ln, k, rate, which: L.cum_metrics_stoi_ex(None, None, n, off, ln, k, rate, None, 0, None, None,
                                                                     None, None, 0, which, None, None, None)
    assert stoi(1000, arr(0), arr(1000), 1, 44100, 3) == -1
    assert b"16000 or 10000" in L.cum_last_error()
    assert stoi(1000, arr(0), arr(0), 1, 16000, 3) == -1
    assert b"fewer than one window" in L.cum_last_error()
    assert stoi(1000, arr(990), arr(20), 1, 10000, 2) == -1
    assert b"outside the sample buffer" in L.cum_last_error()
    assert stoi(0, arr(), arr(), 0, 16000, 2) == -1
    assert b"1 to 65535 clips" in L.cum_last_error()
    assert stoi(1000, arr(0), arr(1000), 1, 16000, 0) == -1 and stoi(1000, arr(0), arr(1000), 1, 16000, 4) == -1
    assert b"which is 1" in L.cum_last_error()

    sums = lambda n, off, ln, k: L.cum_metrics_sums(None, None, n, off, ln, k, None, 0, None, None)
    assert sums(1000, arr(0), arr(0), 1) == -1
    assert b"fewer than one window" in L.cum_last_error()
    assert sums(1000, arr(999), arr(2), 1) == -1
    assert b"outside the sample buffer" in L.cum_last_error()
    assert sums(1000, arr(-1), arr(2), 1) == -1
    assert sums(0, arr(), arr(), 0) == -1
    assert b"1 to 65535 clips" in L.cum_last_error()
    assert L.cum_metrics_sums_workspace_bytes(arr(), 0) == -1
    # rows + three int64 per 8192-sample chunk; a start that is not 16-byte aligned can cost a chunk more
    assert L.cum_metrics_sums_workspace_bytes(arr(8185, 8186, 480), 3) == 3 * 64 + (1 + 2 + 1) * 24

    assert L.cum_metrics_clip_nanmean(None, arr(479), 1, None, 0, None, None) == -1
    assert b"shorter than one window" in L.cum_last_error()
    assert L.cum_metrics_clip_nanmean(None, arr(), 0, None, 0, None, None) == -1
    assert L.cum_metrics_clip_reduce(None, arr(1000), 1, 3, None, 0, None, None) == -1     # modes stay 0, 1, 2


def test_header_and_bindings_carry_the_new_symbols():
    from cleanumamba_amd import hip
    text = open(os.path.join(ROOT, "include", "cleanumamba_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = hip.lib()
    for s in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % s, code), s
        assert s in hip.SIGNATURES and hasattr(lib, s), s
    assert "#define CUM_ABI_VERSION 16" in text and lib.cum_abi_version() == 16
