"""Speech metrics without a GPU: argument checks, the host-built tables, and the STOI restatement tests/stoi_ref.py."""
import ctypes

import numpy as np
import pytest

import stoi_ref


def voiced(n, rate=16000, f0=140.0, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    ph = 2 * np.pi * np.cumsum(f0 * (1 + 0.1 * np.sin(2 * np.pi * 0.7 * t))) / rate
    x = sum(np.sin(k * ph + rng.uniform(0, 2 * np.pi)) / k for k in range(1, 25))
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 3.1 * t)
    return 8000.0 * env * x / np.max(np.abs(x))


def test_argument_errors_raise_before_any_launch():
    from cleanumamba_amd.util import metrics as M
    x = np.zeros(16000, np.int16)
    with pytest.raises(ValueError, match="empty batch"):
        M.speech_metrics([], [])
    with pytest.raises(ValueError, match="clean has 16000 samples, processed 15999"):
        M.speech_metrics([x], [x[:-1]])
    with pytest.raises(ValueError, match="fewer than one 480-sample window"):
        M.speech_metrics([x, x[:479]], [x, x[:479]])
    with pytest.raises(ValueError, match="not supported"):
        M.speech_metrics([x], [x], rate=8000)
    with pytest.raises(ValueError, match="not supported"):
        M.speech_metrics([x], [x], rate=10000)                  # the frame metrics are 16 kHz only
    with pytest.raises(ValueError, match="not supported"):
        M.stoi(x, x, 22050)
    with pytest.raises(ValueError, match="int16 values"):
        M.speech_metrics([x + 0.5], [x])
    with pytest.raises(ValueError, match="unknown metric"):
        M.speech_metrics([x], [x], metrics=("pesq",))
    from cleanumamba_amd.util import python_eval as PE
    with pytest.raises(ValueError, match="same length"):
        PE.wss(x, x[:-1], 16000)
    with pytest.raises(ValueError, match="16 kHz"):
        PE.llr(x, x, 8000)


def test_c_entries_check_their_arguments():
    from cleanumamba_amd import hip
    L = hip.lib()
    arr = lambda *v: (ctypes.c_int64 * len(v))(*v)
    # bad arguments come back as CUM_EINVAL before anything touches a device pointer
    assert L.cum_metrics_frames(None, None, 1000, arr(0), arr(1000), 1, 8000, *([None] * 5), 0, None, None, None, 0,
                                None) == -1
    assert b"16 kHz" in L.cum_last_error()
    assert L.cum_metrics_frames(None, None, 1000, arr(0), arr(479), 1, 16000, *([None] * 5), 0, None, None, None, 0,
                                None) == -1
    assert b"fewer than one window" in L.cum_last_error()
    assert L.cum_metrics_frames(None, None, 1000, arr(600), arr(480), 1, 16000, *([None] * 5), 0, None, None, None, 0,
                                None) == -1
    assert b"outside the sample buffer" in L.cum_last_error()
    assert L.cum_metrics_frames(None, None, 0, arr(), arr(), 0, 16000, *([None] * 5), 0, None, None, None, 0, None) == -1
    assert L.cum_metrics_stoi(None, None, 1000, arr(0), arr(1000), 1, 44100, None, 0, None, None, None, None, 0, None,
                              None) == -1
    assert b"16000 or 10000" in L.cum_last_error()
    assert L.cum_metrics_clip_reduce(None, arr(1000), 1, 3, None, 0, None, None) == -1
    assert L.cum_metrics_frame_count(480) == 0 and L.cum_metrics_frame_count(599) == 0
    assert L.cum_metrics_frame_count(600) == 1 and L.cum_metrics_frame_count(160000) == 1329
    assert L.cum_metrics_frame_count(479) == -1
    for n in range(0, 400):                                    # Python's round: half to even
        assert L.cum_metrics_reduce_keep(n) == round(n * 0.95), n
    assert L.cum_metrics_stoi_workspace_bytes(arr(16000), 1, 8000) == -1


def test_critical_band_table():
    from cleanumamba_amd.util import metrics as M
    tab, w = M.crit_band_table()
    assert tab.shape == (25, 3) and tab.dtype == np.int32
    assert w.shape == (int(tab[:, 1].sum()),)
    assert np.array_equal(tab[:, 2], np.concatenate([[0], np.cumsum(tab[:-1, 1])]))
    assert tab[0, 0] == 0 and tab[:, 0].min() >= 0 and (tab[:, 0] + tab[:, 1]).max() <= 512
    assert np.all(np.diff(tab[:, 0]) >= 0) and np.all(tab[:, 1] >= 7) and tab[:, 1].max() < 40   # sparse supports
    min_factor = np.exp(-30.0 / (2.0 * 2.303))
    assert np.all(w > min_factor) and np.all(w <= 1.0)
    for b, (lo, n, o) in enumerate(tab):                      # each support peaks at floor of the centre bin
        f0 = int(np.floor(M.CRIT_CENTRE[b] / 8000 * 512))
        assert lo + int(np.argmax(w[o:o + n])) == f0
        assert w[o:o + n].max() == pytest.approx(M.CRIT_BANDWIDTH[0] / M.CRIT_BANDWIDTH[b])


def test_third_octave_table_and_resampler():
    from cleanumamba_amd.util import metrics as M
    bands = M.third_octave_table()
    assert bands.shape == (15, 2)
    assert bands[0].tolist() == [7, 9] and bands[-1].tolist() == [174, 219]
    assert np.all(bands[:, 1] > bands[:, 0]) and np.array_equal(bands[1:, 0], bands[:-1, 1])   # contiguous
    obm = stoi_ref.third_octave()
    for b, (lo, hi) in enumerate(bands):
        assert np.array_equal(np.nonzero(obm[b])[0], np.arange(lo, hi))
    h = M.resample_taps()
    assert h.shape == (581,) and h.sum() == pytest.approx(5.0) and np.allclose(h, h[::-1])
    assert np.allclose(h / 5, stoi_ref.resample_filter(10000, 16000), rtol=0, atol=1e-15)
    assert np.allclose(M.stoi_window(), np.hanning(258)[1:-1])


def test_stoi_ref_properties():
    x = voiced(32000)
    assert stoi_ref.stoi(x, x, 16000) == pytest.approx(1.0, abs=1e-12)
    assert stoi_ref.stoi(x, 3 * x, 16000) == pytest.approx(1.0, abs=1e-12)
    rng = np.random.default_rng(1)
    noise = rng.standard_normal(x.size) * np.std(x)
    scores = [stoi_ref.stoi(x, x + g * noise, 16000) for g in (0.05, 0.3, 1.0, 3.0)]
    assert all(a > b for a, b in zip(scores, scores[1:])), scores
    assert scores[0] > 0.9 and scores[-1] < 0.6
    assert abs(stoi_ref.stoi(x, rng.standard_normal(x.size), 16000)) < 0.1
    x10 = voiced(20000, rate=10000)
    assert stoi_ref.stoi(x10, x10, 10000) == pytest.approx(1.0, abs=1e-12)
    # 30 STFT frames need about 31 * 128 + 128 samples at 10 kHz: below that, 1e-5
    short = voiced(3500, rate=10000)
    assert stoi_ref.stoi(short, short, 10000) == 1e-5
