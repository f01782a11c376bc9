"""Extended speech metrics on the GPU (eSTOI, SI-SDR, SNR, cepstrum distance, fwSegSNR) against their f64 numpy
definitions in tests/metrics_ext_ref.py, on the clips of tests/golden/metrics.npz and three seeded speech-like pairs."""
import os
import warnings

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import metrics_ext_ref as R
from conftest import golden_json, load_ckpt, load_golden

pytestmark = pytest.mark.gpu

EXT = ("estoi", "si_sdr", "snr", "cep_dist", "fwsegSNR")


@pytest.fixture(scope="module")
def fx():
    """every input with the definition's frame series and clip values, computed once"""
    g = load_golden("metrics")
    clips = [(n, g[f"clean_{i}"], g[f"processed_{i}"]) for i, n in enumerate(golden_json(g["__names__"]))]
    clips += R.speech_like_pairs()
    out = []
    for name, c, p in clips:
        out.append(dict(name=name, clean=c, processed=p, cep=R.cep_frames(c, p), fwseg=R.fwseg_frames(c, p),
                        cep_dist=R.cep_dist(c, p), fwsegSNR=R.fwseg_snr(c, p)))
    return out


@pytest.fixture(autouse=True)
def _keep_pesq_warning_state():
    """python_eval warns once per process that pesq is missing; tests that run later still expect that warning"""
    from cleanumamba_amd.util import python_eval as PE
    was = PE._PESQ_WARNED
    yield
    PE._PESQ_WARNED = was


def _same(a, b):
    return torch.equal(a.nan_to_num(7.0, 8.0, 9.0), b.nan_to_num(7.0, 8.0, 9.0))


# ---------------------------------------------------------------- sums
def _sum_clips():
    rng = np.random.default_rng(11)
    rnd = lambda n: rng.integers(-32768, 32768, n).astype(np.int16)
    clips = [(rnd(n), rnd(n)) for n in (480, 481, 487, 488, 489)]       # the clip after 481 starts at an odd offset
    clips.append((rnd(8193), rnd(8193)))                                # one chunk + 1 sample
    clips.append((np.full(4099, -32768, np.int16), np.full(4099, -32768, np.int16)))
    clips.append((np.full(4099, 32767, np.int16), np.full(4099, -32768, np.int16)))
    clips.append((np.full(160000, -32768, np.int16), np.full(160000, -32768, np.int16)))   # full scale, 20 chunks
    clips.append((rnd(16391), rnd(16391)))                              # starts odd, ends mid-group in a third chunk
    return clips


def _np_sums(c, p):
    c, p = c.astype(np.int64), p.astype(np.int64)
    return [int(np.sum(c * c)), int(np.sum(p * p)), int(np.sum(c * p))]


def test_sums_are_exact_alone_and_in_a_ragged_batch(cuda):
    from cleanumamba_amd.util import metrics as M
    clips = _sum_clips()
    want = [_np_sums(c, p) for c, p in clips]
    b = M.Batch([c for c, _ in clips], [p for _, p in clips], 16000).upload()
    assert any(o % 2 == 1 for o in b.offsets) and any(o % 8 not in (0, 1) for o in b.offsets)
    got = M.clip_sums(b).cpu().tolist()
    assert got == want
    assert M.clip_sums(b).cpu().tolist() == want                        # rerun
    for (c, p), w in zip(clips, want):
        assert M.clip_sums(M.Batch([c], [p], 16000).upload()).cpu().tolist() == [w]
    # -32768 * -32768 pairs: what a packed 16-bit dot into int32 would overflow on
    assert want[6] == [4099 << 30, 4099 << 30, 4099 << 30] and want[8][0] == 160000 << 30


def test_si_sdr_and_snr_match_the_definition(cuda, fx):
    from cleanumamba_amd.util import metrics as M
    from cleanumamba_amd.util import python_eval as PE
    clips = [(f["clean"], f["processed"]) for f in fx] + _sum_clips()[:8]
    x = fx[0]["clean"]
    # silent clean (NaN), silent processed (si_sdr -inf), y = 3 x (si_sdr +inf: f64 gets Sxx Syy - Sxy^2 wrong there)
    clips += [(np.zeros(600, np.int16), x[:600]), (x[:600], np.zeros(600, np.int16)), (x[:4800] // 4, 3 * (x[:4800] // 4))]
    r = M.speech_metrics([c for c, _ in clips], [p for _, p in clips], rate=8000, metrics=("si_sdr", "snr"))
    assert list(r) == ["si_sdr", "snr"] and r["snr"].dtype == torch.float64 and r["snr"].is_cuda
    for i, (c, p) in enumerate(clips):
        for k, ref in (("si_sdr", R.si_sdr), ("snr", R.snr)):
            got, want = float(r[k][i]), ref(c, p)
            assert got == want or (np.isnan(got) and np.isnan(want)), (i, k, got, want)
    assert float(r["si_sdr"][-1]) == np.inf and np.isnan(float(r["snr"][-3])) and float(r["si_sdr"][-2]) == -np.inf
    assert PE.si_sdr(*clips[0]) == R.si_sdr(*clips[0])


# ---------------------------------------------------------------- eSTOI
@pytest.mark.parametrize("rate", [16000, 10000])
def test_estoi_matches_the_definition(cuda, fx, rate):
    """1e-5 is the project's STOI bound; the f32 band powers of the shared front end account for <= 3e-9 of it"""
    from cleanumamba_amd.util import metrics as M
    clips = [f for f in fx if f["clean"].size >= 4099]
    cl, pr = [f["clean"] for f in clips], [f["processed"] for f in clips]
    both = M.speech_metrics(cl, pr, rate=rate, metrics=("stoi", "estoi"))
    for f, g in zip(clips, both["estoi"].cpu().numpy()):
        want = R.estoi(f["clean"], f["processed"], rate)
        print(f["name"], rate, g, want, abs(g - want))
        assert abs(g - want) < 1e-5, (f["name"], rate, g, want)
    i4099 = [f["name"] for f in clips].index("len4099")
    if rate == 10000:                                       # 30 STFT frames: exactly one segment
        assert R.estoi(cl[i4099], pr[i4099], rate) > 1e-3
    else:
        assert float(both["estoi"][i4099]) == pytest.approx(1e-5, abs=1e-15)
    short = [f for f in fx if f["name"] == "len599"][0]
    assert M.stoi(short["clean"], short["processed"], rate, extended=True) == pytest.approx(1e-5, abs=1e-15)
    assert R.estoi(short["clean"], short["processed"], rate) == 1e-5
    assert M.stoi(cl[0], pr[0], rate, extended=True) == float(both["estoi"][0])
    # asked together = asked alone, bit for bit; STOI alone is cum_metrics_stoi itself
    assert _same(M.speech_metrics(cl, pr, rate=rate, metrics=("estoi",))["estoi"], both["estoi"])
    assert _same(M.speech_metrics(cl, pr, rate=rate, metrics=("stoi",))["stoi"], both["stoi"])
    assert _same(M._stoi(M.Batch(cl, pr, rate).upload(), 1)[0], both["stoi"])


# ---------------------------------------------------------------- cep / fwseg frames
def _check_frames(name, got_cep, got_fw, want_cep, want_fw):
    assert got_cep.shape == want_cep.shape == got_fw.shape == want_fw.shape, name
    assert np.array_equal(np.isnan(got_cep), np.isnan(want_cep)), name
    assert np.array_equal(np.isnan(got_fw), np.isnan(want_fw)), name
    ec = np.abs(got_cep - want_cep)[~np.isnan(want_cep)]
    ef = np.abs(got_fw - want_fw)[~np.isnan(want_fw)]
    print(name, "cep err", ec.max(initial=0), "fwseg err", ef.max(initial=0))
    assert ec.max(initial=0) < 1e-6, (name, ec.max())       # the LLR's bound; the definition's own f64 error is ~1e-11
    assert ef.max(initial=0) < 1e-3, (name, ef.max())       # the segSNR bound, dB


def test_cep_and_fwseg_frames_match_the_definition(cuda, fx):
    from cleanumamba_amd.util import metrics as M
    fm = M.frame_metrics([f["clean"] for f in fx], [f["processed"] for f in fx], extended=True)
    assert list(fm) == ["segSNR", "llr", "wss", "cep", "fwseg"]
    for i, f in enumerate(fx):
        _check_frames(f["name"], fm["cep"][i].cpu().numpy(), fm["fwseg"][i].cpu().numpy(), f["cep"], f["fwseg"])
    by = {f["name"]: i for i, f in enumerate(fx)}
    assert int(torch.isnan(fm["cep"][by["silences"]]).sum()) == 34 and fm["cep"][by["silences"]].numel() == 129
    assert torch.all(fm["cep"][by["identical"]] == 0) and torch.all(fm["fwseg"][by["identical"]] == 35)
    for k in ("cep", "fwseg"):                              # the limits hold and keep NaN
        v = torch.cat(fm[k])
        v = v[~torch.isnan(v)]
        lo, hi = (0.0, 10.0) if k == "cep" else (-10.0, 35.0)
        assert float(v.min()) >= lo and float(v.max()) <= hi


@pytest.mark.parametrize("length,frames", [(599, 0), (600, 1), (2400, 16), (2520, 17), (4440, 33)])
def test_frame_count_edges(cuda, fx, length, frames):
    """0, 1, 16, 17 and 33 frames: around the 16 frames of one workgroup"""
    from cleanumamba_amd.util import metrics as M
    from cleanumamba_amd.util import python_eval as PE
    f = [f for f in fx if f["name"] == "coloured_snr10"][0]
    c, p = f["clean"][1000:1000 + length], f["processed"][1000:1000 + length]
    cep, fw = PE.cepstrum_distance(c, p, 16000), PE.fwsegsnr(c, p, 16000)
    assert cep.shape == (frames,) and fw.shape == (frames,)
    _check_frames(str(length), cep, fw, R.cep_frames(c, p), R.fwseg_frames(c, p))
    r = M.speech_metrics([c], [p], metrics=("cep_dist", "fwsegSNR"))
    if frames == 0:
        assert torch.isnan(r["cep_dist"]).all() and torch.isnan(r["fwsegSNR"]).all()
    else:
        assert float(r["cep_dist"][0]) == pytest.approx(R.cep_dist(c, p), rel=1e-5)
        assert float(r["fwsegSNR"][0]) == pytest.approx(R.fwseg_snr(c, p), rel=1e-5)


# ---------------------------------------------------------------- per clip, batches, defaults
def test_clip_values_match_the_definition(cuda, fx):
    from cleanumamba_amd.util import metrics as M
    r = M.speech_metrics([f["clean"] for f in fx], [f["processed"] for f in fx], metrics=("fwsegSNR", "cep_dist"))
    assert list(r) == ["fwsegSNR", "cep_dist"]                        # in the order asked
    for k in r:
        got = r[k].cpu().numpy()
        for i, f in enumerate(fx):
            want = f[k]
            print(f["name"], k, got[i], want)
            if np.isnan(want):
                assert np.isnan(got[i]), (f["name"], k)
            else:
                assert abs(got[i] - want) <= 1e-5 * abs(want), (f["name"], k, got[i], want)


def test_extended_set_is_bitwise_per_clip_and_reproducible(cuda, fx):
    from cleanumamba_amd.util import metrics as M
    cl, pr = [f["clean"] for f in fx], [f["processed"] for f in fx]
    a = M.speech_metrics(cl, pr, metrics=EXT)
    b = M.speech_metrics(cl, pr, metrics=EXT)
    fa, fb = M.frame_metrics(cl, pr, extended=True), M.frame_metrics(cl, pr, extended=True)
    assert list(a) == list(EXT)
    for k in a:
        assert _same(a[k], b[k]), k
    for k in fa:
        for x, y in zip(fa[k], fb[k]):
            assert _same(x, y), k
    for i in range(len(fx)):
        one = M.speech_metrics([cl[i]], [pr[i]], metrics=EXT)
        for k in a:
            assert _same(one[k], a[k][i:i + 1]), (fx[i]["name"], k)
        f1 = M.frame_metrics([cl[i]], [pr[i]], extended=True)
        for k in ("cep", "fwseg"):
            assert _same(f1[k][0], fa[k][i]), (fx[i]["name"], k)


def test_defaults_are_unchanged(cuda, fx):
    from cleanumamba_amd.util import metrics as M
    from cleanumamba_amd.util import python_eval as PE
    cl, pr = [f["clean"] for f in fx[:2]], [f["processed"] for f in fx[:2]]
    assert tuple(M.speech_metrics(cl, pr)) == M.METRICS == ("wss_dist", "llr_mean", "segSNR", "stoi")
    assert list(M.frame_metrics(cl, pr)) == ["segSNR", "llr", "wss"]
    today = {"pesq_wb", "pesq_nb", "stoi", "CSIG", "CBAK", "COVL", "wss_dist", "segSNR", "llr_mean", "count"}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert set(PE.eval_waveform(cl[0], pr[0], 16000)) == today
        r = PE.eval_waveforms(cl, pr, 16000, extra=("snr", "estoi"))
    assert set(r[0]) == today | {"snr", "estoi"}
    assert r[1]["snr"] == pytest.approx(R.snr(cl[1], pr[1]) * cl[1].size, rel=1e-12)


def test_validate_with_extra_metrics(cuda, fx, tmp_path):
    from cleanumamba_amd.network import CleanUMamba
    from cleanumamba_amd.util.denoise_eval import KEYS, validate
    from cleanumamba_amd.util.python_eval import eval_waveforms
    sd, cfg = load_ckpt("442k")
    net = CleanUMamba(**cfg)
    net.load_state_dict(sd, strict=True)
    net = net.to(cuda)
    rng = np.random.default_rng(7)
    clean = [f["clean"][:16000] for f in fx[:3]]
    noisy = [np.clip(c + 1500 * rng.standard_normal(c.size), -32768, 32767).astype(np.int16) for c in clean]
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "clean"))
    os.makedirs(os.path.join(root, "noisy"))
    for i, (c, n) in enumerate(zip(clean, noisy)):
        wavfile.write(os.path.join(root, "clean", f"clean_fileid_{i}.wav"), 16000, c)
        wavfile.write(os.path.join(root, "noisy", f"book_{i:05d}_snr5_fileid_{i}.wav"), 16000, n)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = validate(net, root, extra_metrics=EXT)
        plain = validate(net, root)
        want = {}
        with torch.no_grad():
            for c, n in zip(clean, noisy):
                x = torch.from_numpy(n.astype(np.float32) / 32768.0)[None, None].to(cuda)
                y = (net(x) * 32767).clamp(-32768, 32767).to(torch.int16).squeeze().cpu().numpy()
                for k, v in eval_waveforms([c], [y], 16000, extra=EXT)[0].items():
                    want["Test/" + k] = want.get("Test/" + k, 0) + v
    assert set(plain) == {"Test/" + k for k in KEYS}
    assert set(res) == set(plain) | {"Test/" + k for k in EXT} == set(want)
    assert res["Test/count"] == 3 * 16000
    for k, v in want.items():
        if np.isnan(v):
            assert np.isnan(res[k]), k
        else:
            assert res[k] == pytest.approx(v, rel=1e-5), k
        if k in plain and not np.isnan(v):
            assert plain[k] == res[k], k
    for k in EXT:
        assert np.isfinite(res["Test/" + k]), k
