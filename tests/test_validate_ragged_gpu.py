"""``validate(batching="ragged")`` (util/denoise_eval.py) and ``denoise(pcm16=True)`` (examples/denoise.py) on the GPU:
the route that keeps the audio on the device from the files to the scores, against the ``"length"`` route, the host
scoring route ``eval_waveforms`` and the f64 oracle on every clip alone.

Measured on an MI355X (442k checkpoint, f32, the eight 16 kHz pairs below; R the ragged route's int16, A the length
route's, Oq the quantised f64 oracle; 73 004 samples): count(A != Oq) = 3, count(R != Oq) = 5, |R - A| <= 1 everywhere;
the per-key differences of the two dicts this file prints are in DESIGN.md 7f "Validation on the device"."""
import os
import warnings

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import pcm16_ref as P
from conftest import load_ckpt, record
from oracle import cleanumamba_ref as R

pytestmark = pytest.mark.gpu
EXTRA = ("estoi", "si_sdr")
LENGTHS_16K = [6400, 7013, 7999, 8640, 9601, 10240, 11111, 12000]
LENGTHS_CROP = [12000, 15000, 18001, 21000, 24000, 17000]          # ``crop=1`` cuts four of the six
LENGTHS_48K = [19200, 24001, 30000, 36000]


def _pair(rng, n, rate):
    """(clean, noisy) int16: band-limited noise bursts (300 Hz - 3.4 kHz, an envelope that never closes) and the same
    plus white noise -- loud enough that no frame is silent."""
    spec = np.fft.rfft(rng.standard_normal(n))
    f = np.fft.rfftfreq(n, 1.0 / rate)
    spec[(f < 300) | (f > 3400)] = 0
    x = np.fft.irfft(spec, n)
    x /= np.abs(x).max()
    seg = max(1, rate // 10)
    env = np.repeat(rng.choice([0.15, 1.0], size=n // seg + 1), seg)[:n]
    clean = np.round(9000 * env * x)
    noisy = np.clip(np.round(clean + 1200 * rng.standard_normal(n)), -32768, 32767)
    return clean.astype(np.int16), noisy.astype(np.int16)


def _write(root, lengths, rate, seed):
    os.makedirs(os.path.join(root, "clean"))
    os.makedirs(os.path.join(root, "noisy"))
    rng = np.random.default_rng(seed)
    for i, n in enumerate(lengths):
        c, nz = _pair(rng, n, rate)
        wavfile.write(os.path.join(root, "clean", f"p{i:03d}.wav"), rate, c)
        wavfile.write(os.path.join(root, "noisy", f"p{i:03d}.wav"), rate, nz)
    return root


@pytest.fixture(scope="module")
def model(cuda):
    from cleanumamba_amd.network import CleanUMamba
    sd, cfg = load_ckpt("442k")
    net = CleanUMamba(**cfg)
    net.load_state_dict(sd, strict=True)
    return net.to(cuda).float().eval(), {k: v.double() for k, v in sd.items()}


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    root = tmp_path_factory.mktemp("validate_ragged")
    return {"16k": _write(str(root / "at16k"), LENGTHS_16K, 16000, 1), "crop": _write(str(root / "crop"), LENGTHS_CROP, 16000, 2),
            "48k": _write(str(root / "at48k"), LENGTHS_48K, 48000, 3)}


def _both_routes(net, root, monkeypatch, **kw):
    """validate on both routes with what each handed to its scorer: (dict, clean int16 clips, processed int16 clips)."""
    from cleanumamba_amd.util import denoise_eval, python_eval
    seen = {}
    real_w, real_b = python_eval.eval_waveforms, python_eval.eval_batch

    def spy_w(cleans, targets, rate, extra=()):
        seen.setdefault("length", ([], []))
        seen["length"][0].extend(np.asarray(c) for c in cleans)
        seen["length"][1].extend(np.asarray(t) for t in targets)
        return real_w(cleans, targets, rate, extra=extra)

    def spy_b(batch, rate, extra=()):
        c, p = batch.clean.cpu().numpy(), batch.processed.cpu().numpy()
        seen.setdefault("ragged", ([], []))
        for o, n in zip(batch.offsets.tolist(), batch.lengths.tolist()):
            seen["ragged"][0].append(c[o:o + n])
            seen["ragged"][1].append(p[o:o + n])
        return real_b(batch, rate, extra=extra)
    monkeypatch.setattr(denoise_eval, "eval_waveforms", spy_w)
    monkeypatch.setattr(python_eval, "eval_batch", spy_b)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = denoise_eval.validate(net, root, VCTK_DEMAND=True, extra_metrics=EXTRA, **kw)
        r = denoise_eval.validate(net, root, VCTK_DEMAND=True, extra_metrics=EXTRA, batching="ragged", **kw)
    monkeypatch.undo()
    return (a,) + seen["length"], (r,) + seen["ragged"]


def _host_sums(cleans, targets, rate):
    """The dict ``validate`` builds, from the existing host scoring route."""
    from cleanumamba_amd.util.denoise_eval import KEYS
    from cleanumamba_amd.util.python_eval import eval_waveforms
    result = {"Test/" + k: 0 for k in KEYS + EXTRA}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for r in eval_waveforms(cleans, targets, rate, extra=EXTRA):
            for k in r:
                result["Test/" + k] += r[k]
    return result


def _same_dict(got, want):
    assert set(got) == set(want)
    for k in want:
        assert np.array_equal(np.float64(got[k]), np.float64(want[k]), equal_nan=True), (k, got[k], want[k])


def _files(root):
    """The pairs in validate's order: (clean int16 arrays, noisy int16 arrays)."""
    from cleanumamba_amd.util.denoise_eval import _pairs
    pairs = _pairs(root, True, True, 1.0)
    return [wavfile.read(c)[1] for c, _ in pairs], [wavfile.read(n)[1] for _, n in pairs]


def test_ragged_route_against_length_route_host_scoring_and_f64_oracle(cuda, model, sets, monkeypatch):
    net, sd64 = model
    (a, a_clean, A), (r, r_clean, Rq) = _both_routes(net, sets["16k"], monkeypatch)
    # 1. keys and count
    assert set(r) == set(a) and r["Test/count"] == a["Test/count"] == sum(LENGTHS_16K)
    assert all(np.isfinite(r["Test/" + k]) for k in ("stoi", "segSNR", "wss_dist", "llr_mean") + EXTRA)
    # 2. the scoring plumbing is exact: the int16 clips of denoise_batch_pcm16 through the host route give the same sums
    cleans, noisy = _files(sets["16k"])
    with torch.no_grad():
        flat, offsets, lens = net.denoise_batch_pcm16([torch.from_numpy(n) for n in noisy], mode=0)
    flat = flat.cpu().numpy()
    targets = [flat[o:o + n] for o, n in zip(offsets.tolist(), lens.tolist())]
    assert all(np.array_equal(t, q) for t, q in zip(targets, Rq)) and all(np.array_equal(c, q) for c, q in zip(cleans, r_clean))
    _same_dict(r, _host_sums(cleans, targets, 16000))
    # 3. the denoise plumbing against the f64 oracle on every clip alone
    diff_r = diff_a = 0
    for nz, qa, qr in zip(noisy, A, Rq):
        x = torch.from_numpy(nz.astype(np.float32) / np.float32(32768.0))
        with torch.no_grad():
            ref = R.forward_ref(sd64, x.double().view(1, 1, -1))[0, 0]
        oq = P.quantise(ref.float().numpy(), 0)
        assert int(np.abs(qr.astype(np.int32) - qa.astype(np.int32)).max()) <= 1
        diff_r += int(np.count_nonzero(qr != oq))
        diff_a += int(np.count_nonzero(qa != oq))
    record("validate_ragged_ne_oracle", diff_r)
    record("validate_length_ne_oracle", diff_a)
    print("samples", sum(LENGTHS_16K), "R != Oq", diff_r, "A != Oq", diff_a)
    for k in sorted(a):
        record("validate_ragged_minus_length[%s]" % k, np.float64(r[k]) - np.float64(a[k]))
        print(k, "ragged", r[k], "length", a[k], "difference", np.float64(r[k]) - np.float64(a[k]))
    assert diff_a > 0, "the length route equals the quantised oracle everywhere: the inputs test nothing"
    assert diff_r <= 2 * diff_a, (diff_r, diff_a)


def test_crop_scores_the_cropped_clips_where_they_stand(cuda, model, sets, monkeypatch):
    net, _ = model
    (a, _, _), (r, r_clean, Rq) = _both_routes(net, sets["crop"], monkeypatch, crop=1)
    want_count = sum(min(n, 16000) for n in LENGTHS_CROP)
    assert set(r) == set(a) and r["Test/count"] == a["Test/count"] == want_count
    assert sum(n > 16000 for n in LENGTHS_CROP) >= len(LENGTHS_CROP) // 2
    cleans, noisy = _files(sets["crop"])
    with torch.no_grad():
        flat, offsets, lens = net.denoise_batch_pcm16([torch.from_numpy(n) for n in noisy], mode=0)
    flat = flat.cpu().numpy()
    targets = [flat[o:o + n][:16000] for o, n in zip(offsets.tolist(), lens.tolist())]
    cleans = [c[:16000] for c in cleans]
    assert all(np.array_equal(t, q) for t, q in zip(targets, Rq)) and all(np.array_equal(c, q) for c, q in zip(cleans, r_clean))
    _same_dict(r, _host_sums(cleans, targets, 16000))


def test_48k_set_is_converted_and_quantised_on_the_device(cuda, model, sets, monkeypatch):
    net, _ = model
    (a, a_clean, A), (r, r_clean, Rq) = _both_routes(net, sets["48k"], monkeypatch, resample=True)
    want = [-(-c.size // 3) for c in _files(sets["48k"])[0]]          # in validate's order (the folder listing's)
    assert sorted(want) == sorted(-(-n // 3) for n in LENGTHS_48K)
    assert [c.size for c in r_clean] == [c.size for c in a_clean] == want
    assert set(r) == set(a) and r["Test/count"] == a["Test/count"] == sum(want)
    for i, (ca, cr) in enumerate(zip(a_clean, r_clean)):       # the converted clean signal: the same bits on both routes
        assert ca.dtype == np.int16 and cr.dtype == np.int16 and np.array_equal(ca, cr), i
        assert int(np.abs(cr.astype(np.int32)).max()) > 1000
    for qa, qr in zip(A, Rq):
        assert int(np.abs(qr.astype(np.int32) - qa.astype(np.int32)).max()) <= 1
    _same_dict(r, _host_sums(r_clean, Rq, 16000))


def test_folder_cli_writes_int16(cuda, sets, tmp_path):
    from cleanumamba_amd.examples.denoise import denoise
    sd, cfg = load_ckpt("442k")
    ckpt = str(tmp_path / "model.pkl")
    torch.save({"network_config": cfg, "model_state_dict": sd}, ckpt)
    for name, rate, count, kw in (("16k", 16000, 3, {}), ("48k", 48000, 1, {"resample": True})):
        src = os.path.join(sets[name], "noisy")
        folder = tmp_path / ("in_" + name)
        folder.mkdir()
        files = sorted(os.listdir(src))[:count]
        for f in files:
            wavfile.write(str(folder / f), rate, wavfile.read(os.path.join(src, f))[1])
        _, as_float = denoise(ckpt, str(folder), None, **kw)
        out = str(tmp_path / ("out_" + name))
        _, as_pcm = denoise(ckpt, str(folder), out, pcm16=True, **kw)
        for f, y, q in zip(files, as_float, as_pcm):
            got_rate, w = wavfile.read(os.path.join(out, "enhanced_" + f))
            n = wavfile.read(str(folder / f))[1].size
            assert got_rate == rate and w.dtype == np.int16 and w.shape == (n,) and y.dtype == np.float32
            assert np.array_equal(w, q) and np.array_equal(w, P.quantise(y, 1)), f
            assert w.min() < 0 < w.max()                       # a signal, not a constant: the equalities above say something
