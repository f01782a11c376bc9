"""Speech metrics on the GPU against the reference's own outputs (tests/golden/metrics.npz, tools/make_golden_metrics.py)
and the STOI restatement tests/stoi_ref.py."""
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import stoi_ref
from conftest import golden_json, load_ckpt, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    g = load_golden("metrics")
    names = golden_json(g["__names__"])
    return [dict(name=n, clean=g[f"clean_{i}"], processed=g[f"processed_{i}"], wss=g[f"wss_{i}"], llr=g[f"llr_{i}"],
                 snr=g[f"snr_{i}"], clip=g[f"clip_{i}"]) for i, n in enumerate(names)]


def test_frame_metrics_match_reference(cuda, fx):
    from cleanumamba_amd.util import metrics as M
    fm = M.frame_metrics([f["clean"] for f in fx], [f["processed"] for f in fx])
    for i, f in enumerate(fx):
        snr, llr, wss = (fm[k][i].cpu().numpy() for k in ("segSNR", "llr", "wss"))
        assert snr.shape == f["snr"].shape == llr.shape == wss.shape, f["name"]
        if snr.size == 0:
            continue
        assert np.max(np.abs(snr - f["snr"])) < 1e-3, f["name"]
        assert np.array_equal(np.isnan(llr), np.isnan(f["llr"])), f["name"]
        fin = ~np.isnan(f["llr"])
        assert np.max(np.abs(llr[fin] - f["llr"][fin]), initial=0) < 1e-6, f["name"]
        err = np.abs(wss - f["wss"])
        bad = err > np.maximum(1e-4 * np.abs(f["wss"]), 1e-4)
        assert not bad.any(), (f["name"], np.nonzero(bad)[0], wss[bad], f["wss"][bad])
    ident = [i for i, f in enumerate(fx) if f["name"] == "identical"][0]
    assert torch.all(fm["wss"][ident] == 0) and torch.all(fm["llr"][ident] == 0)


def test_clip_metrics_match_reference(cuda, fx):
    from cleanumamba_amd.util import metrics as M
    r = M.speech_metrics([f["clean"] for f in fx], [f["processed"] for f in fx], metrics=("wss_dist", "llr_mean", "segSNR"))
    got = torch.stack([r["wss_dist"], r["llr_mean"], r["segSNR"]], 1).cpu().numpy()
    for i, f in enumerate(fx):
        want = f["clip"]
        assert np.array_equal(np.isnan(got[i]), np.isnan(want)), f["name"]
        ok = ~np.isnan(want)
        assert np.all(np.abs(got[i][ok] - want[ok]) <= 1e-5 * np.maximum(np.abs(want[ok]), 1e-12) + 1e-12), \
            (f["name"], got[i], want)


def test_python_eval_mirror(cuda, fx):
    from cleanumamba_amd.util import python_eval as PE
    f = fx[1]
    assert np.allclose(PE.wss(f["clean"], f["processed"], 16000), f["wss"], rtol=1e-4, atol=1e-4)
    _, seg = PE.snr(f["clean"], f["processed"], 16000)
    assert np.allclose(seg, f["snr"], rtol=0, atol=1e-3)
    with pytest.warns(UserWarning, match="pesq") if not _has_pesq() else _nullcontext():
        r = PE.eval_waveform(f["clean"], f["processed"], 16000)
    n = f["clean"].size
    assert r["count"] == n
    assert r["wss_dist"] / n == pytest.approx(f["clip"][0], rel=1e-5)
    assert r["llr_mean"] / n == pytest.approx(f["clip"][1], rel=1e-5)
    assert r["segSNR"] / n == pytest.approx(f["clip"][2], rel=1e-5)
    if not _has_pesq():
        assert all(np.isnan(r[k]) for k in ("pesq_wb", "pesq_nb", "CSIG", "CBAK", "COVL"))


def _has_pesq():
    try:
        import pesq  # noqa: F401
        return True
    except ImportError:
        return False


class _nullcontext:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


@pytest.mark.parametrize("rate", [16000, 10000])
def test_stoi_matches_restatement(cuda, fx, rate):
    from cleanumamba_amd.util import metrics as M
    clips = [f for f in fx if f["clean"].size >= 16000]
    got = M.speech_metrics([f["clean"] for f in clips], [f["processed"] for f in clips], rate=rate,
                           metrics=("stoi",))["stoi"].cpu().numpy()
    for f, g in zip(clips, got):
        want = stoi_ref.stoi(f["clean"], f["processed"], rate)
        assert abs(g - want) < 1e-5, (f["name"], rate, g, want)
    # a clip too short for 30 STFT frames at either rate
    short = [f for f in fx if f["name"] == "len599"][0]
    assert M.stoi(short["clean"], short["processed"], rate) == pytest.approx(1e-5)
    assert stoi_ref.stoi(short["clean"], short["processed"], rate) == 1e-5


def test_ragged_batch_is_bitwise_per_clip_and_reproducible(cuda, fx):
    from cleanumamba_amd.util import metrics as M
    cl, pr = [f["clean"] for f in fx], [f["processed"] for f in fx]
    a = M.speech_metrics(cl, pr)
    b = M.speech_metrics(cl, pr)
    fa, fb = M.frame_metrics(cl, pr), M.frame_metrics(cl, pr)
    for k in a:
        assert torch.equal(a[k].nan_to_num(7.0), b[k].nan_to_num(7.0)), k
    for k in fa:
        for x, y in zip(fa[k], fb[k]):
            assert torch.equal(x.nan_to_num(7.0), y.nan_to_num(7.0)), k
    for i in range(len(fx)):
        one = M.speech_metrics([cl[i]], [pr[i]])
        for k in a:
            assert torch.equal(one[k].nan_to_num(7.0), a[k][i:i + 1].nan_to_num(7.0)), (fx[i]["name"], k)
        f1 = M.frame_metrics([cl[i]], [pr[i]])
        for k in fa:
            assert torch.equal(f1[k][0].nan_to_num(7.0), fa[k][i].nan_to_num(7.0)), (fx[i]["name"], k)


def _write_dns(root, clips, noisy):
    os.makedirs(os.path.join(root, "clean"))
    os.makedirs(os.path.join(root, "noisy"))
    for i, (c, n) in enumerate(zip(clips, noisy)):
        wavfile.write(os.path.join(root, "clean", f"clean_fileid_{i}.wav"), 16000, c)
        wavfile.write(os.path.join(root, "noisy", f"book_{i:05d}_snr5_fileid_{i}.wav"), 16000, n)


def test_validate_matches_per_clip_forward(cuda, fx, tmp_path):
    from cleanumamba_amd.network import CleanUMamba
    from cleanumamba_amd.util.denoise_eval import validate
    from cleanumamba_amd.util.python_eval import eval_waveform
    sd, cfg = load_ckpt("442k")
    net = CleanUMamba(**cfg)
    net.load_state_dict(sd, strict=True)
    net = net.to(cuda)
    rng = np.random.default_rng(7)
    clean = [f["clean"][:16000] for f in fx[:3]]
    noisy = [np.clip(c + 1500 * rng.standard_normal(c.size), -32768, 32767).astype(np.int16) for c in clean]
    _write_dns(str(tmp_path), clean, noisy)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = validate(net, str(tmp_path))
        want = {}
        with torch.no_grad():
            for c, n in zip(clean, noisy):
                x = torch.from_numpy(n.astype(np.float32) / 32768.0)[None, None].to(cuda)
                y = (net(x) * 32767).clamp(-32768, 32767).to(torch.int16).squeeze().cpu().numpy()
                for k, v in eval_waveform(c, y, 16000).items():
                    want["Test/" + k] = want.get("Test/" + k, 0) + v
    assert res["Test/count"] == 3 * 16000
    for k, v in want.items():
        if np.isnan(v):
            assert np.isnan(res[k]), k
        else:
            assert res[k] == pytest.approx(v, rel=1e-5), k
    if not _has_pesq():
        assert all(np.isnan(res["Test/" + k]) for k in ("pesq_wb", "pesq_nb", "CSIG", "CBAK", "COVL"))
