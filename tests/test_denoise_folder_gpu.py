"""examples/denoise.py on a folder of int16 mono files of mixed lengths (GPU): the interface of the reference's
src/examples/denoise.py:14-72 -- ``enhanced_<name>`` float32 WAV files and the two returned lists -- on the ragged route,
and the ``denoise_long`` route for a file over the sample budget."""
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from conftest import load_ckpt, rel_l2

pytestmark = pytest.mark.gpu
E2E_TOL = 1e-4                                            # the bound test_block_denoise_gpu.py uses for block == forward
LENGTHS = [300, 766, 767, 1500, 2047, 1022, 1023]


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    root = tmp_path_factory.mktemp("denoise_folder")
    sd, cfg = load_ckpt("442k")
    ckpt = str(root / "model.pkl")
    torch.save({"network_config": cfg, "model_state_dict": sd}, ckpt)
    noisy = root / "noisy"
    noisy.mkdir()
    rng = np.random.default_rng(0)
    files = {}
    for k, n in enumerate(LENGTHS):
        x = np.clip(np.round(3000 * rng.standard_normal(n) + 500), -32768, 32767).astype(np.int16)
        name = f"clip_{k:02d}_{n}.wav"
        wavfile.write(str(noisy / name), 16000, x)
        files[name] = x
    return ckpt, str(noisy), files, root


def test_folder_outputs_equal_denoise_batch(cuda, folder):
    from cleanumamba_amd.examples.denoise import denoise
    from cleanumamba_amd.examples.loading_pretrained_models import load_pretrained_CleanUMamba
    ckpt, noisy_dir, files, root = folder
    out_dir = str(root / "enhanced")
    noisy, cleaned = denoise(ckpt, noisy_dir, out_dir)
    names = sorted(files)
    assert sorted(os.listdir(out_dir)) == ["enhanced_" + n for n in names]
    model = load_pretrained_CleanUMamba(ckpt).eval()
    assert next(model.parameters()).is_cuda and next(model.parameters()).dtype == torch.float32
    with torch.no_grad():
        want = model.denoise_batch([torch.from_numpy(files[n]) for n in names])
    assert len(noisy) == len(cleaned) == len(names)
    for k, n in enumerate(names):
        rate, y = wavfile.read(os.path.join(out_dir, "enhanced_" + n))
        assert rate == 16000 and y.dtype == np.float32 and y.shape == files[n].shape
        assert np.array_equal(y, cleaned[k]) and cleaned[k].dtype == np.float32
        assert np.array_equal(y, want[k].cpu().numpy()), n
        assert noisy[k].dtype == np.float32 and np.array_equal(noisy[k], files[n].astype(np.float32) / np.float32(32768.0))
    # nothing is written without an output directory; the lists are the same
    again = denoise(ckpt, noisy_dir, None, max_batch=3)
    assert sorted(os.listdir(str(root))) == ["enhanced", "model.pkl", "noisy"]
    with torch.no_grad():
        for k, n in enumerate(names):
            x = torch.from_numpy(files[n].astype(np.float32) / np.float32(32768.0)).to(cuda)
            lone = model(x.view(1, 1, -1))[0, 0]
            assert rel_l2(again[1][k], lone) < E2E_TOL and rel_l2(cleaned[k], lone) < E2E_TOL, n


def test_a_file_over_the_budget_takes_the_block_route(cuda, folder, monkeypatch):
    from cleanumamba_amd.examples import denoise as D
    from cleanumamba_amd.network import blockdenoise
    ckpt, noisy_dir, files, root = folder
    calls = []
    real = blockdenoise.denoise_long

    def spy(model, x, **kw):
        calls.append(int(x.shape[-1]))
        return real(model, x, **kw)
    monkeypatch.setattr(blockdenoise, "denoise_long", spy)
    # budget 1000 samples: files whose padded length (766 + 256 k) is above it go through denoise_long one by one
    noisy, cleaned = D.denoise(ckpt, noisy_dir, None, budget_samples=1000)
    assert sorted(calls) == sorted(n for n in LENGTHS if n > 766)
    model = D.load_pretrained_CleanUMamba(ckpt).eval()
    with torch.no_grad():
        for k, n in enumerate(sorted(files)):
            x = torch.from_numpy(noisy[k]).to(cuda)
            lone = model(x.view(1, 1, -1))[0, 0]
            assert cleaned[k].shape == (len(files[n]),)
            assert rel_l2(cleaned[k], lone) < E2E_TOL, n
