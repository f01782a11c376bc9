"""Fused multi-resolution STFT loss (one HIP kernel per direction on the library's own in-LDS FFT; HIP kernels around
rocFFT for other transform lengths) against the CPU oracle.

Oracle: oracle/cleanumamba_ref.py::mrstft_loss_ref (restates src/util/stft_loss.py:16-184, pinned to the
reference's own module by tests/golden/loss.npz), evaluated in float64.  Tolerances: values 1e-5 relative;
gradient of the spectral-convergence term 1e-5 rel-L2; gradient of the log-magnitude term 1e-3 rel-L2 -- it
contains sign(log X - log Y), so every bin where the two magnitudes tie to within f32 rounding flips a +-1/(n X)
contribution: the reference's own f32 arithmetic sits 1.6e-4..2.1e-4 from the f64 result for the same reason
(tools/debug_stft.py prints both distances).  Silence, the clamp, equal signals and odd window geometry:
tests/test_stft_edges_gpu.py.
"""
import pytest
import torch

from oracle import cleanumamba_ref as R

pytestmark = pytest.mark.gpu


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _pair(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    clean = 0.05 * torch.randn(B, L, generator=g)
    return clean, clean + 0.05 * torch.randn(B, L, generator=g)


@pytest.mark.parametrize("band", ["full", "high"])
@pytest.mark.parametrize("B,L", [(1, 1025), (3, 4001), (2, 16000), (2, 48000)])
def test_mrstft_loss_value_and_grad(cuda, band, B, L):
    from cleanumamba_amd.util.stft_loss import MultiResolutionSTFTLoss
    clean, den = _pair(B, L, seed=L + B)
    cfg = dict(sc_lambda=0.5, mag_lambda=0.5, band=band, hop_sizes=[50, 120, 240], win_lengths=[240, 600, 1200],
               fft_sizes=[512, 1024, 2048])
    mr = MultiResolutionSTFTLoss(**cfg).to(cuda)
    for w_sc, w_mag, tol in ((2.0, 0.0, 1e-5), (0.0, 3.0, 1e-3), (2.0, 3.0, 1e-3)):
        xg = den.to(cuda).requires_grad_(True)
        sc, mag = mr(xg, clean.to(cuda))
        (w_sc * sc + w_mag * mag).backward()
        xr = den.double().requires_grad_(True)
        sc_r, mag_r = R.mrstft_loss_ref(xr, clean.double(), band=band)
        (w_sc * sc_r + w_mag * mag_r).backward()
        assert abs(sc.item() - sc_r.item()) < 1e-5 * abs(sc_r.item())
        assert abs(mag.item() - mag_r.item()) < 1e-5 * abs(mag_r.item())
        assert rel_l2(xg.grad, xr.grad) < tol


def test_mrstft_loss_3d_input_strided_and_one_sided_grads(cuda):
    """(B, 1, L) inputs as loss_fn passes them after squeeze, a strided view, and backward through only one term."""
    from cleanumamba_amd.util.stft_loss import MultiResolutionSTFTLoss
    clean, den = _pair(2, 8000, seed=5)
    mr = MultiResolutionSTFTLoss(sc_lambda=0.5, mag_lambda=0.5).to(cuda)      # default resolutions / order
    wide = torch.zeros(2, 8000, 2, device=cuda)
    wide[..., 0] = den.to(cuda)
    xg = wide.requires_grad_(True)
    sc, mag = mr(xg[..., 0].unsqueeze(1), clean.to(cuda).unsqueeze(1))
    sc.backward()
    xr = den.double().requires_grad_(True)
    sc_r, mag_r = R.mrstft_loss_ref(xr, clean.double(), fft_sizes=(1024, 2048, 512), hop_sizes=(120, 240, 50),
                                    win_lengths=(600, 1200, 240))
    sc_r.backward()
    assert abs(sc.item() - sc_r.item()) < 1e-5 * abs(sc_r.item())
    assert abs(mag.item() - mag_r.item()) < 1e-5 * abs(mag_r.item())
    assert rel_l2(xg.grad[..., 0], xr.grad) < 1e-5
    assert float(xg.grad[..., 1].abs().max()) == 0.0


def test_mrstft_loss_is_reproducible_and_rejects_cpu_mix(cuda):
    from cleanumamba_amd.util.stft_loss import STFTLossFn, MultiResolutionSTFTLoss
    clean, den = _pair(2, 16000, seed=9)
    mr = MultiResolutionSTFTLoss(sc_lambda=0.5, mag_lambda=0.5).to(cuda)
    outs = []
    for _ in range(2):
        xg = den.to(cuda).requires_grad_(True)
        sc, mag = mr(xg, clean.to(cuda))
        (sc + mag).backward()
        outs.append((sc.item(), mag.item(), xg.grad.clone()))
    assert outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1]
    assert torch.equal(outs[0][2], outs[1][2])                     # fixed-order sums: bit-reproducible
    with pytest.raises(RuntimeError):
        STFTLossFn.apply(den.to(cuda), clean, mr.stft_losses[0].window, 1024, 120, 600, False)


@pytest.mark.parametrize("band", ["full", "high"])
@pytest.mark.parametrize("B,L", [(2, 20000), (3, 4001)])
def test_fused_packed_and_r2c_paths_agree(cuda, band, B, L, monkeypatch):
    """Three implementations of one loss: the fused kernels (own in-LDS FFT: framing + both transforms + loss terms in one
    launch per direction, the default), the packed route (rocFFT complex transform of n_fft/2 points, spectrum recovered
    inside the loss kernels) and the r2c / c2r route.  Values to 1e-6, the spectral-convergence gradient to 1e-5 (odd L:
    misaligned rows take the fused kernels' element-wise loads)."""
    from cleanumamba_amd.util import stft_loss as S
    clean, den = _pair(B, L, seed=11)
    cfg = dict(sc_lambda=0.5, mag_lambda=0.5, band=band, hop_sizes=[50, 120, 240], win_lengths=[240, 600, 1200],
               fft_sizes=[512, 1024, 2048])
    mr = S.MultiResolutionSTFTLoss(**cfg).to(cuda)
    res = {}
    for mode in ("fused", "packed", "r2c"):
        monkeypatch.setattr(S, "_FUSED", mode == "fused")
        monkeypatch.setattr(S, "_PACKED", mode != "r2c")
        xg = den.to(cuda).requires_grad_(True)
        sc, mag = mr(xg, clean.to(cuda))
        sc.backward()
        g_sc = xg.grad.clone()
        xg.grad = None
        sc, mag = mr(xg, clean.to(cuda))
        mag.backward()
        res[mode] = (float(sc), float(mag), g_sc, xg.grad.clone())
    for mode in ("fused", "r2c"):
        assert abs(res[mode][0] - res["packed"][0]) <= 1e-6 * abs(res["packed"][0]), mode
        assert abs(res[mode][1] - res["packed"][1]) <= 1e-6 * abs(res["packed"][1]), mode
        assert rel_l2(res[mode][2], res["packed"][2]) < 1e-5, mode
        assert rel_l2(res[mode][3], res["packed"][3]) < 2e-3, mode      # sign(log X - log Y) ties: see the module docstring
