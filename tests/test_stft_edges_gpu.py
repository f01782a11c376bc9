"""The multi-resolution STFT loss where tests/test_stft_loss_gpu.py never goes: digital silence and the 1e-7 power clamp
(the clamp branch of the forward kernels, the `live` gate of the gradient), equal signals (||Y| - |X|| exactly 0: the
gradient must be 0 as torch's norm backward is, not 0 / 0), odd window geometry (the element-wise load path of the fused
kernels, the pair that straddles an odd window start, samples under no frame), loss_fn on such clips, and rejection of
a clip no longer than the reflect padding.

Oracle: oracle/cleanumamba_ref.py::mrstft_loss_ref in float64, differentiated with the three weightings of the existing
test.  Bounds are the existing ones for the existing reason (module docstring of tests/test_stft_loss_gpu.py): values
1e-5 relative, gradient 1e-5 rel-L2 for the spectral-convergence term, 1e-3 with the log-magnitude term (sign ties).  On
these inputs the reference's own f32 arithmetic sits at <= 1.2e-7 (values), <= 1.5e-6 (sc gradient) and <= 9.5e-5 (mag
gradient) from f64.  Where the f64 value or a gradient element is exactly 0 the kernels' must be exactly 0.

Every gradient comparison is preceded by the guard of tests/stft_edges.py, asserted on the CPU before the GPU is touched:
no bin of either signal within 10 % of the clamp, where the gradient is discontinuous.  Seeds: 3 everywhere, 4 for the
hop > window geometry.  Each case runs through the fused, packed and r2c routes, which must also agree with each other
within the bounds of test_fused_packed_and_r2c_paths_agree.

Measured on an MI355X (worst case over cases, bands and routes): values 1.5e-7, sc gradient 5.2e-7 (short1024 / high),
mag gradient 1.2e-4 (win_eq_nfft / full, fused), both 1.2e-4; loss_fn: values 1.1e-7, gradient 3.4e-5.  Nothing within
3x of a bound.  Oracle zero share of hop_gt_win: 20.3 % (full), 56.2 % (high).

What the equal-signal cases found before the kernels were fixed: the packed and r2c routes returned value 0 and an
all-NaN gradient (c_sc = g / (0 * ||Y||), for sc alone, mag alone and both); the fused route returned sc = 1.5e-8,
mag = 5.4e-9 and a finite noise gradient (|g| up to 2.7e-3 through sc, 9.5e-2 through mag) -- the compiler had
contracted a * b - c * d differently in the x and the y copy of the spectrum arithmetic, so equal signals got spectra
that differed in the last bit (the fused kernels now see that a frame's samples are equal when they load them: such a
frame adds exactly 0 to both sums and gets a zero gradient; the arithmetic of every other frame is unchanged.  The
rocFFT-route loss kernels spell their x / y multiply-adds out instead).
"""
import pytest
import torch

import stft_edges as E
from conftest import record, rel_l2
from oracle import cleanumamba_ref as R

pytestmark = pytest.mark.gpu

WEIGHTS = (("sc", 2.0, 0.0, 1e-5), ("mag", 0.0, 3.0, 1e-3), ("both", 2.0, 3.0, 1e-3))
ROUTES = ("fused", "packed", "r2c")
_REF = {}


def _reference(key, resolutions, band, clean, den):
    """(sc, mag, {weighting: gradient}) of the f64 oracle, computed once per case and never modified."""
    if key not in _REF:
        for sig in (clean, den):
            assert E.guard_count(sig.double(), resolutions) == 0, key          # precondition, before any GPU work
        kw = E.ref_kwargs(resolutions, band)
        grads = {}
        for tag, w_sc, w_mag, _ in WEIGHTS:
            x = den.double().requires_grad_(True)
            sc, mag = R.mrstft_loss_ref(x, clean.double(), **kw)
            (w_sc * sc + w_mag * mag).backward()
            grads[tag] = x.grad
        _REF[key] = (sc.item(), mag.item(), grads)
    return _REF[key]


def _module(resolutions, band, cuda):
    from cleanumamba_amd.util.stft_loss import MultiResolutionSTFTLoss
    kw = E.ref_kwargs(resolutions, band)
    return MultiResolutionSTFTLoss(fft_sizes=list(kw["fft_sizes"]), hop_sizes=list(kw["hop_sizes"]),
                                   win_lengths=list(kw["win_lengths"]), sc_lambda=0.5, mag_lambda=0.5, band=band).to(cuda)


def _set_route(monkeypatch, route):
    from cleanumamba_amd.util import stft_loss as S
    monkeypatch.setattr(S, "_FUSED", route == "fused")
    monkeypatch.setattr(S, "_PACKED", route != "r2c")


def _run(mr, cuda, clean, den):
    grads = {}
    for tag, w_sc, w_mag, _ in WEIGHTS:
        xg = den.to(cuda).requires_grad_(True)
        sc, mag = mr(xg, clean.to(cuda))
        (w_sc * sc + w_mag * mag).backward()
        grads[tag] = xg.grad.cpu()
    return sc.item(), mag.item(), grads


def _close(got, want, rel):
    return got == 0.0 if want == 0.0 else abs(got - want) < rel * abs(want)


def _compare(name, got, ref):
    """One route's (sc, mag, gradients) against the oracle's; every distance is recorded before it is asserted."""
    for i, term in enumerate(("sc", "mag")):
        d = record(f"stft_edges/{name}/value_{term}", abs(got[i] - ref[i]) / abs(ref[i]) if ref[i] else abs(got[i]))
        print(f"{name} value {term}: got {got[i]!r} want {ref[i]!r} dist {d:.3e}")
        assert _close(got[i], ref[i], 1e-5), (name, term, got[i], ref[i])
    for tag, _, _, tol in WEIGHTS:
        g, g_r = got[2][tag], ref[2][tag]
        assert torch.isfinite(g).all(), (name, tag)
        d = record(f"stft_edges/{name}/grad_{tag}", rel_l2(g, g_r))
        print(f"{name} grad {tag}: rel_l2 {d:.3e} (bound {tol:g}), oracle zero share {float((g_r == 0).double().mean()):.4f}")
        assert d < tol, (name, tag, d)
        assert float(g[g_r == 0].abs().sum()) == 0.0, (name, tag)       # exact zeros of the oracle are exact zeros here


def _routes_agree(name, res):
    for route in ("fused", "r2c"):
        a, b = res[route], res["packed"]
        assert a[0] == b[0] or _close(a[0], b[0], 1e-6), (name, route, a[0], b[0])
        assert a[1] == b[1] or _close(a[1], b[1], 1e-6), (name, route, a[1], b[1])
        for tag, tol in (("sc", 1e-5), ("mag", 2e-3), ("both", 2e-3)):
            d = record(f"stft_edges/{name}/{route}_vs_packed/grad_{tag}", rel_l2(a[2][tag], b[2][tag]))
            assert d < tol, (name, route, tag, d)


def _all_routes(name, resolutions, band, clean, den, cuda, monkeypatch):
    ref = _reference((name, band), resolutions, band, clean, den)
    mr = _module(resolutions, band, cuda)
    res = {}
    for route in ROUTES:
        _set_route(monkeypatch, route)
        res[route] = _run(mr, cuda, clean, den)
    for route in ROUTES:
        _compare(f"{name}/{band}/{route}", res[route], ref)
    _routes_agree(f"{name}/{band}", res)
    return ref, res


@pytest.mark.parametrize("band", ["full", "high"])
@pytest.mark.parametrize("case", sorted(E.SILENCE))
def test_silence(cuda, case, band, monkeypatch):
    """Digital silence over [1500:4200) of den, of clean, of both; den all zero or faint (every bin dead); clean all zero."""
    clean, den = E.SILENCE[case](E.SILENCE_SEED)
    if case in ("den_zero", "den_faint"):
        assert E.max_power(den.double(), E.STANDARD) < 0.9e-7              # dead with the guard's margin
    ref, res = _all_routes(case, E.STANDARD, band, clean, den, cuda, monkeypatch)
    if case in ("den_zero", "den_faint"):
        for route in ROUTES:
            for tag, *_ in WEIGHTS:
                assert float(res[route][2][tag].abs().max()) == 0.0, (route, tag)


@pytest.mark.parametrize("case,band", [("equal", "full"), ("equal", "high"), ("half_equal", "high")])
def test_equal_signals_give_zero_loss_and_zero_gradient(cuda, case, band, monkeypatch):
    """den == clean over the band: value 0 and a finite, exactly-zero gradient through sc alone, mag alone and both (the
    kernels divide by ||Y| - |X|| * ||Y||; torch's norm backward is 0 at a zero norm).  half_equal differs before sample
    2400, outside every frame of the high band."""
    if case == "equal":
        clean = E.pair(E.B, E.L, E.SILENCE_SEED)[0]
        den = clean.clone()
    else:
        clean, den = E.half_equal()
        assert not torch.equal(clean[:, :E.HALF_EQUAL_FROM], den[:, :E.HALF_EQUAL_FROM])
    ref, res = _all_routes(case, E.STANDARD, band, clean, den, cuda, monkeypatch)
    assert ref[0] == 0.0 and ref[1] == 0.0 and all(float(g.abs().max()) == 0.0 for g in ref[2].values())
    for route in ROUTES:
        sc, mag, grads = res[route]
        assert sc == 0.0 and mag == 0.0, route
        for tag, g in grads.items():
            assert torch.isfinite(g).all() and float(g.abs().max()) == 0.0, (route, tag)


def test_equal_frames_among_unequal_ones(cuda, monkeypatch):
    """half_equal over the full band: frames of equal samples (zero contribution, zero gradient -- the oracle's gradient
    is exactly 0 on the samples only they cover) next to ordinary ones, in one launch."""
    clean, den = E.half_equal()
    ref, _ = _all_routes("half_equal", E.STANDARD, "full", clean, den, cuda, monkeypatch)
    assert ref[0] > 0 and ref[1] > 0
    assert float((ref[2]["both"] == 0).double().mean()) >= 0.25


@pytest.mark.parametrize("band", ["full", "high"])
@pytest.mark.parametrize("case", sorted(E.GEOMETRY))
def test_odd_geometry(cuda, case, band, monkeypatch):
    """Single resolutions with odd hop / window / offset, window = n_fft, hop > window, a transform length outside the
    fused kernels, and the shortest legal clips (tests/stft_edges.py::GEOMETRY says what each one exercises)."""
    resolutions, clean, den = E.geometry(case)
    ref, _ = _all_routes(case, resolutions, band, clean, den, cuda, monkeypatch)
    if case == "hop_gt_win":                  # 20.3 % (full) of the samples lie under no frame: the zero check is not vacuous
        share = record(f"stft_edges/{case}/{band}/oracle_zero_share", float((ref[2]["both"] == 0).double().mean()))
        assert share >= 0.10


def test_loss_fn_on_silent_clips(cuda, monkeypatch):
    """loss_fn (components + _Combine) with the default high band: clip 0's clean all zero, clip 1's den silent in its
    second half; loss, stft_sc, stft_mag and d loss / d den against loss_ref in f64."""
    from cleanumamba_amd.util.stft_loss import MultiResolutionSTFTLoss
    from cleanumamba_amd.util.util import loss_fn
    clean, den = E.loss_fn_batch()
    for sig in (clean, den):
        assert E.guard_count(sig.squeeze(1).double(), E.STANDARD) == 0
    x = den.double().requires_grad_(True)
    loss_r = R.loss_ref(x, clean.double(), stft_config=dict(band="high"))
    loss_r.backward()
    sc_r, mag_r = R.mrstft_loss_ref(den.squeeze(1).double(), clean.squeeze(1).double(), band="high")
    mr = MultiResolutionSTFTLoss(sc_lambda=0.5, mag_lambda=0.5, band="high", hop_sizes=[50, 120, 240],
                                 win_lengths=[240, 600, 1200], fft_sizes=[512, 1024, 2048]).to(cuda)
    for route in ROUTES:
        _set_route(monkeypatch, route)
        xg = den.to(cuda).requires_grad_(True)
        loss, dic = loss_fn(lambda _: xg, (clean.to(cuda), clean.to(cuda)), mrstftloss=mr)
        loss.backward()
        for term, got, want in (("loss", loss.item(), loss_r.item()), ("stft_sc", dic["stft_sc"].item(), sc_r.item()),
                                ("stft_mag", dic["stft_mag"].item(), mag_r.item())):
            d = record(f"stft_edges/loss_fn/{route}/value_{term}", abs(got - want) / abs(want))
            print(f"loss_fn {route} {term}: got {got!r} want {want!r} dist {d:.3e}")
            assert d < 1e-5, (route, term)
        assert torch.isfinite(xg.grad).all()
        d = record(f"stft_edges/loss_fn/{route}/grad", rel_l2(xg.grad, x.grad))
        print(f"loss_fn {route} grad: rel_l2 {d:.3e}")
        assert d < 1e-3, route


@pytest.mark.parametrize("n_fft,hop,win", E.STANDARD)
def test_clip_as_short_as_the_reflect_padding_is_rejected(cuda, n_fft, hop, win, monkeypatch):
    """L == n_fft / 2: the library refuses before any launch (fused and rocFFT routes), as torch.stft does on the CPU."""
    from cleanumamba_amd.util.stft_loss import STFTLoss
    x = 0.05 * torch.randn(2, n_fft // 2, generator=torch.Generator().manual_seed(3))
    f = STFTLoss(n_fft, hop, win)
    with pytest.raises(RuntimeError):
        f(x, x)
    f = f.to(cuda)
    for route in ROUTES:
        _set_route(monkeypatch, route)
        with pytest.raises(RuntimeError, match="shorter than the reflect padding"):
            f(x.to(cuda), x.to(cuda))
    torch.cuda.synchronize()
    _set_route(monkeypatch, "fused")
    ok = 0.05 * torch.randn(2, n_fft // 2 + 1, generator=torch.Generator().manual_seed(3)).to(cuda)
    sc, mag = f(ok, ok)                                        # one sample more is legal
    assert torch.isfinite(sc) and torch.isfinite(mag)
