"""Mamba2 bottleneck (mamba_v2=True) on the HIP kernels of csrc/ssd.hip against the f64 restatement
(tests/mamba2_ref.py): the chunked scan forward and backward, the gated RMSNorm, the one-token step, the whole
Experiment_CleanU_Mamba2 model against the reference-class fixture, and streaming."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from conftest import load_ckpt, load_golden, record, rel_l2
import mamba2_ref as M2

pytestmark = pytest.mark.gpu

PN = [(p, n) for p in (16, 32, 64) for n in (16, 32, 64)]
TB = [(1, 1), (7, 3), (63, 1), (64, 3), (65, 16), (625, 1)]
TOL_FWD = {torch.float32: 1e-5, torch.float16: 5e-4, torch.bfloat16: 3e-3}


def _inputs(cuda, b, T, H, P, N, dtype, seed):
    g = torch.Generator(device=cuda).manual_seed(seed)
    conv_dim = H * P + 2 * N
    xBC = torch.randn(b, T, conv_dim, generator=g, device=cuda).to(dtype)
    zx = torch.randn(b, T, 2 * H * P + 2 * N + H, generator=g, device=cuda)
    zx[..., -H:] = zx[..., -H:] * 0.5 - 1.0
    zx = zx.to(dtype)
    A_log = torch.log(torch.rand(H, generator=g, device=cuda) * 15 + 1)
    D = torch.randn(H, generator=g, device=cuda)
    bias = 0.5 * torch.randn(H, generator=g, device=cuda)
    return xBC, zx, A_log, D, bias


def _ssd(cuda, xBC, zx, A_log, D, bias, H, P, N):
    """cum_ssd_fwd alone -> (y, states)."""
    from cleanumamba_amd import hip
    from cleanumamba_amd.mamba_ssm.modules.mamba2 import _ssd_shape
    b, T, _ = xBC.shape
    d = H * P
    dt = zx[..., -H:]
    y = torch.empty(b, T, d, dtype=xBC.dtype, device=cuda)
    st = torch.empty(max(hip.lib().cum_ssd_states_elems(b, T, H, P, N), 1), device=cuda)
    s = _ssd_shape(xBC, dt, xBC[..., d:], xBC[..., d + N:], y, H, P, N)
    hip.check(hip.lib().cum_ssd_fwd(ctypes.byref(s), hip.ptr(xBC), hip.ptr(dt), hip.ptr(bias), hip.ptr(A_log),
                                    hip.ptr(D), hip.ptr(xBC[..., d:]), hip.ptr(xBC[..., d + N:]), hip.ptr(y),
                                    hip.ptr(st), None, hip.stream_ptr()))
    return y, st


def _ref_args(xBC, zx, A_log, D, bias, H, P, N):
    b, T, _ = xBC.shape
    d = H * P
    xd = xBC.double()
    return (xd[..., :d].reshape(b, T, H, P), zx[..., -H:].double(), A_log.double(), xd[..., d:d + N],
            xd[..., d + N:], D.double(), bias.double())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("P,N", PN)
@pytest.mark.parametrize("T,b", TB)
def test_ssd_forward_against_f64(cuda, T, b, P, N, dtype):
    H = 3
    xBC, zx, A_log, D, bias = _inputs(cuda, b, T, H, P, N, dtype, seed=T * 131 + b * 7 + P + N)
    y, _ = _ssd(cuda, xBC, zx, A_log, D, bias, H, P, N)
    x, dt, Al, Bm, Cm, Dd, bd = _ref_args(xBC, zx, A_log, D, bias, H, P, N)
    want = M2.ssd_ref(x, dt, Al, Bm, Cm, Dd, bd).reshape(b, T, H * P)
    assert record(f"ssd_fwd[{T}-{b}-{P}-{N}-{dtype}]", rel_l2(y, want)) < TOL_FWD[dtype]


@pytest.mark.parametrize("P,N", PN)
@pytest.mark.parametrize("T,b", TB)
def test_ssd_core_backward_against_f64_autograd_and_reproducible(cuda, T, b, P, N):
    """Scan + gated norm (the autograd node of the mixer): every gradient against f64 autograd of the restatement, and
    two backward passes give the same bits."""
    from cleanumamba_amd.mamba_ssm.modules.mamba2 import mamba2_core
    H = 2
    xBC, zx, A_log, D, bias = _inputs(cuda, b, T, H, P, N, torch.float32, seed=T * 17 + b + P * 3 + N)
    w = 1 + 0.1 * torch.randn(H * P, device=cuda)
    leaves = [t.clone().requires_grad_() for t in (xBC, zx, bias, A_log, D, w)]
    out = mamba2_core(*leaves, P, 1e-5)
    gout = torch.randn_like(out)
    grads = torch.autograd.grad(out, leaves, gout)
    grads2 = torch.autograd.grad(mamba2_core(*leaves, P, 1e-5), leaves, gout)
    for a, c in zip(grads, grads2):
        assert torch.equal(a, c)
    d = H * P
    ref = [t.detach().double().requires_grad_() for t in (xBC, zx, bias, A_log, D, w)]
    rx, rz, rb, ra, rD, rw = ref
    y = M2.ssd_ref(rx[..., :d].reshape(b, T, H, P), rz[..., -H:], ra, rx[..., d:d + N], rx[..., d + N:], rD, rb)
    want = M2.gated_rmsnorm_ref(y.reshape(b, T, d), rz[..., :d], rw)
    assert rel_l2(out, want) < 1e-5
    rgrads = torch.autograd.grad(want, ref, gout.double())
    for name, a, r in zip(("xBC", "zxbcdt", "dt_bias", "A_log", "D", "norm_w"), grads, rgrads):
        assert record(f"ssd_bwd[{T}-{b}-{P}-{N}].{name}", rel_l2(a, r)) < 1e-4, name


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("P,N", PN)
@pytest.mark.parametrize("T,b", [(65, 3), (100, 2)])
def test_ssd_core_backward_half(cuda, T, b, P, N, dtype):
    from cleanumamba_amd.mamba_ssm.modules.mamba2 import mamba2_core
    H = 4
    xBC, zx, A_log, D, bias = _inputs(cuda, b, T, H, P, N, dtype, seed=5 + T + P + N)
    w = torch.ones(H * P, device=cuda)
    leaves = [t.clone().requires_grad_() for t in (xBC, zx, bias, A_log, D, w)]
    out = mamba2_core(*leaves, P, 1e-5)
    gout = torch.randn_like(out)
    grads = torch.autograd.grad(out, leaves, gout)
    d = H * P
    ref = [t.detach().double().requires_grad_() for t in (xBC, zx, bias, A_log, D, w)]
    rx, rz, rb, ra, rD, rw = ref
    y = M2.ssd_ref(rx[..., :d].reshape(b, T, H, P), rz[..., -H:], ra, rx[..., d:d + N], rx[..., d + N:], rD, rb)
    want = M2.gated_rmsnorm_ref(y.reshape(b, T, d), rz[..., :d], rw)
    tol = 5e-3 if dtype == torch.float16 else 3e-2
    assert rel_l2(out, want) < tol
    for a, r in zip(grads, torch.autograd.grad(want, ref, gout.double())):
        assert rel_l2(a, r) < tol


def test_step_kernel_against_the_stored_vector(cuda):
    from cleanumamba_amd import hip
    g = load_golden("mamba2_ops")
    t = {k: torch.from_numpy(g["step_" + k]).float().to(cuda).contiguous()
         for k in ("zxbcdt", "conv_state", "ssm_state", "conv_w", "conv_b", "dt_bias", "A_log", "D", "norm_w")}
    S, H, P, N = t["ssm_state"].shape
    out = torch.empty(S, H * P, device=cuda)
    hip.check(hip.lib().cum_ssd_step(S, H * P, H, N, t["conv_w"].shape[1], 1e-5, hip.ptr(t["zxbcdt"]),
                                     t["zxbcdt"].stride(0), hip.ptr(t["conv_state"]), hip.ptr(t["conv_w"]),
                                     hip.ptr(t["conv_b"]), hip.ptr(t["dt_bias"]), hip.ptr(t["A_log"]), hip.ptr(t["D"]),
                                     hip.ptr(t["norm_w"]), hip.ptr(t["ssm_state"]), hip.ptr(out), H * P,
                                     hip.stream_ptr()))
    assert rel_l2(out, g["step_out"]) < 1e-5
    assert rel_l2(t["conv_state"], g["step_conv_state_out"]) < 1e-6
    assert rel_l2(t["ssm_state"], g["step_ssm_state_out"]) < 1e-5


@pytest.mark.parametrize("P,N", PN + [("E8", "E8")])
def test_step_iterated_equals_chunked_forward(cuda, P, N):
    """cum_ssd_step iterated over T tokens == the chunked forward, at every supported (headdim, d_state) (d_model 64,
    d_ssm 128) and at the E8 shape (d_model 512, 32 heads of 64, d_state 64)."""
    from cleanumamba_amd.mamba_ssm.modules.mamba2 import Mamba2
    from cleanumamba_amd.mamba_ssm.utils.generation import InferenceParams
    d_model, P, N = (512, 64, 64) if P == "E8" else (64, P, N)
    torch.manual_seed(P * 100 + N)
    m = Mamba2(d_model, d_state=N, headdim=P, expand=2, layer_idx=0).to(cuda)
    S, T = 3, 70
    u = torch.randn(S, T, d_model, device=cuda)
    with torch.no_grad():
        full = m(u)
        ip = InferenceParams(max_seqlen=1, max_batch_size=S, seqlen_offset=1)
        steps = torch.cat([m(u[:, t:t + 1], inference_params=ip) for t in range(T)], 1)
    assert record(f"mamba2_step_vs_fwd[{P}-{N}]", rel_l2(steps, full)) < 1e-5


@pytest.mark.parametrize("L", [16000, 4099])
def test_experiment_mamba2_forward_matches_the_reference_fixture(cuda, L, monkeypatch):
    from cleanumamba_amd.network import CleanUMamba
    sd, cfg = load_ckpt("mamba2")
    net = CleanUMamba(**cfg)
    net.load_state_dict(sd, strict=True)
    net = net.to(cuda).eval()
    g = load_golden("e2e_mamba2")

    def trap(*a, **k):
        raise AssertionError("vendor / ATen path taken")
    monkeypatch.setattr(F, "linear", trap)
    monkeypatch.setattr(F, "layer_norm", trap)
    monkeypatch.setattr(torch.nn.LayerNorm, "forward", trap)
    with torch.no_grad():
        y = net(torch.from_numpy(g[f"input_{L}"]).float().to(cuda))
    assert record(f"e2e_mamba2[{L}]", rel_l2(y, g[f"out_{L}"])) < 1e-4
    # training mode too: forward + backward run on the kernels
    net.train()
    x = torch.from_numpy(g[f"input_{L}"]).float().to(cuda)
    y = net(x)
    assert rel_l2(y.detach(), g[f"out_{L}"]) < 1e-4
    y.square().mean().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())


@pytest.mark.parametrize("graph", [False, True])
def test_streaming_equals_forward(cuda, graph):
    from cleanumamba_amd.network import CleanUMamba
    sd, cfg = load_ckpt("mamba2")
    net = CleanUMamba(**cfg)
    net.load_state_dict(sd, strict=True)
    net = net.to(cuda).eval()
    net.normalize_input = False
    net.use_hop_graph = graph
    x = 0.1 * torch.randn(4, 1, 6000, generator=torch.Generator().manual_seed(2))
    x = x.to(cuda)
    with torch.no_grad():
        want = net(x)[:, 0, :6000]
        net.reset_stream()
        outs = [net.feed_batch(x[:, 0, i:i + 1500]) for i in range(0, 6000, 1500)]
        assert net.hop_graph_status == ("captured" if graph else "off")
        assert "Mamba2" in net.hop_kernel_status
        out = torch.cat(outs + [net.flush_batch()], 1)
    assert out.shape == (4, 6000)
    assert record(f"mamba2_stream[graph={graph}]", rel_l2(out, want)) < 1e-5
