"""Selective scan and causal conv with an ENTERING state (cum_selective_scan_fwd_from, cum_causal_conv1d_fwd_from), and
Mamba.forward continuing from its cached states (GPU).

Oracle of the scan: the f64 recurrence of tests/scan_ref64.py started from h0.  Bounds: the per-op f32 bound of
test_scan_gpu.py (FWD_TOL 1e-5), 3e-6 between the time-parallel and the sequential kernels (only the rounding of the
segment decay differs, as in test_time_parallel_scan_vs_oracle_and_sequential), 6e-4 for f16 I/O (output rounding)."""
import pytest
import torch

import scan_ref64 as S
from conftest import rel_l2
from oracle import mamba_ref as M

pytestmark = pytest.mark.gpu
FWD_TOL = 1e-5


def _inputs(shape, dev, io=torch.float32):
    """Inputs as test_scan_odd_shapes_vs_oracle makes them (channel-contiguous memory), plus h0 = randn."""
    bsz, dim, N, L = shape
    gen = torch.Generator().manual_seed(sum(shape))
    rn = lambda *s: torch.randn(*s, generator=gen)
    t = dict(u=rn(bsz, L, dim).transpose(1, 2), delta=0.5 * rn(bsz, L, dim).transpose(1, 2),
             A=-torch.exp(0.5 * rn(dim, N)), B=rn(bsz, L, N).transpose(1, 2), C=rn(bsz, L, N).transpose(1, 2),
             D=rn(dim), z=rn(bsz, L, dim).transpose(1, 2), delta_bias=0.5 * rn(dim), h0=rn(bsz, dim, N))
    for k in ("u", "delta", "z"):
        t[k] = t[k].to(io).float()                         # the values the kernels read
    return {k: v.to(dev) for k, v in t.items()}


def _oracle(t, h0=None, sl=slice(None)):
    """f64 recurrence from h0 over the time slice sl: out (B, D, L), leaving state (B, D, N)."""
    cut = lambda v: v[..., sl]
    ut, _, dlt, zt, A_, Bt, Ct, Dv = S._prep(cut(t["u"]), cut(t["delta"]), t["A"], cut(t["B"]), cut(t["C"]), t["D"],
                                             cut(t["z"]), t["delta_bias"], True, False, torch.float64)
    h = (t["h0"] if h0 is None else h0).double().clone()
    _, out = S._gate(S._walk(ut, dlt, A_, Bt, Ct, h), ut, zt, Dv)
    return S._bdl(out), h


def _run(t, init, io=torch.float32, sl=slice(None), time_parallel=True):
    from cleanumamba_amd.mamba_ssm.ops import selective_scan_interface as ssi
    c = lambda v: v[..., sl].to(io)
    ssi.TIME_PARALLEL = time_parallel
    try:
        with torch.no_grad():
            y, last = ssi.selective_scan_fn(c(t["u"]), c(t["delta"]), t["A"], t["B"][..., sl], t["C"][..., sl], t["D"],
                                            z=c(t["z"]), delta_bias=t["delta_bias"], delta_softplus=True,
                                            return_last_state=True, **({} if init is None else {"initial_state": init}))
    finally:
        ssi.TIME_PARALLEL = True
    return y.float(), last


def _segments(shape):
    from cleanumamba_amd import hip
    return hip.lib().cum_scan_fwd_workspace_elems(*shape)


@pytest.mark.parametrize("shape", [(1, 1, 1, 1),
                                   # d_state > 16 (LDS-staged kernel), ragged channels and states
                                   (2, 130, 64, 16), (2, 130, 64, 17), (1, 64, 37, 50),
                                   # d_state <= 16: wave-specialised kernels, lengths around the 8-step half and the chunk
                                   (2, 130, 16, 41), (2, 70, 12, 23), (3, 64, 9, 7), (2, 48, 8, 15),
                                   # more waves than the wave-specialised form takes: the one-wave kernels
                                   (100, 2048, 8, 41)])
def test_sequential_scan_from_state_vs_f64(cuda, shape):
    t = _inputs(shape, cuda)
    yr, hr = _oracle(t)
    y, last = _run(t, t["h0"], time_parallel=False)
    assert rel_l2(y, yr) < FWD_TOL
    assert rel_l2(last, hr) < FWD_TOL


TP_SHAPES = [(1, 2048, 64, 624), (16, 128, 16, 624), (2, 70, 13, 257), (3, 8, 8, 129)]


@pytest.mark.parametrize("shape", TP_SHAPES)
def test_time_parallel_scan_from_state_vs_f64_and_sequential(cuda, shape):
    assert _segments(shape) > 0, "the plan does not segment this shape"
    t = _inputs(shape, cuda)
    yr, hr = _oracle(t)
    y, last = _run(t, t["h0"])
    assert rel_l2(y, yr) < FWD_TOL
    assert rel_l2(last, hr) < FWD_TOL
    ys, lasts = _run(t, t["h0"], time_parallel=False)
    assert rel_l2(y, ys) < 3e-6 and rel_l2(last, lasts) < 3e-6


@pytest.mark.parametrize("shape", [TP_SHAPES[0], TP_SHAPES[2]])
def test_time_parallel_scan_from_state_f16_io(cuda, shape):
    assert _segments(shape) > 0
    t = _inputs(shape, cuda, io=torch.float16)
    yr, hr = _oracle(t)
    y, last = _run(t, t["h0"], io=torch.float16)
    assert rel_l2(y, yr) < 6e-4
    assert rel_l2(last, hr) < FWD_TOL


@pytest.mark.parametrize("shape", [(2, 130, 64, 100), (2, 70, 13, 257)])
def test_scan_split_in_two_calls_equals_one_call(cuda, shape):
    t = _inputs(shape, cuda)
    y, last = _run(t, t["h0"])
    y1, mid = _run(t, t["h0"], sl=slice(0, 37))
    y2, end = _run(t, mid, sl=slice(37, None))
    assert rel_l2(torch.cat([y1, y2], -1), y) < 3e-6
    assert rel_l2(end, last) < 3e-6


@pytest.mark.parametrize("time_parallel", [True, False])
def test_zero_entering_state_is_the_plain_forward_and_one_tensor_can_carry(cuda, time_parallel):
    shape = (2, 70, 13, 257)
    t = _inputs(shape, cuda)
    y0, last0 = _run(t, None, time_parallel=time_parallel)
    state = torch.zeros_like(t["h0"])
    y, last = _run(t, state, time_parallel=time_parallel)
    assert torch.equal(y, y0) and torch.equal(last, last0)
    # one tensor as the entering and the leaving state of every call: three pieces equal the uncut call
    ys = []
    for sl in (slice(0, 100), slice(100, 101), slice(101, None)):
        yi, nxt = _run(t, state, sl=sl, time_parallel=time_parallel)
        state.copy_(nxt)
        ys.append(yi)
    assert rel_l2(torch.cat(ys, -1), y0) < 3e-6 and rel_l2(state, last0) < 3e-6


def test_scan_with_state_refuses_grad(cuda):
    from cleanumamba_amd.mamba_ssm.ops.selective_scan_interface import selective_scan_fn
    t = _inputs((1, 8, 4, 5), cuda)
    with pytest.raises(RuntimeError, match="inference only"):
        selective_scan_fn(t["u"].requires_grad_(True), t["delta"], t["A"], t["B"], t["C"], initial_state=t["h0"])


@pytest.mark.parametrize("io,tol", [(torch.float32, 1e-5), (torch.float16, 5e-4)])
@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("W", [2, 3, 4])
@pytest.mark.parametrize("L", [1, 2, 3, 5, 50])
def test_conv_from_state(cuda, L, W, silu, io, tol):
    from cleanumamba_amd.causal_conv1d import causal_conv1d_fn, causal_conv1d_update
    gen = torch.Generator().manual_seed(100 * L + W)
    rn = lambda *s: torch.randn(*s, generator=gen)
    x = rn(2, L, 70).transpose(1, 2).to(io).to(cuda)
    w, b, st = rn(70, W).to(cuda), rn(70).to(cuda), rn(2, 70, W).to(cuda)
    act = "silu" if silu else None
    ref = M.causal_conv1d_ref(torch.cat([st, x.float()], -1).double(), w.double(), b.double(), act)[..., W:]
    state = st.clone()
    with torch.no_grad():
        y = causal_conv1d_fn(x, w, b, act, state=state)
    assert y.dtype == io and y.shape == x.shape
    assert rel_l2(y.float(), ref) < tol
    stepped = st.clone()
    for i in range(L):
        causal_conv1d_update(x[:, :, i].float(), stepped, w, b, act)
    assert torch.equal(state, stepped)


@pytest.mark.parametrize("d_model,d_state", [(64, 16), (512, 64), (56, 12)])
def test_mamba_forward_in_chunks_equals_one_call(cuda, d_model, d_state):
    """Mamba.forward over 100 tokens in chunks of (37, 1, 62) -- prefill, one-token step, continuation from the cached
    states -- against one call; bounds of test_mamba_inner_single_node_equals_separate_ops in f32."""
    from cleanumamba_amd.mamba_ssm.modules import mamba_simple as ms
    from cleanumamba_amd.mamba_ssm.utils.generation import InferenceParams
    torch.manual_seed(d_model + d_state)
    blk = ms.Mamba(d_model, d_state=d_state, d_conv=4, expand=2, layer_idx=0).to(cuda)
    x = torch.randn(3, 100, d_model, generator=torch.Generator().manual_seed(1)).to(cuda)
    with torch.no_grad():
        whole = blk(x)
        ref_ip = InferenceParams(max_seqlen=100, max_batch_size=3)
        blk(x, inference_params=ref_ip)
        ip = InferenceParams(max_seqlen=100, max_batch_size=3)
        outs = []
        for n in (37, 1, 62):
            outs.append(blk(x[:, ip.seqlen_offset:ip.seqlen_offset + n], inference_params=ip))
            ip.seqlen_offset += n
    assert rel_l2(torch.cat(outs, 1), whole) < 2e-5
    for got, want in zip(ip.key_value_memory_dict[0], ref_ip.key_value_memory_dict[0]):
        assert rel_l2(got, want) < 2e-5
