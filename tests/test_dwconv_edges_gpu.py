"""Causal depthwise conv (csrc/dwconv.hip) at every width, option, length / channel edge and 16-bit route, forward,
backward and streaming update: every element of y, dx, dw and db against its own bound (tests/block_bounds.py) around
oracle.mamba_ref.causal_conv1d_ref / causal_conv1d_update_ref in float64 and their autograd.

The kernels walk 16 time steps per thread, four such chunks per workgroup, 64 channels (128 on the 16-bit
two-channels-per-lane route) per wave; the weight-gradient finalize adds the per-(batch, chunk) slabs eight at a time per
wave from 29 slabs up."""
import ctypes

import pytest
import torch

import block_bounds as bb
from conftest import record, rel_l2
from oracle import mamba_ref as M

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
TOL = {F32: 1e-5, BF16: 4e-3, F16: 5e-4}
NAN = float("nan")


def _inputs(B, D, L, W, dt, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(x=rn(B, D, L).to(dt), dy=rn(B, D, L).to(dt), w=rn(D, W) / W ** 0.5, b=0.1 * rn(D))


_REF = {}


def _reference(i, silu, bias, key=None):
    """float64 reference with autograd and the bounds: {name: (want, bound)}; computed once per key."""
    if key is not None and key in _REF:
        return _REF[key]
    dt = i["x"].dtype
    xd, wd = i["x"].double().requires_grad_(True), i["w"].double().requires_grad_(True)
    bd = i["b"].double().requires_grad_(True) if bias else None
    y = M.causal_conv1d_ref(xd, wd, bd, "silu" if silu else None)
    y.backward(i["dy"].double())
    ref = bb.conv(i["x"], i["w"], i["b"] if bias else None, silu, dt, i["dy"])
    auto = {"y": y.detach(), "dx": xd.grad, "dw": wd.grad, "db": bd.grad.view(1, -1) if bias else None}
    for name, t in auto.items():
        if t is None:
            del ref[name]
            continue
        assert float((ref[name][0] - t).abs().max()) <= 1e-11 * (1 + float(t.abs().max())), name
        ref[name] = (t, ref[name][1])
    if key is not None:
        _REF[key] = ref
    return ref


def _check(tag, ref, got):
    worst = 0.0
    for name, t in got.items():
        want, bound = ref[name]
        worst = max(worst, bb.check(t.detach().cpu(), want, bound, f"{tag}.{name}"))
        assert rel_l2(t.detach().float(), want) < (TOL[t.dtype] if name in ("y", "dx") else 1e-5), (tag, name)
    record(f"dwconv.{tag}.elem", worst)
    return worst


def _lay(vals, kind, fill, cuda, pad=2, offset=0):
    """vals (B, D, L) -> (buffer, view): the values as a strided (B, D, L) view of a flat buffer otherwise full of `fill`.
    "cl": channels last, time pitch D + pad, one spare row per batch; "bdl": (B, D, L)-contiguous rows inside
    (B, D + 1, L + 3); the view starts `offset` elements into the allocation."""
    B, D, L = vals.shape
    shape = (B, L + 1, D + pad) if kind == "cl" else (B, D + 1, L + 3)
    n = shape[0] * shape[1] * shape[2]
    buf = torch.full((offset + n,), fill, dtype=vals.dtype, device=cuda)
    box = buf[offset:].view(shape)
    view = box[:, :L, :D].transpose(1, 2) if kind == "cl" else box[:, :D, :L]
    view.copy_(vals.to(cuda))
    return buf, view


def _gap_mask(buf, view):
    m = torch.ones_like(buf, dtype=torch.bool)
    m.as_strided(view.shape, view.stride(), view.storage_offset() - buf.storage_offset()).fill_(False)
    return m


def _direct(cuda, i, silu, bias, x_kind="cl", dy_kind=None, pad=2, offset=0, fill=0.0, ws_fill=None):
    """cum_causal_conv1d_fwd / _bwd on operands laid out by _lay (y and dx like x, dy as dy_kind), dw / db fronted by a
    guard, the workspace filled.  -> ({name: view}, {name: (buffer, view)})."""
    from cleanumamba_amd import hip
    lib = hip.lib()
    B, D, L = i["x"].shape
    W = i["w"].shape[1]
    dt = i["x"].dtype
    dy_kind = x_kind if dy_kind is None else dy_kind
    zeros = torch.zeros(B, D, L, dtype=dt)
    bufs = {"x": _lay(i["x"], x_kind, fill, cuda, pad, offset), "dy": _lay(i["dy"], dy_kind, fill, cuda, pad, offset),
            "y": _lay(zeros, x_kind, fill, cuda, pad, offset), "dx": _lay(zeros, x_kind, fill, cuda, pad, offset)}
    w = i["w"].to(cuda).contiguous()
    b = i["b"].to(cuda).contiguous() if bias else None
    for name, n in (("dw", D * W), ("db", D)):
        if name == "dw" or bias:
            buf = torch.full((n + 256,), fill, dtype=F32, device=cuda)
            bufs[name] = (buf, buf[:n].view(D, W) if name == "dw" else buf[:n].view(1, D))
    ws = torch.full((max(lib.cum_conv_bwd_workspace_elems(B, D, L, W), 1),), fill if ws_fill is None else ws_fill,
                    dtype=F32, device=cuda)

    def shape(a, o):
        s = hip.ConvShape()
        s.batch, s.dim, s.len, s.width = B, D, L, W
        s.x_sb, s.x_sd, s.x_sl = a.stride()
        s.y_sb, s.y_sd, s.y_sl = o.stride()
        s.silu, s.io_dtype = int(silu), hip.dtype_code(dt)
        return s

    x, dy, y, dx = (bufs[k][1] for k in ("x", "dy", "y", "dx"))
    with torch.cuda.device(cuda):
        hip.check(lib.cum_causal_conv1d_fwd(ctypes.byref(shape(x, y)), hip.ptr(x), hip.ptr(w), hip.ptr(b), hip.ptr(y),
                                            hip.stream_ptr()))
        hip.check(lib.cum_causal_conv1d_bwd(ctypes.byref(shape(x, dy)), hip.ptr(x), hip.ptr(w), hip.ptr(b), hip.ptr(dy),
                                            hip.ptr(dx), dx.stride(0), dx.stride(1), dx.stride(2), hip.ptr(bufs["dw"][1]),
                                            hip.ptr(bufs["db"][1]) if bias else None, hip.ptr(ws), hip.stream_ptr()))
    torch.cuda.synchronize()
    outs = {k: bufs[k] for k in ("y", "dx", "dw", "db") if k in bufs}
    return {k: v[1] for k, v in outs.items()}, outs


# ------------------------------------------------------------------------------------------------ widths and options
@pytest.mark.parametrize("silu,bias", [(True, True), (False, False), (True, False)])
@pytest.mark.parametrize("W", [1, 2, 3, 4])
def test_widths_and_options(cuda, W, silu, bias):
    """Through causal_conv1d_fn and its autograd, on the channel-contiguous layout the mixer hands over."""
    from cleanumamba_amd.causal_conv1d import causal_conv1d_fn
    i = _inputs(2, 70, 37, W, F32, seed=W)
    ref = _reference(i, silu, bias)
    x = i["x"].transpose(1, 2).contiguous().to(cuda).transpose(1, 2).requires_grad_(True)
    w = i["w"].to(cuda).requires_grad_(True)
    b = i["b"].to(cuda).requires_grad_(True) if bias else None
    y = causal_conv1d_fn(x, w, b, "silu" if silu else None)
    y.backward(i["dy"].transpose(1, 2).contiguous().to(cuda).transpose(1, 2))
    got = {"y": y, "dx": x.grad, "dw": w.grad}
    if bias:
        got["db"] = b.grad.view(1, -1)
    _check(f"width[{W}:{int(silu)}{int(bias)}]", ref, got)
    # the same through the entry points on the (B, D, L)-contiguous layout
    got2, _ = _direct(cuda, i, silu, bias, x_kind="bdl")
    _check(f"width_bdl[{W}:{int(silu)}{int(bias)}]", ref, got2)


@pytest.mark.parametrize("W", [4, 2])
@pytest.mark.parametrize("L", [1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 129])
def test_lengths(cuda, L, W):
    """The 16-step chunk, the 4-chunk workgroup and sequences shorter than the filter."""
    i = _inputs(2, 70, L, W, F32, seed=100 + L)
    got, _ = _direct(cuda, i, True, True)
    _check(f"len[{L}:{W}]", _reference(i, True, True), got)


@pytest.mark.parametrize("D,dt", [(d, F32) for d in (1, 2, 63, 64, 65, 127, 128, 129, 130)]
                         + [(d, BF16) for d in (2, 64, 128, 130)])
def test_channels(cuda, D, dt):
    i = _inputs(2, D, 37, 4, dt, seed=200 + D)
    got, _ = _direct(cuda, i, True, True)
    _check(f"dim[{D}:{dt}]", _reference(i, True, True), got)


# ------------------------------------------------------------------------------------------------ 16-bit routes
ROUTES = {"pair": dict(), "bdl_x": dict(x_kind="bdl"), "odd_pitch": dict(pad=1), "moved_base": dict(offset=1),
          "dy_other_layout": dict(dy_kind="bdl")}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("dt", [BF16, F16])
def test_sixteen_bit_routes(cuda, dt, route):
    """The two-channels-per-lane kernels and each reason to leave them, one at a time: x with the time axis innermost, an
    odd time pitch, a base pointer off 4-byte alignment, dy laid out differently from x (the forward of that case still
    pairs).  Every route inside its element bound; not bit-equal to each other (the packed form may contract to FMA
    differently)."""
    i = _inputs(2, 130, 45, 4, dt, seed=300)
    got, _ = _direct(cuda, i, True, True, **ROUTES[route])
    _check(f"route[{route}:{dt}]", _reference(i, True, True, key=("route", dt)), got)


@pytest.mark.parametrize("k", [1, 4, 28, 29, 33, 61])
def test_finalize_slab_counts(cuda, k):
    """batch 1, dim 8, L = 16 k: k slabs; the eight-deep pass of the finalize starts at 29, with remainders 0, 4 and 1
    beyond it at 33 and 61."""
    i = _inputs(1, 8, 16 * k, 4, F32, seed=400 + k)
    got, _ = _direct(cuda, i, True, True)
    _check(f"slabs[{k}]", _reference(i, True, True), got)


# ------------------------------------------------------------------------------------------------ update kernel
@pytest.mark.parametrize("silu,bias", [(True, True), (False, False)])
@pytest.mark.parametrize("B,D", [(1, 255), (2, 128), (1, 257), (3, 86)])
@pytest.mark.parametrize("W", [1, 2, 3, 4])
def test_update_kernel(cuda, W, B, D, silu, bias):
    """Five steps of cum_causal_conv1d_update: 255 ... 258 (batch, channel) pairs around one 256-thread workgroup.  y per
    element (the step at time t is the conv over [state | x_1 .. x_t]); the state is pure data movement: bit-exact."""
    from cleanumamba_amd.causal_conv1d import causal_conv1d_update
    g = torch.Generator().manual_seed(W * 1000 + B * D)
    seq = torch.randn(B, D, W + 5, generator=g)
    w, b = torch.randn(D, W, generator=g) / W ** 0.5, (0.1 * torch.randn(D, generator=g) if bias else None)
    act = "silu" if silu else None
    want, bound = bb.conv(seq, w, b, silu, F32)["y"]
    state = seq[:, :, :W].contiguous().to(cuda)
    state_ref = seq[:, :, :W].double().clone()
    wd, bd = w.to(cuda), None if b is None else b.to(cuda)
    worst = 0.0
    for t in range(5):
        x = seq[:, :, W + t].contiguous()
        y = causal_conv1d_update(x.to(cuda), state, wd, bd, act)
        y_ref = M.causal_conv1d_update_ref(x.double(), state_ref, w.double(), None if b is None else b.double(), act)
        assert float((want[:, :, W + t] - y_ref).abs().max()) <= 1e-11 * (1 + float(y_ref.abs().max()))
        worst = max(worst, bb.check(y.cpu(), y_ref, bound[:, :, W + t], f"update[{W}:{B}x{D}] step {t}"))
        assert rel_l2(y, y_ref) < 1e-6
        assert torch.equal(state.cpu(), seq[:, :, t + 1:t + 1 + W]) and torch.equal(state.cpu().double(), state_ref)
    record(f"dwconv.update[{W}:{B}x{D}:{int(silu)}{int(bias)}].elem", worst)


# ------------------------------------------------------------------------------------------------ poisoning
@pytest.mark.parametrize("ws_fill", [NAN, 1e30])
@pytest.mark.parametrize("dt", [F32, BF16])
def test_poisoned_surroundings(cuda, dt, ws_fill):
    """W = 3, (2, 70, 37): x, dy, y and dx are strided views of NaN-filled buffers, dw and db end in NaN guards, the
    workspace is full of NaN (its rows for the unused fourth tap are never written) or of a large finite value (which a
    store to dw beyond k < W would carry into the guard).  Outputs finite and bit-equal to the clean run, every gap and
    guard still NaN."""
    i = _inputs(2, 70, 37, 3, dt, seed=500)
    clean, _ = _direct(cuda, i, True, True, fill=0.0)
    dirty, bufs = _direct(cuda, i, True, True, fill=NAN, ws_fill=ws_fill)
    for name, (buf, view) in bufs.items():
        assert bool(torch.isfinite(view.float()).all()), name
        assert torch.equal(view, clean[name]), name
        assert bool(torch.isnan(buf[_gap_mask(buf, view)].float()).all()), name
    _check(f"poison[{dt}:{ws_fill}]", _reference(i, True, True, key=("poison", dt)), dirty)
