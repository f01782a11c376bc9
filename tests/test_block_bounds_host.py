"""tests/block_bounds.py checked on the CPU.  Validity: a correct kernel, emulated in plain torch f32 with every sum taken
in an order torch.sum does not use (back to front; 64 strided lanes then a butterfly), stays inside each bound against
float64.  Non-vacuity: one element moved by twice its own bound makes check_elements raise and name it.  And the argument
errors of the entry points these bounds are for, rejected before any launch (no GPU needed)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import block_bounds as bb
import mamba2_ref
from oracle import mamba_ref as M

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
ORDERS = ["reversed", "lanes64"]


def alt_sum(x, dim, order):
    """f32 sum over `dim` in a fixed order: "reversed" = one running sum from the last element to the first; "lanes64" =
    lane l adds elements l, l + 64, ... in turn, then a butterfly over the 64 lanes (the kernels' wave reduction)."""
    x = x.movedim(dim, -1)
    n = x.shape[-1]
    if order == "reversed":
        acc = torch.zeros_like(x[..., 0])
        for i in range(n - 1, -1, -1):
            acc = acc + x[..., i]
        return acc
    pad = (-n) % 64
    x = F.pad(x, (0, pad)).reshape(*x.shape[:-1], -1, 64)
    acc = torch.zeros_like(x[..., 0, :])
    for i in range(x.shape[-2]):
        acc = acc + x[..., i, :]
    o = 32
    while o >= 1:
        acc = acc[..., :o] + acc[..., o:2 * o]
        o //= 2
    return acc[..., 0]


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


# ------------------------------------------------------------------------------------------------ emulations (f32)
def ln_emulated(h, r, w, b, eps, y_dtype, dy, dres, dx_dtype, order):
    v = h.float() + (0 if r is None else r)
    D = v.shape[1]
    mean = alt_sum(v, 1, order).unsqueeze(1) / D
    d = v - mean
    rstd = torch.rsqrt(alt_sum(d * d, 1, order).unsqueeze(1) / D + eps)
    y = (d * rstd * w + (0 if b is None else b)).to(y_dtype)
    xh = d * rstd
    g = dy.float() * w
    c1, c2 = alt_sum(g, 1, order).unsqueeze(1) / D, alt_sum(g * xh, 1, order).unsqueeze(1) / D
    dx = rstd * (g - c1 - xh * c2) + (0 if dres is None else dres)
    return {"res": v, "y": y, "mean": mean, "rstd": rstd, "dx": dx.to(dx_dtype),
            "dw": alt_sum(dy.float() * xh, 0, order).unsqueeze(0), "db": alt_sum(dy.float(), 0, order).unsqueeze(0)}


def conv_emulated(x, w, b, silu, dy, order):
    B, D, L = x.shape
    W = w.shape[1]
    taps = bb._taps(x.float(), W)
    pre = torch.zeros(B, D, L) + (0 if b is None else b.view(1, D, 1))
    ks = range(W) if order == "lanes64" else range(W - 1, -1, -1)
    for k in ks:
        pre = pre + w[:, k].view(1, D, 1) * taps[k]
    y = F.silu(pre) if silu else pre
    g = dy.float()
    if silu:
        sg = torch.sigmoid(pre)
        g = g * (sg * (1 + pre * (1 - sg)))
    gp = F.pad(g, (0, W - 1))
    dx = torch.zeros(B, D, L)
    for k in ks:
        dx = dx + w[:, k].view(1, D, 1) * gp[..., W - 1 - k:W - 1 - k + L]
    flat = lambda a: a.transpose(0, 1).reshape(D, B * L)
    dw = torch.stack([alt_sum(flat(g * taps[k]), 1, order) for k in range(W)], 1)
    return {"y": y.to(x.dtype), "dx": dx.to(x.dtype), "dw": dw, "db": alt_sum(flat(g), 1, order).view(1, D)}


def gnorm_emulated(y, z, w, eps, dout, order):
    yf, zf, go = y.float(), z.float(), dout.float()
    D = yf.shape[1]
    sg = torch.sigmoid(zf)
    sz = zf * sg
    gv = yf * sz
    r = torch.rsqrt(alt_sum(gv * gv, 1, order).unsqueeze(1) / D + eps)
    out = gv * r * w
    k = alt_sum(go * w * gv, 1, order).unsqueeze(1) * r * r * r / D
    dg = go * w * r - gv * k
    return {"out": out.to(y.dtype), "rstd": r, "dy": (dg * sz).to(y.dtype),
            "dz": (dg * yf * sg * (1 + zf * (1 - sg))).to(y.dtype), "dw": alt_sum(go * (gv * r), 0, order).unsqueeze(0)}


def _ln_case(D, dt, rows=111):
    g = torch.Generator().manual_seed(D + 3 * DTYPES.index(dt))
    off = 3 * (2 * torch.rand(rows, 1, generator=g) - 1)                  # a row offset of up to +-3
    h = (_randn(g, rows, D) + off).to(dt)
    r, w, b = _randn(g, rows, D), 1 + 0.1 * _randn(g, D), 0.1 * _randn(g, D)
    dy, dres = _randn(g, rows, D).to(dt), _randn(g, rows, D)
    return h, r, w, b, dy, dres


def _conv_case(W, dt, silu=True):
    g = torch.Generator().manual_seed(W + 5 * DTYPES.index(dt))
    x, dy = _randn(g, 2, 70, 37).to(dt), _randn(g, 2, 70, 37).to(dt)
    return x, _randn(g, 70, W) / W ** 0.5, 0.1 * _randn(g, 70), dy


def _gnorm_case(D, dt, rows=37):
    g = torch.Generator().manual_seed(D + 7 * DTYPES.index(dt))
    return _randn(g, rows, D).to(dt), _randn(g, rows, D).to(dt), 1 + 0.1 * _randn(g, D), _randn(g, rows, D).to(dt)


def _all_inside(got, ref, tag):
    worst = {}
    for name, (want, bound) in ref.items():
        if name in got:
            worst[name] = bb.check(got[name], want, bound, f"{tag}.{name}")
    print(tag, {k: round(v, 4) for k, v in worst.items()})
    return worst


# ------------------------------------------------------------------------------------------------ validity
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D", [1, 7, 2048])
def test_layernorm_bounds_hold_for_a_correct_kernel(D, dt, order):
    h, r, w, b, dy, dres = _ln_case(D, dt)
    ref = bb.layernorm(h, r, w, b, 1e-5, dt, dy, dres, dt)
    # the closed form the bounds are built on is torch's own operator and autograd
    hd, rd = h.double().requires_grad_(True), r.double()
    wd, bd = w.double().requires_grad_(True), b.double().requires_grad_(True)
    yd = F.layer_norm(hd + rd, (D,), wd, bd, 1e-5)
    ((yd * dy.double()).sum() + ((hd + rd) * dres.double()).sum()).backward()
    for name, t in (("y", yd), ("dx", hd.grad), ("dw", wd.grad.view(1, D)), ("db", bd.grad.view(1, D))):
        assert float((ref[name][0] - t.detach()).abs().max()) <= 1e-11 * (1 + float(t.detach().abs().max())), name
    worst = _all_inside(ln_emulated(h, r, w, b, 1e-5, dt, dy, dres, dt, order), ref, f"ln[{D}:{dt}:{order}]")
    assert set(worst) == {"res", "y", "mean", "rstd", "dx", "dw", "db"}
    assert all(v <= 1 for v in worst.values())
    if dt != torch.float32 and D > 1:
        assert worst["y"] > 0.5 and worst["dx"] > 0.5                     # 16-bit: the bound is the rounding itself


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("W", [1, 4])
def test_conv_bounds_hold_for_a_correct_kernel(W, silu, dt, order):
    x, w, b, dy = _conv_case(W, dt)
    ref = bb.conv(x, w, b, silu, dt, dy)
    xd = x.double().requires_grad_(True)
    wd, bd = w.double().requires_grad_(True), b.double().requires_grad_(True)
    yd = M.causal_conv1d_ref(xd, wd, bd, "silu" if silu else None)
    yd.backward(dy.double())
    for name, t in (("y", yd), ("dx", xd.grad), ("dw", wd.grad), ("db", bd.grad.view(1, -1))):
        assert float((ref[name][0] - t.detach()).abs().max()) <= 1e-11 * (1 + float(t.detach().abs().max())), name
    worst = _all_inside(conv_emulated(x, w, b, silu, dy, order), ref, f"conv[{W}:{silu}:{dt}:{order}]")
    assert set(worst) == {"y", "dx", "dw", "db"} and all(v <= 1 for v in worst.values())
    if dt != torch.float32:
        assert worst["y"] > 0.5 and worst["dx"] > 0.5


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D", [1, 4096])
def test_gated_rmsnorm_bounds_hold_for_a_correct_kernel(D, dt, order):
    y, z, w, dout = _gnorm_case(D, dt)
    ref = bb.gated_rmsnorm(y, z, w, 1e-5, dt, dout)
    yd, zd, wd = (t.double().requires_grad_(True) for t in (y, z, w))
    od = mamba2_ref.gated_rmsnorm_ref(yd, zd, wd, 1e-5)
    od.backward(dout.double())
    for name, t in (("out", od), ("dy", yd.grad), ("dz", zd.grad), ("dw", wd.grad.view(1, D))):
        assert float((ref[name][0] - t.detach()).abs().max()) <= 1e-11 * (1 + float(t.detach().abs().max())), name
    worst = _all_inside(gnorm_emulated(y, z, w, 1e-5, dout, order), ref, f"gnorm[{D}:{dt}:{order}]")
    assert set(worst) == {"out", "rstd", "dy", "dz", "dw"} and all(v <= 1 for v in worst.values())
    if dt != torch.float32 and D > 1:
        assert worst["out"] > 0.5 and worst["dy"] > 0.5 and worst["dz"] > 0.5


# ------------------------------------------------------------------------------------------------ non-vacuity
def _planted(got, ref, name, row, col, tag):
    """Move got[name][row, col] (2-D view) by twice its own bound: the checker names that element."""
    want, bound = ref[name]
    n = want.shape[-1]
    moved = got[name].double().reshape(-1, n).clone()
    assert float(bound.reshape(-1, n)[row, col]) > 0
    moved[row, col] = want.reshape(-1, n)[row, col] + 2 * bound.reshape(-1, n)[row, col]
    with pytest.raises(AssertionError, match=rf"{tag}.*row {row}, column {col}[;,]"):
        bb.check(moved.reshape(want.shape), want, bound, tag)


@pytest.mark.parametrize("dt", DTYPES)
def test_one_element_twice_its_bound_away_raises(dt):
    h, r, w, b, dy, dres = _ln_case(520, dt)
    ref = bb.layernorm(h, r, w, b, 1e-5, dt, dy, dres, dt)
    got = ln_emulated(h, r, w, b, 1e-5, dt, dy, dres, dt, "lanes64")
    for name, row, col in (("res", 110, 519), ("y", 57, 512), ("mean", 3, 0), ("rstd", 110, 0), ("dx", 0, 64),
                           ("dw", 0, 513), ("db", 0, 7)):
        _planted(got, ref, name, row, col, f"ln.{name}")
    x, w, b, dy = _conv_case(3, dt)
    ref = bb.conv(x, w, b, True, dt, dy)
    got = conv_emulated(x, w, b, True, dy, "lanes64")
    for name, row, col in (("y", 139, 36), ("dx", 71, 0), ("dw", 69, 2), ("db", 0, 33)):
        _planted(got, ref, name, row, col, f"conv.{name}")
    y, z, w, dout = _gnorm_case(96, dt)
    ref = bb.gated_rmsnorm(y, z, w, 1e-5, dt, dout)
    got = gnorm_emulated(y, z, w, 1e-5, dout, "lanes64")
    for name, row, col in (("out", 36, 95), ("rstd", 5, 0), ("dy", 1, 64), ("dz", 20, 63), ("dw", 0, 65)):
        _planted(got, ref, name, row, col, f"gnorm.{name}")


def test_rel_l2_accepts_what_the_element_bound_catches():
    """Why these bounds exist: one entirely wrong element (a stale lane) of a (111, 2048) bf16 output passes the
    whole-tensor limit of 4e-3."""
    from conftest import rel_l2
    h, r, w, b, dy, dres = _ln_case(2048, torch.bfloat16)
    ref = bb.layernorm(h, r, w, b, 1e-5, torch.bfloat16, dy, dres, torch.bfloat16)
    got = ln_emulated(h, r, w, b, 1e-5, torch.bfloat16, dy, dres, torch.bfloat16, "lanes64")["y"]
    got[77, 1999] = got[77, 1998]
    assert rel_l2(got, ref["y"][0]) < 4e-3
    with pytest.raises(AssertionError, match=r"row 77, column 1999[;,]"):
        bb.check(got, *ref["y"], "stale lane")


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_are_rejected_before_any_launch():
    from cleanumamba_amd import hip
    lib = hip.lib()
    fake = lambda i: ctypes.c_void_p(0x100000 + 0x10000 * i)            # never dereferenced
    p = [fake(i) for i in range(16)]
    F32_, BF, FH = hip.CUM_F32, hip.CUM_BF16, hip.CUM_F16

    def ln_fwd(xd, yd, dim):
        return lib.cum_add_layernorm_fwd(xd, yd, 2, 3, dim, p[0], 3 * dim, dim, p[1], p[2], p[3], 1e-5, p[4], p[5], p[6],
                                         p[7], None)

    def ln_bwd(yd, hd, dim):
        return lib.cum_add_layernorm_bwd(yd, hd, 6, dim, *p[:11], None)

    for dim in (0, 2049):
        assert ln_fwd(F32_, F32_, dim) == -1 and b"d_model" in lib.cum_last_error()
        assert ln_bwd(F32_, F32_, dim) == -1 and b"d_model" in lib.cum_last_error()
    for a, b in ((BF, FH), (FH, BF)):
        assert ln_fwd(a, b, 64) == -1 and b"one 16-bit type" in lib.cum_last_error()
        assert ln_bwd(a, b, 64) == -1 and b"one 16-bit type" in lib.cum_last_error()

    assert lib.cum_gated_rmsnorm_fwd(F32_, 4, 8193, p[0], 8193, p[1], 8193, p[2], 1e-5, p[3], 8193, p[4], None) == -1
    assert b"cum_gated_rmsnorm_fwd" in lib.cum_last_error()
    assert lib.cum_gated_rmsnorm_bwd(F32_, 4, 4097, p[0], 4097, p[1], 4097, p[2], p[3], p[4], 4097, p[5], 4097, p[6], 4097,
                                     p[7], p[8], None) == -1
    assert b"cum_gated_rmsnorm_bwd" in lib.cum_last_error()

    def ola(L2=4, Cp=8, C=8, y_pitch=6):
        return lib.cum_stream_overlap_add(F32_, 2, L2, Cp, C, p[0], y_pitch, p[1], p[2], p[3], L2, p[4], L2, 1, None)

    assert ola(L2=1, y_pitch=3) == -1 and b"bad shape" in lib.cum_last_error()
    assert ola(C=9) == -1 and b"bad shape" in lib.cum_last_error()
    assert ola(y_pitch=5) == -1 and b"bad buffer" in lib.cum_last_error()

    def win(dc, rows, n_new, Cp, tmp, tail, window=p[0]):
        return lib.cum_stream_window_update(dc, 2, rows, n_new, Cp, window, p[1], rows, rows, 0, tmp, tail, n_new + 2, None)

    assert win(F32_, 9, 8, 8, p[2], p[3]) == -1 and b"two carried rows" in lib.cum_last_error()      # keep = 1
    assert win(F32_, 8, 8, 8, p[2], p[3]) == -1 and b"two carried rows" in lib.cum_last_error()      # keep = 0
    assert win(BF, 2053, 4, 8, p[2], p[3]) == -1 and b"in-place path" in lib.cum_last_error()        # keep = 2049
    assert win(BF, 22, 8, 20, p[2], p[3]) == -1 and b"in-place path" in lib.cum_last_error()         # 40-byte rows
    assert win(F32_, 22, 8, 8, p[2], p[3], window=ctypes.c_void_p(0x100004)) == -1                   # misaligned window
    assert b"in-place path" in lib.cum_last_error()
    assert win(BF, 2053, 4, 8, None, None) == -1 and b"scratch buffer" in lib.cum_last_error()
    assert win(BF, 22, 8, 20, None, None) == -1 and b"scratch buffer" in lib.cum_last_error()

    assert lib.cum_causal_conv1d_update(2, 8, 0, p[0], p[1], p[2], p[3], 1, p[4], None) == -1
    assert b"conv_update" in lib.cum_last_error()
