"""add + LayerNorm (csrc/layernorm.hip) at the edges of its loops and operand paths, every output and gradient element
against its own bound (tests/block_bounds.py) around float64 F.layer_norm(h + r) and its autograd; the whole-tensor
rel_l2 limits of test_scan_gpu.py::test_add_layernorm_vs_torch hold alongside.

What each group enters that no other unit test does:
  widths      ragged chunk counts of the LN_MAXCH kernels (520: only lane 0 owns a second chunk; 2040: lane 63 lacks its
              fourth), the element kernels beyond 8 elements per lane (513 ... 2047), the single-element row;
  rows        the second trip of the persistent backward (`row += gridDim.x * 4`, from 1025 rows) and the unrolled pass of
              the finalize (`s + 28 < nslab`, from 113 rows), with ragged remainders;
  operands    null residual / bias / dres / dx32 / dxh, mixed element types, the forward on the element kernel with the
              backward on the vector kernel (f32 rows of width 72 at a pitch of 76);
  poisoning   no kernel reads or writes outside its operands: NaN between and behind the rows, in the workspace and
              behind every output."""
import pytest
import torch
import torch.nn.functional as F

import block_bounds as bb
from conftest import record, rel_l2

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
YTOL = {F32: 1e-6, BF16: 4e-3, F16: 5e-4}
GTOL = {F32: 1e-5, BF16: 5e-3, F16: 7e-4}
EPS = 1e-5


def _inputs(bsz, L, dim, dt_h, dt_y, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    off = 3 * (2 * torch.rand(bsz, L, 1, generator=g) - 1)
    return dict(h=(rn(bsz, L, dim) + off).to(dt_h), r=rn(bsz, L, dim), w=1 + 0.1 * rn(dim), b=0.1 * rn(dim),
                gy=rn(bsz, L, dim).to(dt_y), gr=rn(bsz, L, dim))


def _reference(i, dt_y, dt_h, residual, bias, use_y, use_res):
    """float64 F.layer_norm and autograd on the CPU, and the bounds: {name: (want, bound)} as 2-D tensors."""
    bsz, L, dim = i["h"].shape
    two = lambda t: t.reshape(bsz * L, dim)
    hd = i["h"].double().requires_grad_(True)
    rd = i["r"].double().requires_grad_(True) if residual else None
    wd = i["w"].double().requires_grad_(True)
    bd = i["b"].double().requires_grad_(True) if bias else None
    res = hd if rd is None else hd + rd
    y = F.layer_norm(res, (dim,), wd, bd, EPS)
    loss = (y * i["gy"].double()).sum() * (1 if use_y else 0) + (res * i["gr"].double()).sum() * (1 if use_res else 0)
    loss.backward()
    ref = bb.layernorm(two(i["h"]), two(i["r"]) if residual else None, i["w"], i["b"] if bias else None, EPS, dt_y,
                       two(i["gy"]) if use_y else None, two(i["gr"]) if use_res else None, dt_h)
    auto = {"res": two(res.detach()), "y": two(y.detach()), "dx": two(hd.grad), "dx32": two(hd.grad),
            "dw": wd.grad.view(1, dim), "db": bd.grad.view(1, dim) if bias else None}
    for name, t in auto.items():        # the closed form under the bounds is torch's operator and autograd
        if t is not None:
            assert float((ref[name][0] - t).abs().max()) <= 1e-11 * (1 + float(t.abs().max())), name
            ref[name] = (t, ref[name][1])
    return ref


def _check(tag, ref, got, tols):
    """got: {name: 2-D tensor}; tols: {name: rel_l2 limit}.  Records the worst element ratio of the case (res_out, one
    rounding whose bound is that rounding, is checked but left out of the record: it sits at 1)."""
    worst = 0.0
    for name, t in got.items():
        want, bound = ref[name]
        ratio = bb.check(t.detach().cpu(), want, bound, f"{tag}.{name}")
        worst = max(worst, ratio if name != "res" else 0.0)
        if name in tols and float(want.abs().max()) > 1e-9:   # (dw of a one-element row is 0: float64's own noise)
            assert rel_l2(t.detach().float(), want) < tols[name], (tag, name)
    record(f"layernorm.{tag}.elem", worst)
    return worst


def _autograd_case(cuda, tag, bsz, L, dim, dt_h=F32, dt_y=None, residual=True, bias=True, use_y=True, use_res=True,
                   h_grad=True, r_grad=True, pitch=None, offset=0):
    from cleanumamba_amd.mamba_ssm.ops.layernorm import AddLayerNormFn
    dt_y = dt_h if dt_y is None else dt_y
    pitch = dim + 8 if pitch is None else pitch
    i = _inputs(bsz, L, dim, dt_h, dt_y, seed=dim * 131 + bsz * L)
    ref = _reference(i, dt_y, dt_h, residual, bias, use_y, use_res)
    # hidden: a (batch, time)-strided view of a wider row buffer that starts `offset` elements into its allocation
    flat = torch.zeros(offset + bsz * (L + 2) * pitch, dtype=dt_h)
    wide = torch.randn(bsz, L + 2, pitch, generator=torch.Generator().manual_seed(1)).to(dt_h)
    wide[:, :L, :dim] = i["h"]
    flat[offset:] = wide.reshape(-1)
    flat = flat.to(cuda).requires_grad_(h_grad)
    h = flat[offset:].view(bsz, L + 2, pitch)[:, :L, :dim]
    r = i["r"].to(cuda).requires_grad_(r_grad) if residual else None
    w = i["w"].to(cuda).requires_grad_(True)
    b = i["b"].to(cuda).requires_grad_(True) if bias else None
    y, res = AddLayerNormFn.apply(h, r, w, b, EPS, dt_y)
    assert y.dtype == dt_y and res.dtype == F32 and y.is_contiguous() and res.is_contiguous()
    loss = 0
    if use_y:
        loss = loss + (y.float() * i["gy"].float().to(cuda)).sum()
    if use_res:
        loss = loss + (res * i["gr"].to(cuda)).sum()
    loss.backward()
    two = lambda t: t.reshape(bsz * L, dim)
    got = {"y": two(y), "res": two(res), "dw": w.grad.view(1, dim)}
    if bias:
        got["db"] = b.grad.view(1, dim)
    if h_grad:
        gw = flat.grad[offset:].view(bsz, L + 2, pitch)
        assert flat.grad.dtype == dt_h
        got["dx"] = two(gw[:, :L, :dim])
        assert float(gw[:, L:].abs().max()) == 0.0 and float(gw[:, :, dim:].abs().max()) == 0.0
        assert float(flat.grad[:offset].abs().sum()) == 0.0
    else:
        assert flat.grad is None
    if residual and r_grad:
        got["dx32"] = two(r.grad)
    elif residual:
        assert r.grad is None
    tols = {"res": 1e-6, "y": YTOL[dt_y], "dx": GTOL[dt_h], "dx32": 1e-5, "dw": 1e-5, "db": 1e-5}
    _check(tag, ref, got, tols)
    return i, got


# ------------------------------------------------------------------------------------------------ width classes
@pytest.mark.parametrize("dim,dt", [(d, F32) for d in (1, 8, 63, 64, 65, 504, 512, 513, 520, 1032, 2040, 2047, 2048)]
                         + [(d, t) for t in (BF16, F16) for d in (65, 520, 2047)])
def test_width_classes(cuda, dim, dt):
    i, got = _autograd_case(cuda, f"width[{dim}:{dt}]", 3, 37, dim, dt_h=dt)
    if dim == 1:        # a single-element row: d = 0 exactly, so y is the bias and the row gradient is the residual's
        assert torch.equal(got["y"].cpu(), i["b"].view(1, 1).expand(111, 1))
        assert torch.equal(got["dx"].cpu(), i["gr"].view(111, 1))
        assert torch.equal(got["dx32"].cpu(), i["gr"].view(111, 1))
        assert float(got["dw"].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ row loops
@pytest.mark.parametrize("dim", [72, 55])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 112, 113, 129, 1024, 1025, 2051])
def test_row_loops(cuda, rows, dim):
    """(1, rows, dim): 112 / 113 rows = 28 / 29 slabs straddle the first unrolled pass of the finalize; from 1025 rows the
    persistent backward takes a second trip; 2051 rows give every wave two or three rows and a ragged last trip."""
    _autograd_case(cuda, f"rows[{rows}:{dim}]", 1, rows, dim)


# ------------------------------------------------------------------------------------------------ operand presence
@pytest.mark.parametrize("dim", [72, 55])
@pytest.mark.parametrize("case", ["no_residual", "no_bias", "only_y", "only_res", "h_no_grad", "r_no_grad", "weights_only"])
def test_operand_presence(cuda, case, dim):
    kw = {"no_residual": dict(residual=False), "no_bias": dict(bias=False), "only_y": dict(use_res=False),
          "only_res": dict(use_y=False), "h_no_grad": dict(h_grad=False), "r_no_grad": dict(r_grad=False),
          "weights_only": dict(h_grad=False, r_grad=False)}[case]
    _, got = _autograd_case(cuda, f"operands[{case}:{dim}]", 3, 37, dim, **kw)
    if case == "only_res":      # no gradient reaches the norm: exact zeros for its parameters, the row gradient is gr
        assert float(got["dw"].abs().max()) == 0.0 and float(got["db"].abs().max()) == 0.0


@pytest.mark.parametrize("dim", [72, 55, 520])
@pytest.mark.parametrize("dt_h,dt_y", [(F32, BF16), (F32, F16), (BF16, F32), (F16, F32)])
def test_element_type_pairs(cuda, dt_h, dt_y, dim):
    """f32 rows normalised into a 16-bit output and 16-bit rows into an f32 output, and the gradients that come back:
    the hidden gradient in hidden's type, the residual's in f32."""
    _autograd_case(cuda, f"types[{dt_h}>{dt_y}:{dim}]", 3, 37, dim, dt_h=dt_h, dt_y=dt_y)


@pytest.mark.parametrize("offset", [0, 1])
def test_route_split(cuda, offset):
    """f32 hidden of width 72 at a time pitch of 76 elements (and one element into its allocation): rows are not 16-byte
    aligned, so the forward runs the element kernel, while the backward (contiguous operands, dim % 8 == 0) runs the
    vector kernel on what that forward saved."""
    _autograd_case(cuda, f"route[{offset}]", 3, 37, 72, pitch=76, offset=offset)


# ------------------------------------------------------------------------------------------------ C entry points
def _fronted(vals, fill, guard=256):
    """vals -> (buffer, view): the contiguous front of a flat buffer that ends in `guard` elements of `fill`."""
    n = vals.numel()
    buf = torch.full((n + guard,), fill, dtype=vals.dtype, device=vals.device)
    buf[:n] = vals.reshape(-1)
    return buf, buf[:n].view(vals.shape)


def _direct(cuda, i, dt_h, dt_y, fill, residual=True, bias=True, dres=True, dx32=True, dxh=False):
    """cum_add_layernorm_fwd / _bwd on operands laid out in buffers prefilled with `fill`: hidden as a strided view
    (fill between the rows and behind the last), every output fronted, the workspace filled.
    -> {name: (buffer, view)} of the outputs."""
    from cleanumamba_amd import hip
    lib = hip.lib()
    bsz, L, dim = i["h"].shape
    rows = bsz * L
    wide = torch.full((bsz, L + 2, dim + 8), fill, dtype=dt_h, device=cuda)
    wide[:, :L, :dim] = i["h"].to(cuda)
    h = wide[:, :L, :dim]
    dev = lambda t: t.to(cuda).contiguous()
    r = _fronted(dev(i["r"]), fill)[1] if residual else None
    w = _fronted(dev(i["w"]), fill)[1]
    b = _fronted(dev(i["b"]), fill)[1] if bias else None
    z = lambda *s, dt=F32: torch.zeros(*s, dtype=dt, device=cuda)
    outs = {"res": _fronted(z(rows, dim), fill), "y": _fronted(z(rows, dim, dt=dt_y), fill),
            "mean": _fronted(z(rows, 1), fill), "rstd": _fronted(z(rows, 1), fill)}
    with torch.cuda.device(cuda):
        hip.check(lib.cum_add_layernorm_fwd(hip.dtype_code(dt_h), hip.dtype_code(dt_y), bsz, L, dim, hip.ptr(h), h.stride(0),
                                            h.stride(1), hip.ptr(r), hip.ptr(w), hip.ptr(b), EPS, hip.ptr(outs["res"][1]),
                                            hip.ptr(outs["y"][1]), hip.ptr(outs["mean"][1]), hip.ptr(outs["rstd"][1]),
                                            hip.stream_ptr()))
    dy = _fronted(dev(i["gy"]), fill)[1]
    gr = _fronted(dev(i["gr"]), fill)[1] if dres else None
    if dx32:
        outs["dx32"] = _fronted(z(rows, dim), fill)
    if dxh:
        outs["dx"] = _fronted(z(rows, dim, dt=dt_h), fill)
    outs["dw"] = _fronted(z(1, dim), fill)
    if bias:
        outs["db"] = _fronted(z(1, dim), fill)
    ws = torch.full((lib.cum_add_layernorm_bwd_workspace_elems(dim),), fill, dtype=F32, device=cuda)
    view = lambda k: hip.ptr(outs[k][1]) if k in outs else None
    with torch.cuda.device(cuda):
        hip.check(lib.cum_add_layernorm_bwd(hip.dtype_code(dt_y), hip.dtype_code(dt_h), rows, dim, hip.ptr(dy), hip.ptr(gr),
                                            view("res"), view("mean"), view("rstd"), hip.ptr(w), view("dx32"), view("dx"),
                                            view("dw"), view("db"), hip.ptr(ws), hip.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(wide[:, :L, :dim].cpu(), i["h"])                  # the input is only read
    return outs


@pytest.mark.parametrize("dim", [55, 72, 520])
@pytest.mark.parametrize("dt", [F32, BF16])
def test_poisoned_surroundings(cuda, dim, dt):
    i = _inputs(3, 37, dim, dt, dt, seed=dim)
    kw = dict(dx32=True, dxh=dt != F32)
    clean = _direct(cuda, i, dt, dt, 0.0, **kw)
    dirty = _direct(cuda, i, dt, dt, float("nan"), **kw)
    assert set(clean) == {"res", "y", "mean", "rstd", "dx32", "dw", "db"} | ({"dx"} if dt != F32 else set())
    for name, (buf, view) in dirty.items():
        assert bool(torch.isfinite(view.float()).all()), name
        assert torch.equal(view, clean[name][1]), name                   # bit-equal to the unpoisoned run
        assert bool(torch.isnan(buf[view.numel():].float()).all()), name    # the guard behind the output is untouched
    ref = _reference(i, dt, dt, True, True, True, True)
    _check(f"poison[{dim}:{dt}]", ref, {k: v[1] for k, v in dirty.items()}, {})


@pytest.mark.parametrize("dim", [55, 72, 520])
@pytest.mark.parametrize("case", ["no_residual", "no_bias", "no_dres", "no_dx32", "no_dx"])
def test_null_operands_of_the_entry_points(cuda, case, dim):
    """The null-pointer forms autograd never produces by itself (it hands over zero tensors): residual, bias / dbias,
    dres_out (norm_f: nothing arrives for the residual stream), and either copy of the input gradient."""
    dt = BF16 if case in ("no_dx32", "no_dx") else F32
    i = _inputs(3, 37, dim, dt, dt, seed=dim + 1)
    kw = {"no_residual": dict(residual=False), "no_bias": dict(bias=False), "no_dres": dict(dres=False),
          "no_dx32": dict(dx32=False, dxh=True), "no_dx": dict(dx32=True, dxh=False)}[case]
    outs = _direct(cuda, i, dt, dt, float("nan"), **kw)
    for name, (buf, view) in outs.items():
        assert bool(torch.isnan(buf[view.numel():].float()).all()), name
    ref = _reference(i, dt, dt, kw.get("residual", True), kw.get("bias", True), True, kw.get("dres", True))
    _check(f"null[{case}:{dim}:{dt}]", ref, {k: v[1] for k, v in outs.items() if k in ref and k not in ("mean", "rstd")}, {})
