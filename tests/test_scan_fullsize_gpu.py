"""The selective scan against an f64 restatement (tests/scan_ref64.py) at every shape bench.py times, over all clips and
channels, forward and every gradient; the fused Mamba node's direct call; and gap poisoning of every operand.

Each output is held to three measures, so that a local error cannot hide in an average: rel-L2 over the whole tensor;
rel-L2 per clip (dB, dC: per clip and per (clip, 16-step chunk)); and the worst element's |error| over the RMS of the
reference on its slice (clip; (clip, chunk) for dB, dC; the whole tensor for dA, dD, d delta_bias)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from conftest import record
import scan_ref64 as S

pytestmark = pytest.mark.gpu

FWD_TOL, BWD_TOL = 1e-5, 1e-4             # as tests/test_scan_gpu.py: f32 I/O
HALF_TOL = {torch.float16: (6e-4, 2e-3)}  # as tests/test_scan_gpu.py: 16-bit output rounding
CHUNK = 16
# worst |error| / RMS(reference slice): about 3x the largest value measured over the cases below on an MI355X.  In 16-bit
# I/O it is the rounding of the largest elements of u / delta / z-sized outputs (up to ~100x their RMS at these sizes)
WORST = {torch.float32: dict(y=6e-5, last=1e-5, y_pre=5e-6, du=4e-5, ddelta=6e-5, dz=5e-5, dA=2e-5, dB=1.2e-5, dC=1e-5,
                             dD=7e-6, ddelta_bias=7e-6),
         torch.float16: dict(y=1e-1, last=1e-5, y_pre=2e-2, du=1e-1, ddelta=1.4e-1, dz=1.2e-1, dA=5e-5, dB=1.2e-5,
                             dC=1e-5, dD=1.3e-5, ddelta_bias=1.2e-5)}


def _tols(io, name):
    ftol, btol = (FWD_TOL, BWD_TOL) if io == torch.float32 else HALF_TOL[io]
    if name == "last":
        return FWD_TOL
    return ftol if name in ("y", "y_pre") else btol


def _name(io):
    return {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}[io]


def _compare(tag, name, got, ref, io, chunked=False):
    """got: kernel output (any dtype, on the GPU); ref: f64 of the same shape.  Clip-major tensors ((B, ., .)) are also
    measured per clip; ``chunked`` (B, N, L) tensors per (clip, 16-step chunk) as well."""
    tol, wtol = _tols(io, name), WORST[io][name]
    g = got.double()
    assert g.shape == ref.shape, (tag, name)
    assert bool(torch.isfinite(g).all()), f"{tag} {name}: non-finite output"
    e = g - ref
    whole = (e.norm() / ref.norm()).item()
    if ref.dim() == 3:
        dims = (1, 2)
        e2, r2, emax = e.square().sum(dims), ref.square().sum(dims), e.abs().amax(dims)
        cnt = ref[0].numel()
        per = (e2 / r2).sqrt().max().item()
        worst = (emax / (r2 / cnt).sqrt()).max().item()
        if chunked:
            L = ref.shape[2]
            pad = (-L) % CHUNK
            fold = lambda t, red: red(F.pad(t, (0, pad)).view(t.shape[0], -1, CHUNK), -1)
            sum_, max_ = (lambda t, d: t.sum(d)), (lambda t, d: t.amax(d))
            e2c, r2c = fold(e.square().sum(1), sum_), fold(ref.square().sum(1), sum_)
            emc = fold(e.abs().amax(1), max_)
            cntc = fold(torch.ones_like(ref[0, 0])[None], sum_) * ref.shape[1]
            per = max(per, (e2c / r2c).sqrt().max().item())
            worst = (emc / (r2c / cntc).sqrt()).max().item()
    else:
        per = whole
        worst = (e.abs().max() / ref.square().mean().sqrt()).item()
    record(f"scan_fullsize {tag} {name} rel_l2", whole)
    record(f"scan_fullsize {tag} {name} max_slice_rel_l2", per)
    record(f"scan_fullsize {tag} {name} worst_over_rms", worst)
    assert whole < tol, f"{tag} {name}: rel-L2 {whole:.3e} >= {tol:.1e}"
    assert per < tol, f"{tag} {name}: worst slice rel-L2 {per:.3e} >= {tol:.1e}"
    assert worst < wtol, f"{tag} {name}: worst element / RMS {worst:.3e} >= {wtol:.1e}"


# Every case of bench.py scan_rows (same order, shapes, I/O types and backward flags), and the path the planner gives it:
# fwd_tp / bwd_tp: time-parallel forward (csrc/scan_seg.hip) / backward (csrc/scan_bwd_small.hip PASS 1 / 0) -- exactly
# the rows for which the bench also times the sequential kernels; keeps_y: the forward keeps y for the backward.
F16 = torch.float16
BENCH_CASES = [
    # name,                              B,    D,   N,    L,  io,            bwd,   fwd_tp, bwd_tp, keeps_y
    ("E8 bottleneck",                    16, 2048, 64, 624, F16, True, False, False, True),
    ("E8 bottleneck f32",                16, 2048, 64, 624, torch.float32, False, False, False, True),
    ("E6 bottleneck",                    32, 2048, 64, 2499, F16, False, False, False, True),
    ("D2048 N16 L2499 B16",              16, 2048, 16, 2499, F16, True, False, False, False),
    ("D2048 N16 L2499 B16 f32",          16, 2048, 16, 2499, torch.float32, False, False, False, False),
    ("D2048 N8 L2499 B16",               16, 2048, 8, 2499, F16, True, False, False, False),
    ("D2048 N8 L2499 B16 f32",           16, 2048, 8, 2499, torch.float32, False, False, False, False),
    ("D2048 N16 L2499 B128 f32",         128, 2048, 16, 2499, torch.float32, False, False, False, False),
    ("D2048 N8 L2499 B128 f32",          128, 2048, 8, 2499, torch.float32, False, False, False, False),
    ("D2048 N8 L2499 B128",              128, 2048, 8, 2499, F16, False, False, False, False),
    ("E8 B1 file denoising",             1, 2048, 64, 624, F16, False, True, False, False),
    ("442K model",                       16, 128, 16, 624, torch.float32, True, True, True, False),
    ("pruned-E8 block B256",             256, 48, 8, 1875, torch.float32, True, True, False, False),
]
# beyond the bench: finalize_rows at d_state > 16 (batch x segments > 64); a ragged-wave d_state-64-family kernel
# (5 waves of 8 states, FULL = false) with the scalar finalize (L * N % 4 != 0)
EXTRA_CASES = [
    ("finalize_rows d_state 64",         72, 130, 64, 45, torch.float32, True, False, False, True),
    ("ragged 5-wave scalar finalize",    3, 100, 37, 37, torch.float32, True, False, False, True),
]


def _plan_shape(bsz, dim, N, L):
    from cleanumamba_amd import hip
    s = hip.ScanShape()
    s.batch, s.dim, s.dstate, s.len = bsz, dim, N, L
    return s


def _assert_path(bsz, dim, N, L, fwd_tp, bwd_tp, keeps):
    from cleanumamba_amd import hip
    from cleanumamba_amd.mamba_ssm.ops import selective_scan_interface as ssi
    lib = hip.lib()
    assert (lib.cum_scan_fwd_workspace_elems(bsz, dim, N, L) > 0) == fwd_tp, "time-parallel forward plan changed"
    assert (lib.cum_scan_bwd_tp_workspace_elems(bsz, dim, N, L) > 0) == bwd_tp, "time-parallel backward plan changed"
    assert ssi.keeps_y(_plan_shape(bsz, dim, N, L)) == keeps, "keeps_y plan changed"


def _bench_inputs(dev, bsz, dim, N, L, io, seed):
    """The bench's operands (bench.py _scan_case): u, z halves of one (B, L, 2D) buffer, delta channel-contiguous, A the
    S4D-real init, B and C column slices of the x_proj output."""
    g = torch.Generator(device=dev).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    R = max(4, dim // 64)
    xz = rn(bsz, L, 2 * dim).to(io)
    dl = (0.3 * rn(bsz, L, dim)).to(io)
    A = -torch.exp(torch.log(torch.arange(1, N + 1, device=dev).float())[None].repeat(dim, 1))
    xd = rn(bsz, L, R + 2 * N)
    t = dict(u=xz[..., :dim].transpose(1, 2), z=xz[..., dim:].transpose(1, 2), delta=dl.transpose(1, 2), A=A,
             B=xd[..., R:R + N].transpose(1, 2), C=xd[..., R + N:].transpose(1, 2), D=rn(dim), delta_bias=0.3 * rn(dim))
    dout = rn(bsz, L, dim).to(io).transpose(1, 2)
    return t, dout


def _free():
    import gc
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("case", BENCH_CASES + EXTRA_CASES, ids=lambda c: c[0].replace(" ", "_"))
def test_scan_fullsize_vs_f64(cuda, case):
    from cleanumamba_amd.mamba_ssm.ops.selective_scan_interface import selective_scan_fn
    name, bsz, dim, N, L, io, bwd, fwd_tp, bwd_tp, keeps = case
    _assert_path(bsz, dim, N, L, fwd_tp, bwd_tp, keeps)
    tag = f"{name} ({bsz},{dim},{N},{L}) {_name(io)}"
    t, dout = _bench_inputs(cuda, bsz, dim, N, L, io, seed=bsz + dim + N + L)
    kw = dict(D=t["D"], z=t["z"], delta_bias=t["delta_bias"], delta_softplus=True)
    # the kernels read u, delta, z in the I/O type: the reference gets those rounded values
    args = (t["u"], t["delta"], t["A"], t["B"], t["C"])
    with torch.no_grad():
        y, last = selective_scan_fn(*args, return_last_state=True, **kw)          # the bench's timed inference call
    if not bwd:
        with torch.no_grad():
            yr, lastr = S.selective_scan64(*args, return_last_state=True, **kw)
        _compare(tag, "y", y, yr, io)
        _compare(tag, "last", last, lastr, io)
        return
    ref = S.selective_scan64_bwd(dout, *args, **kw)
    _compare(tag, "y", y, ref["out"], io)
    _compare(tag, "last", last, ref["last"], io)
    del y, last
    keys = ("u", "delta", "A", "B", "C", "D", "z", "delta_bias")
    leaves = {k: t[k].detach().requires_grad_(True) for k in keys}
    yg = selective_scan_fn(*(leaves[k] for k in ("u", "delta", "A", "B", "C")), D=leaves["D"], z=leaves["z"],
                           delta_bias=leaves["delta_bias"], delta_softplus=True)
    grads = torch.autograd.grad(yg, [leaves[k] for k in keys], dout)
    _compare(tag + " (training forward)", "y", yg.detach(), ref["out"], io)
    for k, gk in zip(keys, grads):
        _compare(tag, "d" + k, gk, ref["d" + k], io, chunked=k in ("B", "C"))
    _free()


def _gapped(vals, fill, off=2, extra_d=70, extra_l=17):
    """vals (B, L, X) -> (buffer, (B, X, L) view): channel-contiguous rows of pitch X + extra_d starting at column
    ``off``, extra_l rows after each clip; everything outside the view holds ``fill``.  The padding exceeds a 64-channel
    group and a 16-step chunk, so a kernel that overran its masks would still read inside the allocation."""
    b, L, X = vals.shape
    buf = torch.full((b, L + extra_l, X + extra_d), fill, dtype=vals.dtype, device=vals.device)
    buf[:, :L, off:off + X] = vals
    return buf, buf[:, :L, off:off + X].transpose(1, 2)


def _fronted(vals, fill, guard=1024):
    """vals (any shape) -> (buffer, view): the contiguous front of a flat buffer with ``guard`` elements of ``fill``."""
    n = vals.numel()
    buf = torch.full((n + guard,), fill, dtype=vals.dtype, device=vals.device)
    buf[:n] = vals.reshape(-1)
    return buf, buf[:n].view(vals.shape)


def _gap_mask(buf, view):
    """True where the contiguous ``buf`` is not covered by ``view``."""
    m = torch.ones_like(buf, dtype=torch.bool)
    m.as_strided(view.shape, view.stride(), view.storage_offset() - buf.storage_offset()).fill_(False)
    return m


def _direct_call(ins, dout, io, flags, fill):
    """Forward and backward through the C entries, as _MambaInnerFn calls them, on buffers this test owns.
    ins: dict of (B, L, X) / parameter values; every operand is laid out gapped (_gapped) or fronted (_fronted) in
    buffers prefilled with ``fill``, and so are the outputs, the checkpoints and the workspace.  Returns
    {name: (buffer, view)} of every output."""
    from cleanumamba_amd import hip
    from cleanumamba_amd.mamba_ssm.ops import selective_scan_interface as ssi
    lib = hip.lib()
    dev = dout.device
    bsz, L, dim = ins["u"].shape
    N = ins["A"].shape[1]
    has_z = ins.get("z") is not None
    u = _gapped(ins["u"], fill)[1]
    delta = _gapped(ins["delta"], fill)[1]
    z = _gapped(ins["z"], fill)[1] if has_z else None
    dyT = _gapped(dout, fill)[1]
    bc_buf = torch.full((bsz, L + 17, 2 * N + 3), fill, dtype=torch.float32, device=dev)
    bc_buf[:, :L, 1:1 + N], bc_buf[:, :L, 2 + N:2 + 2 * N] = ins["B"], ins["C"]
    Bm, Cm = bc_buf[:, :L, 1:1 + N].transpose(1, 2), bc_buf[:, :L, 2 + N:2 + 2 * N].transpose(1, 2)
    A = _fronted(ins["A"], fill)[1]
    Dv = _fronted(ins["D"], fill)[1] if ins.get("D") is not None else None
    bias = _fronted(ins["delta_bias"], fill)[1] if ins.get("delta_bias") is not None else None
    zeros_bld = torch.zeros(bsz, L, dim, dtype=io, device=dev)
    outs = {"y": _gapped(zeros_bld, fill)}
    s = ssi._shape(u, delta, z, outs["y"][1], Bm, Cm, True)
    s.delta_softplus |= flags
    if has_z and ssi.keeps_y(s):
        outs["y_pre"] = _gapped(zeros_bld, fill)
    outs["last"] = _fronted(torch.zeros(bsz, dim, N, device=dev), fill)
    ckpt = torch.full((max(lib.cum_scan_ckpt_elems(bsz, dim, N, L), 1),), fill, dtype=torch.float32, device=dev)
    ssi.scan_forward(s, u, delta, A, Bm, Cm, Dv, z, bias, outs["y"][1], outs["last"][1], ckpt, True,
                     y_pre=outs["y_pre"][1] if "y_pre" in outs else None)
    # backward: o_* strides := dout's; y_pre has the same layout as dout here
    su = ssi._shape(u, delta, z, dyT, Bm, Cm, True)
    su.delta_softplus |= flags
    for k in ("du", "ddelta") + (("dz",) if has_z else ()):
        outs[k] = _gapped(zeros_bld, fill)
    gs = hip.ScanGradStrides()
    gs.du_sb, gs.du_sd, gs.du_sl = outs["du"][1].stride()
    gs.dd_sb, gs.dd_sd, gs.dd_sl = outs["ddelta"][1].stride()
    if has_z:
        gs.dz_sb, gs.dz_sd, gs.dz_sl = outs["dz"][1].stride()
    outs["dA"] = _fronted(torch.zeros(dim, N, device=dev), fill)
    outs["dB"] = _fronted(torch.zeros(bsz, L, N, device=dev), fill)
    outs["dC"] = _fronted(torch.zeros(bsz, L, N, device=dev), fill)
    if Dv is not None:
        outs["dD"] = _fronted(torch.zeros(dim, device=dev), fill)
    if bias is not None:
        outs["ddelta_bias"] = _fronted(torch.zeros(dim, device=dev), fill)
    bwd, ws = ssi.scan_backward_entry(bsz, dim, N, L, dev)
    ws.fill_(fill)
    p = lambda k: hip.ptr(outs[k][1]) if k in outs else None
    with torch.cuda.device(dev):
        hip.check(bwd(ctypes.byref(su), ctypes.byref(gs), hip.ptr(u), hip.ptr(delta), hip.ptr(A), hip.ptr(Bm),
                      hip.ptr(Cm), hip.ptr(Dv), hip.ptr(z), hip.ptr(bias), hip.ptr(dyT), p("y_pre"), hip.ptr(ckpt),
                      p("du"), p("ddelta"), p("dA"), p("dB"), p("dC"), p("dD"), p("dz"), p("ddelta_bias"),
                      hip.ptr(ws), hip.stream_ptr()))
    torch.cuda.synchronize()
    return outs


def _ref_of(ins, dout, flags):
    """f64 reference on the values the kernels read, outputs in the direct call's layouts."""
    from cleanumamba_amd.mamba_ssm.ops import selective_scan_interface as ssi
    bdl = lambda k: ins[k].transpose(1, 2) if ins.get(k) is not None else None
    r = S.selective_scan64_bwd(dout.transpose(1, 2), bdl("u"), bdl("delta"), ins["A"], bdl("B"), bdl("C"),
                               D=ins.get("D"), z=bdl("z"), delta_bias=ins.get("delta_bias"), delta_softplus=True,
                               a_is_log=bool(flags & ssi.A_IS_LOG))
    r["y"] = r.pop("out")
    r["dB"], r["dC"] = r["dB"].transpose(1, 2), r["dC"].transpose(1, 2)     # (B, L, N) as the C entry writes them
    return r


def test_scan_fused_node_call_at_e8_f16(cuda):
    """The call _MambaInnerFn (mamba_simple.py) makes, at the benched E8 shape in f16: A given as A_log (CUM_SCAN_A_IS_LOG;
    the backward returns dA_log), y before the gate kept for the backward, B | C as views of one (B, L, 2N) f32 buffer,
    z with row pitch 2D, u / delta / y / dy channel-contiguous."""
    from cleanumamba_amd import hip
    from cleanumamba_amd.mamba_ssm.ops import selective_scan_interface as ssi
    lib = hip.lib()
    Bn, Dn, N, L, cd = 16, 2048, 64, 624, torch.float16
    g = torch.Generator(device=cuda).manual_seed(8)
    rn = lambda *s: torch.randn(*s, generator=g, device=cuda)
    xz = rn(Bn, L, 2 * Dn).to(cd)
    zv = xz[..., Dn:].transpose(1, 2)
    xc = rn(Bn, L, Dn).to(cd)
    xcT = xc.transpose(1, 2)
    dt = (0.3 * rn(Bn * L, Dn)).to(cd)
    dtT = dt.view(Bn, L, Dn).transpose(1, 2)
    bc = rn(Bn, L, 2 * N)
    Bm, Cm = bc[..., :N].transpose(1, 2), bc[..., N:].transpose(1, 2)
    A = (torch.log(torch.arange(1, N + 1, device=cuda).float())[None].repeat(Dn, 1) + 0.1 * rn(Dn, N)).contiguous()
    Df, bias = rn(Dn), 0.3 * rn(Dn)
    y = torch.empty(Bn, L, Dn, dtype=cd, device=cuda)
    yT = y.transpose(1, 2)
    ckpt = torch.empty(max(lib.cum_scan_ckpt_elems(Bn, Dn, N, L), 1), dtype=torch.float32, device=cuda)
    ss = ssi._shape(xcT, dtT, zv, yT, Bm, Cm, True)
    ss.delta_softplus |= ssi.A_IS_LOG
    assert ssi.keeps_y(ss, ssi.TIME_PARALLEL)
    ypre = torch.empty_like(y)
    ssi.scan_forward(ss, xcT, dtT, A, Bm, Cm, Df, zv, bias, yT, None, ckpt, ssi.TIME_PARALLEL, y_pre=ypre.transpose(1, 2))
    dy = rn(Bn, L, Dn).to(cd)
    dyT = dy.transpose(1, 2)
    dxz = torch.full_like(xz, float("nan"))
    dzT = dxz[..., Dn:].transpose(1, 2)
    du = torch.empty(Bn, L, Dn, dtype=cd, device=cuda)
    ddelta = torch.empty(Bn, L, Dn, dtype=cd, device=cuda)
    duT, ddT = du.transpose(1, 2), ddelta.transpose(1, 2)
    dBC = torch.empty(2, Bn, L, N, dtype=torch.float32, device=cuda)
    dA_log, dD, dbias = torch.empty_like(A), torch.empty_like(Df), torch.empty_like(bias)
    bwd, ws = ssi.scan_backward_entry(Bn, Dn, N, L, cuda)
    assert bwd == lib.cum_selective_scan_bwd                                # d_state 64: the sequential backward
    su = ssi._shape(xcT, dtT, zv, dyT, Bm, Cm, True)
    su.delta_softplus |= ssi.A_IS_LOG
    gs = hip.ScanGradStrides()
    gs.du_sb, gs.du_sd, gs.du_sl = duT.stride()
    gs.dd_sb, gs.dd_sd, gs.dd_sl = ddT.stride()
    gs.dz_sb, gs.dz_sd, gs.dz_sl = dzT.stride()
    with torch.cuda.device(cuda):
        hip.check(bwd(ctypes.byref(su), ctypes.byref(gs), hip.ptr(xcT), hip.ptr(dtT), hip.ptr(A), hip.ptr(Bm), hip.ptr(Cm),
                      hip.ptr(Df), hip.ptr(zv), hip.ptr(bias), hip.ptr(dyT), hip.ptr(ypre.transpose(1, 2)), hip.ptr(ckpt),
                      hip.ptr(duT), hip.ptr(ddT), hip.ptr(dA_log), hip.ptr(dBC[0]), hip.ptr(dBC[1]), hip.ptr(dD),
                      hip.ptr(dzT), hip.ptr(dbias), hip.ptr(ws), hip.stream_ptr()))
    assert bool(torch.isnan(dxz[..., :Dn]).all()), "the backward wrote into the u half of dxz"
    r = S.selective_scan64_bwd(dyT, xcT, dtT, A, Bm, Cm, D=Df, z=zv, delta_bias=bias, delta_softplus=True, a_is_log=True)
    tag = "fused node E8 (16,2048,64,624) f16"
    _compare(tag, "y", yT, r["out"], cd)
    _compare(tag, "y_pre", ypre.transpose(1, 2), r["y_pre"], cd)
    for k, got in (("du", duT), ("ddelta", ddT), ("dz", dzT), ("dA", dA_log), ("dD", dD), ("ddelta_bias", dbias),
                   ("dB", dBC[0].transpose(1, 2)), ("dC", dBC[1].transpose(1, 2))):
        _compare(tag, k, got, r[k], cd, chunked=k in ("dB", "dC"))


POISON_CASES = [(3, 48, 5, 37), (2, 130, 13, 45), (3, 100, 37, 37), (2, 130, 37, 45), (2, 70, 13, 257),
                (1, 130, 21, 201)]


@pytest.mark.parametrize("io", [torch.float32, torch.float16], ids=_name)
@pytest.mark.parametrize("opts", ["plain", "a_log_no_z"])
@pytest.mark.parametrize("shape", POISON_CASES, ids=lambda s: "x".join(map(str, s)))
def test_scan_gap_poisoning(cuda, shape, opts, io):
    """Every operand a strided view in a larger NaN-filled buffer (u, delta, z, dout, y, y_pre, du, ddelta, dz: rows of
    a wider pitch with rows after each clip; B, C: column slices of one wider buffer; A, D, bias, last, dA, dB, dC, dD,
    d bias: the front of a buffer with a NaN guard behind it; checkpoints and workspace NaN-filled).  Every output in
    range is finite and bit-identical to a control run whose gaps hold zeros (same layout, same kernel path), matches the
    f64 reference, and every gap and guard element is still NaN."""
    from cleanumamba_amd import hip
    from cleanumamba_amd.mamba_ssm.ops import selective_scan_interface as ssi
    bsz, dim, N, L = shape
    assert dim % 64 and N % 8 and L % CHUNK
    g = torch.Generator(device=cuda).manual_seed(sum(shape))
    rn = lambda *s: torch.randn(*s, generator=g, device=cuda)
    a_log = opts == "a_log_no_z"
    ins = dict(u=rn(bsz, L, dim).to(io), delta=(0.5 * rn(bsz, L, dim)).to(io), z=None if a_log else rn(bsz, L, dim).to(io),
               A=0.5 * rn(dim, N) if a_log else -torch.exp(0.5 * rn(dim, N)), B=rn(bsz, L, N), C=rn(bsz, L, N),
               D=rn(dim), delta_bias=0.5 * rn(dim))
    dout = rn(bsz, L, dim).to(io)
    flags = ssi.A_IS_LOG if a_log else 0
    nan = float("nan")
    ctrl = _direct_call(ins, dout, io, flags, 0.0)
    pois = _direct_call(ins, dout, io, flags, nan)
    assert ctrl.keys() == pois.keys()
    for k, (buf, view) in pois.items():
        assert bool(torch.isfinite(view).all()), f"{k}: non-finite in range"
        assert torch.equal(view, ctrl[k][1]), f"{k}: differs from the zero-gap control run"
        gap = _gap_mask(buf, view)
        assert bool(torch.isnan(buf[gap]).all()), f"{k}: written outside its tensor"
    r = _ref_of(ins, dout, flags)
    tag = f"poison ({bsz},{dim},{N},{L}) {opts} {_name(io)}"
    for k, (_, view) in ctrl.items():
        _compare(tag, k, view, r[k], io, chunked=False)
