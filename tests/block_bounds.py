"""Element-wise error bounds of the block kernels around the scan and the GEMMs: add + LayerNorm (csrc/layernorm.hip), the
causal depthwise conv (csrc/dwconv.hip) and the gated RMSNorm (csrc/ssd.hip).  Same rule as gemm_bounds.py, whose U, FLOOR,
TRANSCENDENTAL, acc_error, element_bound and check_elements are used here: every output element has its own budget, and
no term comes from an error measured on the kernel under test.  Plain torch, float64, on whatever device the arguments
live on.  Each function returns {name: (want, bound)}; `want` is the closed form in float64 of the inputs as stored (the
tests compare it with torch's own float64 operator and autograd before they use the bound).

Notation.  u = 2^-24, one f32 rounding.  acc_error(S, K) = 2 (K + 8) u S bounds ANY order of K f32 additions of terms
whose absolute sum is S, the rounding of the terms themselves and of a final division included (gemm_bounds.py).  An
error d(x) of an input of f moves f by |f'| d(x) to first order; a product of n factors rounds n - 1 times.  A fused
multiply-add rounds less often than the separate operations: every count below is of the unfused form.

Transcendentals.  sigmoid(p) = rcp(1 + exp2(-p log2 e)) on the hardware instructions, 1 ulp each.  The rounding of the
exponent's argument is a relative u of p log2 e, i.e. a relative |p| u of the exponential; with the addition, the
reciprocal and the hardware exp that is a relative (|p| + 4) u of sigmoid, and (|p| + 6) u of silu(p) = p sigmoid(p) times
one more factor                                                                                             (silu_rel()).
silu'(p) = sg (1 + p (1 - sg)) can vanish (p = -1.278), so its error is absolute: the subtraction 1 - sg inherits the
ABSOLUTE error of sg, (|p| + 4) u sg <= 3 u where sg is near 1, multiplied by |p| sg; the remaining operations are
relative roundings of terms bounded by M = sg (1 + |p| (1 - sg)) >= |silu'|:
        d(silu') = (4 |p| + 8) u M                                                                        (dsilu_abs()).
|silu'| <= 1.1 and |silu''| <= 0.5 everywhere.

add + LayerNorm, forward, one row of width D.  v = fl(h + r), one rounding (none without a residual).
    d(mean) = acc_error(sum |v|, D) / D
    d(d_e)  = d(mean) + u (|v_e| + |d_e|)                   d_e = v_e - mean: the rounding of v_e and of the subtraction
    d(q)    = acc_error(sum d^2, D) + 2 sum |d_e| d(d_e)    q = sum d^2
    rho     = (d(q) / D) / (2 (var + eps)) + 2^-22          relative error of rstd; 2^-22: the division, the addition of
                                                            eps and rsqrtf (1 ulp)
    d(xhat_e) = rstd d(d_e) + |xhat_e| (rho + 2 u)          xhat = d rstd, what the backward recomputes from the saved row
    eps_l(y_e) = rstd |w_e| d(d_e) + |d_e rstd w_e| (rho + 4 u) + u |b_e|
    y: element_bound(want, eps_l, T);  res_out: u |want| (0 without a residual);  mean: d(mean);  rstd: rho rstd.
Backward.  g_e = dy_e w_e, c1 = sum g / D, c2 = sum g xhat / D, t_e = g_e - c1 - xhat_e c2, dx_e = rstd t_e + dres_e.
    d(c1) = acc_error(sum |g|, D) / D
    d(c2) = acc_error(sum |g xhat|, D) / D + sum |g_e| d(xhat_e) / D
    d(t_e) = d(c1) + |xhat_e| d(c2) + |c2| d(xhat_e) + 4 u (|g_e| + |c1| + |xhat_e c2|)
    eps_l(dx_e) = rstd d(t_e) + |rstd t_e| (rho + 2 u)      the last addition is inside element_bound's 2^-20 |want|
    dw_c = sum_rows dy xhat:  acc_error(sum_rows |dy xhat|, rows) + sum_rows |dy| d(xhat);  db_c: acc_error(sum |dy|, rows).
The forward's errors are carried because the backward reads the row, mean and rstd the forward kernel stored.

Causal conv, width W.  pre_t = b + sum_k w_k x_(t-(W-1)+k): K = W + 1 terms, S = |b| + sum_k |w_k x|,
    d(pre) = acc_error(S, W + 1);   y = pre: eps_l = d(pre);   y = silu(pre): eps_l = 1.1 d(pre) + silu_rel(pre) |y|.
Backward.  g_s = dy_s silu'(pre_s) (g = dy, exact, without the activation):
    d(g) = |dy| (0.5 d(pre) + dsilu_abs(pre))
    dx_t = sum_k w_k g_(t+(W-1)-k):  acc_error(sum_k |w_k g|, W) + sum_k |w_k| d(g)
    dw_(d,k) = sum_(b,s) g_s x_(s-(W-1)+k):  acc_error(sum |g x|, B L) + sum |x| d(g);   db_d: acc_error(sum |g|, B L) + sum d(g).

Gated RMSNorm, width D.  gv_e = y_e silu(z_e): d(gv_e) = |gv_e| silu_rel(z_e) (the product's rounding is the + 6's last unit).
    d(q) = acc_error(sum gv^2, D) + 2 sum |gv_e| d(gv_e);   rho = (d(q) / D) / (2 (q / D + eps)) + 2^-22
    out_e = gv_e r w_e:  eps_l = |out_e| (rho + silu_rel(z_e) + 2 u);   rstd: rho r.
Backward.  dot = sum go w gv, k = dot r^3 / D, dg_e = go_e w_e r - gv_e k, dy_e = dg_e silu(z_e), dz_e = dg_e y_e silu'(z_e).
    d(dot) = acc_error(sum |go w gv|, D) + sum |go_e w_e| d(gv_e)
    d(k)   = (r^3 / D) d(dot) + |k| (3 rho + 4 u)
    d(dg_e) = |go_e w_e r| (rho + 3 u) + |gv_e| d(k) + |k| d(gv_e) + 2 u (|go_e w_e r| + |gv_e k|)
    eps_l(dy_e) = |silu(z_e)| d(dg_e) + |dy_e| silu_rel(z_e)
    eps_l(dz_e) = |y_e silu'(z_e)| d(dg_e) + |dg_e y_e| (dsilu_abs(z_e) + 2 u M_e)
    dw_c = sum_rows go gv r:  acc_error(sum_rows |go gv r|, rows) + sum_rows |go| (|gv| r rho + r d(gv)).
"""
import torch
import torch.nn.functional as F

from gemm_bounds import FLOOR, TRANSCENDENTAL, U, acc_error, check_elements, element_bound  # noqa: F401 (re-exported)

P24 = 2.0 ** -24
F32 = torch.float32


def silu_rel(p):
    """Relative error of silu(p) (and, with two units to spare, of sigmoid(p)) as the kernels compute it."""
    return (p.abs() + 6) * P24


def _sig_m(p):
    sg = torch.sigmoid(p)
    return sg, sg * (1 + p.abs() * (1 - sg))


def dsilu(p):
    sg = torch.sigmoid(p)
    return sg * (1 + p * (1 - sg))


def dsilu_abs(p):
    """Absolute error of silu'(p) = sg (1 + p (1 - sg))."""
    return (4 * p.abs() + 8) * P24 * _sig_m(p)[1]


def check(got, want, bound, tag):
    """check_elements on tensors of any rank: rows = all leading dimensions flattened, columns = the last one."""
    n = want.shape[-1] if want.dim() else 1
    assert tuple(got.shape) == tuple(want.shape) == tuple(bound.shape), (tag, got.shape, want.shape, bound.shape)
    return check_elements(got.reshape(-1, n), want.reshape(-1, n), bound.reshape(-1, n), tag)


# ------------------------------------------------------------------------------------------------ add + LayerNorm
def layernorm(h, r, w, b, eps, y_dtype, dy=None, dres=None, dx_dtype=F32):
    """h [rows, D] (its own element type), r [rows, D] f32 or None, w, b [D] f32 (b may be None); dy [rows, D] or None
    (= zeros), dres [rows, D] f32 or None.  -> {"res", "y", "mean", "rstd", "dx", "dx32", "dw", "db"}: (want, bound), the
    vectors as [rows, 1] / [1, D]; "dx" is rounded to dx_dtype (hidden's gradient), "dx32" to f32 (the residual's)."""
    v = h.double() if r is None else h.double() + r.double()
    rows, D = v.shape
    wd = w.double()
    bd = torch.zeros_like(wd) if b is None else b.double()
    mean = v.mean(1, keepdim=True)
    d = v - mean
    var = (d * d).mean(1, keepdim=True)
    rstd = (var + eps).rsqrt()
    xhat = d * rstd
    y = xhat * wd + bd
    d_mean = acc_error(v.abs().sum(1, keepdim=True), D) / D
    d_d = d_mean + P24 * (v.abs() + d.abs())
    d_q = acc_error((d * d).sum(1, keepdim=True), D) + 2 * (d.abs() * d_d).sum(1, keepdim=True)
    rho = 0.5 * (d_q / D) / (var + eps) + 2.0 ** -22
    d_xhat = rstd * d_d + xhat.abs() * (rho + 2 * P24)
    eps_y = rstd * wd.abs() * d_d + (xhat * wd).abs() * (rho + 4 * P24) + P24 * bd.abs()
    out = {"res": (v, P24 * v.abs() if r is not None else torch.zeros_like(v)),
           "y": (y, element_bound(y, eps_y, y_dtype)),
           "mean": (mean, d_mean + P24 * mean.abs()),
           "rstd": (rstd, rho * rstd)}
    dyd = torch.zeros_like(v) if dy is None else dy.double()
    g = dyd * wd
    c1 = g.mean(1, keepdim=True)
    c2 = (g * xhat).mean(1, keepdim=True)
    t = g - c1 - xhat * c2
    dx = rstd * t + (0 if dres is None else dres.double())
    d_c1 = acc_error(g.abs().sum(1, keepdim=True), D) / D
    d_c2 = acc_error((g * xhat).abs().sum(1, keepdim=True), D) / D + (g.abs() * d_xhat).sum(1, keepdim=True) / D
    d_t = d_c1 + xhat.abs() * d_c2 + c2.abs() * d_xhat + 4 * P24 * (g.abs() + c1.abs() + (xhat * c2).abs())
    eps_dx = rstd * d_t + (rstd * t).abs() * (rho + 2 * P24)
    dw = (dyd * xhat).sum(0, keepdim=True)
    db = dyd.sum(0, keepdim=True)
    eps_dw = acc_error((dyd * xhat).abs().sum(0, keepdim=True), rows) + (dyd.abs() * d_xhat).sum(0, keepdim=True)
    eps_db = acc_error(dyd.abs().sum(0, keepdim=True), rows)
    out["dx"] = (dx, element_bound(dx, eps_dx, dx_dtype))
    out["dx32"] = (dx, element_bound(dx, eps_dx, F32))      # the f32 copy a 16-bit call writes for the residual stream
    out["dw"] = (dw, element_bound(dw, eps_dw, F32))
    out["db"] = (db, element_bound(db, eps_db, F32))
    return out


# ------------------------------------------------------------------------------------------------ causal conv
def _taps(x, W):
    """x (B, D, L) -> [W] of (B, D, L): tap k holds x at time t - (W - 1) + k (zero before the start)."""
    L = x.shape[-1]
    xp = F.pad(x, (W - 1, 0))
    return [xp[..., k:k + L] for k in range(W)]


def conv(x, w, b, silu, dtype, dy=None):
    """x, dy (B, D, L) of `dtype`, w (D, W), b (D) or None, f32.  -> {"y", "dx", "dw", "db"}: (want, bound); dw as
    (D, W), db as (1, D)."""
    xd, wd = x.double(), w.double()
    B, D, L = xd.shape
    W = wd.shape[1]
    bd = torch.zeros(D, dtype=torch.float64, device=xd.device) if b is None else b.double()
    taps = _taps(xd, W)
    wk = [wd[:, k].view(1, D, 1) for k in range(W)]
    pre = bd.view(1, D, 1) + sum(wk[k] * taps[k] for k in range(W))
    S = bd.abs().view(1, D, 1) + sum((wk[k] * taps[k]).abs() for k in range(W))
    d_pre = acc_error(S, W + 1)
    if silu:
        y = F.silu(pre)
        eps_y = 1.1 * d_pre + silu_rel(pre) * y.abs()
    else:
        y, eps_y = pre, d_pre
    out = {"y": (y, element_bound(y, eps_y, dtype))}
    if dy is None:
        return out
    dyd = dy.double()
    if silu:
        g = dyd * dsilu(pre)
        d_g = dyd.abs() * (0.5 * d_pre + dsilu_abs(pre))
    else:
        g, d_g = dyd, torch.zeros_like(dyd)
    gp, dgp = F.pad(g, (0, W - 1)), F.pad(d_g, (0, W - 1))
    sl = lambda a, k: a[..., W - 1 - k:W - 1 - k + L]
    dx = sum(wk[k] * sl(gp, k) for k in range(W))
    eps_dx = acc_error(sum((wk[k] * sl(gp, k)).abs() for k in range(W)), W) + sum(wk[k].abs() * sl(dgp, k) for k in range(W))
    dw = torch.stack([(g * taps[k]).sum((0, 2)) for k in range(W)], 1)
    eps_dw = torch.stack([acc_error((g * taps[k]).abs().sum((0, 2)), B * L) + (taps[k].abs() * d_g).sum((0, 2))
                          for k in range(W)], 1)
    db = g.sum((0, 2)).view(1, D)
    eps_db = (acc_error(g.abs().sum((0, 2)), B * L) + d_g.sum((0, 2))).view(1, D)
    out["dx"] = (dx, element_bound(dx, eps_dx, dtype))
    out["dw"] = (dw, element_bound(dw, eps_dw, F32))
    out["db"] = (db, element_bound(db, eps_db, F32))
    return out


# ------------------------------------------------------------------------------------------------ gated RMSNorm
def gated_rmsnorm(y, z, w, eps, dtype, dout=None):
    """y, z, dout [rows, D] of `dtype`, w [D] f32.  -> {"out", "rstd", "dy", "dz", "dw"}: (want, bound); rstd as
    [rows, 1], dw as [1, D]."""
    yd, zd, wd = y.double(), z.double(), w.double()
    rows, D = yd.shape
    sz = F.silu(zd)
    gv = yd * sz
    d_gv = gv.abs() * silu_rel(zd)
    q = (gv * gv).sum(1, keepdim=True)
    r = (q / D + eps).rsqrt()
    d_q = acc_error(q, D) + 2 * (gv.abs() * d_gv).sum(1, keepdim=True)
    rho = 0.5 * (d_q / D) / (q / D + eps) + 2.0 ** -22
    o = gv * r * wd
    out = {"out": (o, element_bound(o, o.abs() * (rho + silu_rel(zd) + 2 * P24), dtype)), "rstd": (r, rho * r)}
    if dout is None:
        return out
    go = dout.double()
    gw = go * wd
    dot = (gw * gv).sum(1, keepdim=True)
    k = dot * r ** 3 / D
    dg = gw * r - gv * k
    dyv = dg * sz
    dzv = dg * yd * dsilu(zd)
    d_dot = acc_error((gw * gv).abs().sum(1, keepdim=True), D) + (gw.abs() * d_gv).sum(1, keepdim=True)
    d_k = r ** 3 / D * d_dot + k.abs() * (3 * rho + 4 * P24)
    d_dg = (gw * r).abs() * (rho + 3 * P24) + gv.abs() * d_k + k.abs() * d_gv + 2 * P24 * ((gw * r).abs() + (gv * k).abs())
    eps_dy = sz.abs() * d_dg + dyv.abs() * silu_rel(zd)
    eps_dz = (yd * dsilu(zd)).abs() * d_dg + (dg * yd).abs() * (dsilu_abs(zd) + 2 * P24 * _sig_m(zd)[1])
    dw = (go * gv * r).sum(0, keepdim=True)
    eps_dw = acc_error((go * gv * r).abs().sum(0, keepdim=True), rows) \
        + (go.abs() * (gv.abs() * r * rho + r * d_gv)).sum(0, keepdim=True)
    out["dy"] = (dyv, element_bound(dyv, eps_dy, dtype))
    out["dz"] = (dzv, element_bound(dzv, eps_dz, dtype))
    out["dw"] = (dw, element_bound(dw, eps_dw, F32))
    return out
