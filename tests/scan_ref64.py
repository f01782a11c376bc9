"""Selective scan (Mamba1) restated for tests that check the HIP kernels at full size: forward and explicit backward in
plain torch, float64 by default, on whatever device the inputs are on.

``oracle.mamba_ref.selective_scan_ref`` materialises (B, D, L, N)-sized graphs for autograd, which is tens of GB at the
benched shapes.  Here the forward keeps only the (B, D, N) state live, and the backward walks the reverse recurrence
over clips taken in groups, each group's stored states kept under ``state_bytes``.

Provenance: a restatement of the published algorithm (Gu & Dao, "Mamba: Linear-Time Sequence Modeling with Selective
State Spaces", 2023, section 3 / Algorithm 2), nothing copied.  With delta' = softplus(delta + bias) (threshold 20) and
A = -exp(A_log) where A is given as its log:
    h_t = exp(delta'_t A) h_{t-1} + delta'_t u_t B_t,    y_t = <C_t, h_t> + D u_t,    out_t = y_t silu(z_t).
Backward, with g_t the total gradient of h_t and a_t = exp(delta'_t A):
    g_t = dy_t C_t + a_{t+1} g_{t+1},   dC_t = sum_d dy_t h_t,   dB_t = sum_d g_t delta'_t u_t,
    d delta'_t = sum_n g_t (h_{t-1} a_t A + u_t B_t),   du_t = D dy_t + delta'_t sum_n g_t B_t,
    dA = sum_{b,t} g_t h_{t-1} a_t delta'_t   (dA_log = dA A).
"""
import torch


def softplus_thr20(x):
    """softplus with the kernels' threshold: x <= 20 ? log1p(exp(x)) : x."""
    return torch.where(x <= 20.0, torch.log1p(torch.exp(torch.clamp(x, max=20.0))), x)


def _prep(u, delta, A, B, C, D, z, delta_bias, delta_softplus, a_is_log, ct):
    """Time-major copies in the compute type: u, delta', z as (L, B, D); B, C as (L, B, N); x = delta + bias (L, B, D)."""
    tm = lambda t: None if t is None else t.to(ct).permute(2, 0, 1).contiguous()
    ut, xt, zt = tm(u), tm(delta), tm(z)
    if delta_bias is not None:
        xt = xt + delta_bias.to(ct)
    dlt = softplus_thr20(xt) if delta_softplus else xt
    A_ = A.to(ct)
    if a_is_log:
        A_ = -torch.exp(A_)
    Dv = None if D is None else D.to(ct)
    return ut, xt, dlt, zt, A_, tm(B), tm(C), Dv


def _walk(ut, dlt, A_, Bt, Ct, h, states=None):
    """Forward recurrence over (L, b, .) time-major inputs from state h (b, D, N), in place.  Returns y before the skip
    term and the gate, (L, b, D); with ``states`` (L + 1, b, D, N) every state is stored there and y is formed from them."""
    L = ut.shape[0]
    y = ut.new_zeros(ut.shape)
    if states is not None:
        states[0] = h
    for t in range(L):
        a = torch.exp(dlt[t][:, :, None] * A_)
        h.mul_(a).addcmul_((dlt[t] * ut[t])[:, :, None], Bt[t][:, None, :])
        if states is not None:
            states[t + 1] = h
        else:
            y[t] = torch.bmm(h, Ct[t][:, :, None])[..., 0]
    if states is not None and L > 0:
        Lb = L * ut.shape[1]
        y = torch.bmm(states[1:].reshape(Lb, *h.shape[1:]), Ct.reshape(Lb, -1, 1)).view(ut.shape)
    return y


def _gate(ypre, ut, zt, Dv):
    y = ypre if Dv is None else ypre + ut * Dv
    return y, (y if zt is None else y * (zt * torch.sigmoid(zt)))


def _bdl(t):
    """(L, B, X) time-major -> the (B, X, L) view callers expect."""
    return t.permute(1, 2, 0)


def selective_scan64(u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False,
                     return_last_state=False, a_is_log=False, dtype=torch.float64):
    """Forward only.  Same arguments and semantics as ``selective_scan_ref`` -- u, delta, z (B, D, L); A (D, N);
    B, C (B, N, L); D, delta_bias (D,) -- plus ``a_is_log`` (A holds A_log) and the compute ``dtype``.  Returns out
    (B, D, L) in ``dtype`` (a view of time-major storage), and last_state (B, D, N) if asked."""
    ut, _, dlt, zt, A_, Bt, Ct, Dv = _prep(u, delta, A, B, C, D, z, delta_bias, delta_softplus, a_is_log, dtype)
    L, bsz, dim = ut.shape
    h = ut.new_zeros(bsz, dim, A_.shape[1])
    _, out = _gate(_walk(ut, dlt, A_, Bt, Ct, h), ut, zt, Dv)
    out = _bdl(out)
    return (out, h) if return_last_state else out


def selective_scan64_bwd(dout, u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False,
                         a_is_log=False, dtype=torch.float64, state_bytes=4 << 30, group=None):
    """Forward and backward.  ``dout`` (B, D, L) is the gradient of out.  Clips are taken ``group`` at a time (default:
    as many as keep (L + 1) states under ``state_bytes``); the batch-summed gradients are accumulated in ``dtype``.
    Returns a dict: out, last, y_pre (before the gate, with the skip term) as (B, D, L) / (B, D, N), and du, ddelta, dz
    (B, D, L), dA (dA_log with ``a_is_log``) (D, N), dB, dC (B, N, L), dD, ddelta_bias (D,); None for absent operands."""
    ut, xt, dlt, zt, A_, Bt, Ct, Dv = _prep(u, delta, A, B, C, D, z, delta_bias, delta_softplus, a_is_log, dtype)
    dot = dout.to(dtype).permute(2, 0, 1).contiguous()
    L, bsz, dim = ut.shape
    N = A_.shape[1]
    elt = torch.empty((), dtype=dtype).element_size()
    if group is None:
        group = max(1, min(bsz, state_bytes // max(1, (L + 1) * dim * N * elt)))
    new = lambda *s: ut.new_zeros(*s)
    r = {k: new(L, bsz, dim) for k in ("out", "y_pre", "du", "ddelta")}
    r["dz"] = new(L, bsz, dim) if zt is not None else None
    r["dB"], r["dC"] = new(L, bsz, N), new(L, bsz, N)
    r["last"] = new(bsz, dim, N)
    dA, dD, dbias = new(dim, N), new(dim), new(dim)
    for b0 in range(0, bsz, group):
        sl = slice(b0, min(bsz, b0 + group))
        u_, dl_, B_, C_, do_ = ut[:, sl], dlt[:, sl], Bt[:, sl], Ct[:, sl], dot[:, sl]
        z_ = None if zt is None else zt[:, sl]
        g = u_.shape[1]
        H = u_.new_empty(L + 1, g, dim, N)
        h = u_.new_zeros(g, dim, N)
        ypre = _walk(u_, dl_, A_, B_, C_, h, states=H)
        y, out = _gate(ypre, u_, z_, Dv)
        r["out"][:, sl], r["y_pre"][:, sl], r["last"][sl] = out, y, h
        if z_ is not None:
            sz = torch.sigmoid(z_)
            dy = do_ * (z_ * sz)
            r["dz"][:, sl] = do_ * y * sz * (1 + z_ * (1 - sz))
        else:
            dy = do_
        du = r["du"][:, sl]
        if Dv is not None:
            dD += (dy * u_).sum((0, 1))
            du += dy * Dv
        if L == 0:
            continue
        Lb = L * g
        # dC_t = sum_d dy_t h_t over every step at once
        r["dC"][:, sl] = torch.bmm(H[1:].reshape(Lb, dim, N).transpose(1, 2), dy.reshape(Lb, dim, 1)).view(L, g, N)
        gs = u_.new_zeros(g, dim, N)
        dAg = u_.new_zeros(g, dim, N)
        a_next = None
        ddl = r["ddelta"][:, sl]
        for t in range(L - 1, -1, -1):
            if a_next is not None:
                gs.mul_(a_next)
            gs.addcmul_(dy[t][:, :, None], C_[t][:, None, :])
            a = torch.exp(dl_[t][:, :, None] * A_)
            gh = gs * H[t] * a                                      # d(delta'_t A) per state
            s = torch.bmm(gs, B_[t][:, :, None])[..., 0]           # sum_n g_t B_t
            ddl[t] = (gh * A_).sum(-1) + s * u_[t]
            du[t] += s * dl_[t]
            r["dB"][t, sl] = torch.bmm(gs.transpose(1, 2), (dl_[t] * u_[t])[:, :, None])[..., 0]
            dAg.addcmul_(gh, dl_[t][:, :, None])
            a_next = a
        dA += dAg.sum(0)
        del H
    if delta_softplus:
        r["ddelta"] *= torch.where(xt <= 20.0, torch.sigmoid(xt), torch.ones_like(xt))
    if delta_bias is not None:
        dbias = r["ddelta"].sum((0, 1))
    res = {k: (_bdl(v) if v is not None else None) for k, v in r.items() if k != "last"}
    res["last"] = r["last"]
    res.update(dA=dA * A_ if a_is_log else dA, dD=dD if Dv is not None else None,
               ddelta_bias=dbias if delta_bias is not None else None)
    return res
