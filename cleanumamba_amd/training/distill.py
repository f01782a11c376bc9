"""Distillation fine-tuning: the teacher branch of the reference's loss_fn (src/util/util.py:259-290), the feature
distillation of Miles & Mikolajczyk, arXiv:2303.11098.

For every feature ``forward(x, return_skip_connections=True)`` returns -- the E encoder skips, deepest first, then
``tsfm_out`` -- the student's feature s (B, Cs, T) and the teacher's t (B, Ct, T) give

    e = embed(s)                                   1x1 Conv1d(Cs, Ct)                       (ad["embed"], :273)
    s^ = (e - mean_e) / sqrt(var_e + eps)          BatchNorm1d(affine=False), training      (ad["bn_s"], :273)
    t^ = (t - mean_t) / sqrt(var_t + eps)                                                    (ad["bn_t"], :274)
    L_i = kd_p log sum (s^ - t^)^4                                                           (:277-282)
    kd_loss = mean_i L_i                                                                     (:288)

``make_adapters`` builds the per-layer modules as the reference indexes them; ``kd_feature_loss`` evaluates the loss.

On the GPU, with exactly these module types in training mode, every layer goes through three streaming passes of
csrc/distill.hip (statistics, loss, backward: one launch each for all layers, plus two small merge launches) instead of
the ~15 elementwise and reduction passes per layer of the eager chain and the four full-size tensors its autograd keeps.
The 1x1 embed is the projection GEMM of network/convstack.py on the channels-last rows the conv stack already holds.
Anything else -- other module types, eval mode, ``affine=True``, ``momentum=None``, the CPU -- takes the plain torch
chain (``fallback_loss``), which is the reference's lines as they stand."""
import numbers

import torch
import torch.nn as nn

from .. import hip
from ..network import convstack as cs

MAX_LAYERS = 16           # CUM_DISTILL_MAX_LAYERS: layers per launch (the E8 model has 9)


# ---------------------------------------------------------------------------------------------------------- adapters
def feature_channels(net):
    """Channel widths of the features ``net(x, return_skip_connections=True)`` returns, in their order (encoder skips
    deepest first, then tsfm_out), read from the weights -- so a pruned model reports its own widths."""
    enc = list(net.encoder)
    widths = []
    for i in range(len(enc)):
        nxt = enc[i + 1][0] if i + 1 < len(enc) else net.tsfm_conv1
        widths.append(nxt.weight.shape[1] * getattr(nxt, "groups", 1))
    return widths[::-1] + [net.tsfm_conv2.weight.shape[1]]


def make_adapters(student, teacher, eps=1e-4, momentum=0.1):
    """One ``nn.ModuleDict(embed=Conv1d(Cs_i, Ct_i, 1), bn_s=BatchNorm1d(Ct_i, affine=False), bn_t=...)`` per returned
    feature, as the reference's ``student_teacher_adapter_layers`` are indexed (src/util/util.py:273-274), on the
    student's device.  The two models must agree in depth, kernel and stride (else their features differ in length)."""
    for name in ("encoder_n_layers", "kernel_size", "stride"):
        a, b = getattr(student, name), getattr(teacher, name)
        if a != b:
            raise ValueError(f"make_adapters: student and teacher differ in {name} ({a} against {b}): their features "
                             "would differ in length")
    cs_, ct_ = feature_channels(student), feature_channels(teacher)
    p = next(student.parameters())
    kw = {"device": p.device, "dtype": p.dtype}
    return nn.ModuleList(
        nn.ModuleDict({"embed": nn.Conv1d(a, b, 1, **kw),
                       "bn_s": nn.BatchNorm1d(b, eps=eps, momentum=momentum, affine=False, **kw),
                       "bn_t": nn.BatchNorm1d(b, eps=eps, momentum=momentum, affine=False, **kw)})
        for a, b in zip(cs_, ct_))


def check_adapters(student, adapters):
    """Raise if an adapter no longer fits the student (it was pruned after the adapters were built)."""
    widths = feature_channels(student)
    if len(widths) != len(adapters):
        raise ValueError(f"distillation: {len(adapters)} adapters for a student with {len(widths)} features")
    for i, (ad, c) in enumerate(zip(adapters, widths)):
        if ad["embed"].weight.shape[1] != c:
            raise ValueError(f"distillation: adapter {i} embeds {ad['embed'].weight.shape[1]} channels but the student's "
                             f"feature has {c}: build the adapters (make_adapters) after pruning the student")


# ---------------------------------------------------------------------------------------------------------- fallback
def fallback_loss(student_feats, teacher_feats, adapters, kd_p):
    """src/util/util.py:273-288 as it stands, in torch ops: -> (kd_loss, [L_i])."""
    kd_losses = []
    for ad, s, t in zip(adapters, student_feats, teacher_feats):
        f_s = ad["bn_s"](ad["embed"](s))
        f_t = ad["bn_t"](t)
        kd_losses.append(torch.log((f_s - f_t).abs().pow(4.0).sum()) * kd_p)
    return torch.mean(torch.stack(kd_losses)), kd_losses


# ------------------------------------------------------------------------------------------------------- kernel route
def _bn_ok(bn):
    return (type(bn) is nn.BatchNorm1d and bn.training and not bn.affine and isinstance(bn.momentum, numbers.Real)
            and not isinstance(bn.momentum, bool)
            and (bn.running_mean is None or (bn.running_mean.dtype == bn.running_var.dtype == torch.float32
                                             and bn.num_batches_tracked.dtype == torch.int64)))


def _embed_ok(conv):
    return (type(conv) is nn.Conv1d and conv.kernel_size == (1,) and conv.stride == (1,) and conv.padding == (0,)
            and conv.dilation == (1,) and conv.groups == 1 and conv.bias is not None
            and conv.weight.dtype == torch.float32)


def kernel_route(student_feats, teacher_feats, adapters):
    """True where csrc/distill.hip takes the loss: everything on one GPU, the adapters exactly make_adapters' module
    types in training mode without affine parameters and with a numeric momentum."""
    feats = list(student_feats) + list(teacher_feats)
    if not feats or len(student_feats) > MAX_LAYERS:
        return False
    dev = feats[0].device
    if any(not f.is_cuda or f.device != dev or f.dtype not in hip.IO_TYPES or f.dim() != 3 for f in feats):
        return False
    for ad in adapters:
        if type(ad) is not nn.ModuleDict or set(ad.keys()) != {"embed", "bn_s", "bn_t"}:
            return False
        if not (_embed_ok(ad["embed"]) and _bn_ok(ad["bn_s"]) and _bn_ok(ad["bn_t"])):
            return False
        if any(t.device != dev for t in list(ad.parameters()) + list(ad.buffers())):
            return False
    return True


def _side(x):
    """(B, C, T) feature -> its (B, T, C) view with unit channel stride for the kernels (a view of x where x is channels
    last -- the conv stack's row buffers, tsfm_out -- and every 16-byte load the kernels would issue stays inside its
    storage; else a compact copy)."""
    v = x.detach().transpose(1, 2)
    B, T, C = v.shape
    if T == 1 and v.stride(2) == 1:       # a one-row clip: torch keeps no meaningful row stride, the clip stride serves
        v = torch.as_strided(v, v.shape, (v.stride(0), max(v.stride(0), C), 1), v.storage_offset())
    Cp = cs.rup(C, 8)
    ok = v.stride(2) == 1 and v.stride(1) >= C and (B == 1 or v.stride(0) >= (T - 1) * v.stride(1) + C)
    if ok and v.stride(1) >= Cp:       # the 16-byte path may touch the pad columns of the last row
        end = v.storage_offset() + (B - 1) * v.stride(0) + (T - 1) * v.stride(1) + Cp
        ok = end * v.element_size() <= v.untyped_storage().nbytes()
    return v if ok else v.contiguous()


class _Embedded:
    """e = embed(s) on the projection GEMM over the channels-last rows of s: what the backward needs of it."""

    def __init__(self, s, conv):
        w, b = conv.weight, conv.bias
        N, K = w.shape[0], w.shape[1]
        B, Cs, T = s.shape
        dt = s.dtype
        Kp = cs.rup(K, cs.bk_of(dt))
        sb, st = s.stride(0), s.stride(2)
        if T == 1:                        # (a one-row clip keeps no meaningful row stride)
            st = sb if B > 1 else cs.rup(K, 8)
        rows = s.stride(1) == 1 and st % 8 == 0 and st >= K and (B == 1 or (sb % st == 0 and sb >= T * st)) \
            and s.data_ptr() % 16 == 0
        if rows:
            # every row of the buffer between the first and the last real one is a GEMM row (the two rows between clips
            # hold zeros and give rows of e nobody reads); a row is read Kp wide, into its successor's finite values
            P = sb // st if B > 1 else T
            M = (B - 1) * P + T
            end = s.storage_offset() + (M - 1) * st + max(Kp, cs.rup(K, 8))
            rows = end * s.element_size() <= s.untyped_storage().nbytes()
        if rows:
            x2 = torch.as_strided(s.detach(), (M, K), (st, 1), s.storage_offset())
        else:
            P, M = T, B * T
            x2 = torch.nn.functional.pad(s.detach().transpose(1, 2).reshape(M, K), (0, Kp - K))[:, :K]
        self.x2, self.B, self.T, self.P, self.M, self.N, self.K, self.dt = x2, B, T, P, M, N, K, dt
        self.Np8, self.Kp8 = cs.rup(N, 8), cs.rup(K, 8)
        Np = cs.rup(N, 32)
        wp = cs.take(w, ("proj", (N, K), Np, Kp), lambda: cs.lay_proj((N, K), Np, Kp), dt)
        bp = cs.take(b, ("vec", N, Np), lambda: cs.lay_vec(N, Np), torch.float32)
        self.e2 = torch.empty(M, self.Np8, dtype=dt, device=s.device)
        cs.gemm(x2, 0, x2.stride(0), wp, bp, self.e2, 0, self.Np8, M, 1 << 30, 1 << 30, hip.EPI_BIAS, self.Np8)

    def view(self, buf2, C):
        """(B, T, C) view of a (M, pitch) row matrix in this layout."""
        return torch.as_strided(buf2, (self.B, self.T, C), (self.P * buf2.stride(0), buf2.stride(0), 1),
                                buf2.storage_offset())

    def new_grad(self):
        """de as the GEMMs of the backward read it: M rows of Np8 columns, then 64 readable zeros (a row is read up to the
        K tile wide, into its successor)."""
        flat = torch.empty(self.M * self.Np8 + 64, dtype=self.dt, device=self.e2.device)
        flat[self.M * self.Np8:].zero_()
        return flat[:self.M * self.Np8].view(self.M, self.Np8)

    def backward(self, de2, conv, need_ds):
        """-> (ds as a (B, Cs, T) channels-last tensor or None, dw, db); dw = db = None where the flat gradient buffer
        took them (convstack.grad_sink, as convstack.Pointwise)."""
        w, b = conv.weight, conv.bias
        N, K, M = self.N, self.K, self.M
        ldx = self.x2.stride(0)
        sink = cs.grad_sink([w, b]) if (N == self.Np8 and K == self.Kp8) else None
        if sink is not None:
            flat, idx, offs = sink
            cs.wgrad(de2, 0, self.Np8, self.Np8, self.x2, 0, ldx, self.Kp8, M,
                     out_w=flat.grad[offs[0]:offs[0] + N * K], out_b=flat.grad[offs[1]:offs[1] + N])
            flat.wrote(idx)
            dw = db = None
        else:
            dwp, dbp = cs.wgrad(de2, 0, self.Np8, self.Np8, self.x2, 0, ldx, self.Kp8, M)
            dw, db = dwp[:N, :K].unsqueeze(-1).to(w.dtype), dbp[:N].to(b.dtype)
        ds = None
        if need_ds:
            dx = torch.empty(M, self.Kp8, dtype=self.dt, device=de2.device)
            cs.proj_dgrad(de2, w.detach().view(N, K), self.dt, out=dx[:, :K], tail_ok=True)
            ds = self.view(dx, K).transpose(1, 2)
        return ds, dw, db


def _layer_record(e, t, de, bn_s, bn_t, eps, momentum):
    d = hip.DistillLayer()
    d.e, d.t, d.de = e.data_ptr(), t.data_ptr(), (de.data_ptr() if de is not None else None)
    for mod, tag in ((bn_s, "s"), (bn_t, "t")):
        if mod is not None and mod.running_mean is not None:
            setattr(d, "rm_" + tag, mod.running_mean.data_ptr())
            setattr(d, "rv_" + tag, mod.running_var.data_ptr())
            setattr(d, "nbt_" + tag, mod.num_batches_tracked.data_ptr())
    d.e_sb, d.e_st, d.t_sb, d.t_st = e.stride(0), e.stride(1), t.stride(0), t.stride(1)
    if de is not None:
        d.de_sb, d.de_st = de.stride(0), de.stride(1)
    d.B, d.T, d.C = e.shape
    d.e_dtype, d.t_dtype = hip.dtype_code(e.dtype), hip.dtype_code(t.dtype)
    d.momentum, d.eps = float(momentum), float(eps)
    return d


class _KDLoss(torch.autograd.Function):
    """[L_i] for all layers: ONE autograd node.  ``specs[i] = (embed or None, bn_s or None, bn_t or None, eps,
    momentum)``; tensors = the n student features (the embedded e itself where embed is None), the n teacher features,
    then weight and bias of every embed."""

    @staticmethod
    def forward(ctx, kd_p, specs, *tensors):
        n = len(specs)
        s_feats, t_feats = tensors[:n], tensors[n:2 * n]
        dev = s_feats[0].device
        emb, es, ts, recs = [], [], [], (hip.DistillLayer * n)()
        for i, (conv, bn_s, bn_t, eps, momentum) in enumerate(specs):
            s, t = s_feats[i], t_feats[i]
            if conv is not None and s.shape[1] != conv.weight.shape[1]:
                raise ValueError(f"distillation: adapter {i} embeds {conv.weight.shape[1]} channels but the student's "
                                 f"feature has {s.shape[1]}: build the adapters (make_adapters) after pruning the student")
            width = conv.weight.shape[0] if conv is not None else s.shape[1]
            if (s.shape[0], width, s.shape[2]) != tuple(t.shape):
                raise ValueError(f"distillation: layer {i}: student feature {tuple(s.shape)} embedded to {width} channels "
                                 f"does not match the teacher's {tuple(t.shape)}")
            if s.shape[0] * s.shape[2] < 2:
                raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(t.shape)}")
            if conv is not None:
                if s.stride(1) != 1:
                    s = s.transpose(1, 2).contiguous().transpose(1, 2)
                em = _Embedded(s, conv)
                e = em.view(em.e2, width)
            else:
                em, e = None, _side(s)
            emb.append(em)
            es.append(e)
            ts.append(_side(t))
            recs[i] = _layer_record(es[i], ts[i], None, bn_s, bn_t, eps, momentum)
        lib = hip.lib()
        sizes = (hip.c_i64 * 3)()
        with torch.cuda.device(dev):
            hip.check(lib.cum_distill_sizes(recs, n, sizes))
            part = torch.empty(max(int(sizes[0]), 4), dtype=torch.float32, device=dev)
            cst = torch.empty(int(sizes[1]) * 8, dtype=torch.float32, device=dev)
            csum = torch.empty(int(sizes[1]) * 2, dtype=torch.float64, device=dev)
            s4 = torch.empty(int(sizes[2]), dtype=torch.float32, device=dev)
            D = torch.empty(n, dtype=torch.float64, device=dev)
            L = torch.empty(n, dtype=torch.float32, device=dev)
            hip.check(lib.cum_distill_fwd(recs, n, float(kd_p), 3, hip.ptr(part), hip.ptr(cst), hip.ptr(csum), hip.ptr(s4),
                                          hip.ptr(D), hip.ptr(L), hip.stream_ptr()))
        ctx.kd_p, ctx.specs, ctx.emb, ctx.n = float(kd_p), specs, emb, n
        ctx.shapes = [tuple(s.shape) for s in s_feats]
        ctx.save_for_backward(cst, csum, D, *es, *ts)
        return L

    @staticmethod
    def backward(ctx, gL):
        n, specs, emb = ctx.n, ctx.specs, ctx.emb
        cst, csum, D = ctx.saved_tensors[:3]
        es, ts = ctx.saved_tensors[3:3 + n], ctx.saved_tensors[3 + n:3 + 2 * n]
        dev = cst.device
        G = gL.to(torch.float32).contiguous()
        recs, des = (hip.DistillLayer * n)(), []
        for i, (conv, bn_s, bn_t, eps, momentum) in enumerate(specs):
            e = es[i]
            if emb[i] is not None:
                de2 = emb[i].new_grad()
                de = emb[i].view(de2, e.shape[2])
            else:
                B, T, C = e.shape
                de2 = torch.empty(B * T, cs.rup(C, 8), dtype=e.dtype, device=dev)
                de = de2.view(B, T, -1)[:, :, :C]
            des.append((de2, de))
            # (the running statistics moved in the forward: the backward's table carries no module pointers)
            recs[i] = _layer_record(e, ts[i], de, None, None, eps, momentum)
        with torch.cuda.device(dev):
            hip.check(hip.lib().cum_distill_bwd(recs, n, ctx.kd_p, hip.ptr(cst), hip.ptr(csum), hip.ptr(D), hip.ptr(G),
                                                hip.stream_ptr()))
        g_s, g_wb = [], []
        for i, (conv, *_rest) in enumerate(specs):
            de2, de = des[i]
            if emb[i] is None:
                g_s.append(de.transpose(1, 2) if ctx.needs_input_grad[2 + i] else None)
                continue
            ds, dw, db = emb[i].backward(de2, conv, ctx.needs_input_grad[2 + i])
            g_s.append(ds)
            g_wb += [dw, db]
        return (None, None, *g_s, *([None] * n), *g_wb)


def kernel_loss(student_feats, teacher_feats, adapters, kd_p):
    """[L_i] (one f32 tensor) on csrc/distill.hip; the caller has checked ``kernel_route``."""
    specs, wb = [], []
    for ad in adapters:
        conv, bn_s, bn_t = ad["embed"], ad["bn_s"], ad["bn_t"]
        if bn_s.eps != bn_t.eps or bn_s.momentum != bn_t.momentum:
            raise ValueError("distillation: bn_s and bn_t of an adapter must share eps and momentum on the kernel route")
        specs.append((conv, bn_s, bn_t, bn_s.eps, bn_s.momentum))
        wb += [conv.weight, conv.bias]
    return _KDLoss.apply(kd_p, tuple(specs), *student_feats, *teacher_feats, *wb)


def embedded_loss(es, ts, kd_p, eps=1e-4, momentum=0.1, bn_s=None, bn_t=None):
    """The three passes alone, on features that are already embedded: es[i], ts[i] (B, C, T) -> [L_i] (one f32 tensor),
    differentiable in es.  bn_s / bn_t: lists of BatchNorm1d whose running statistics move (None: no side effect)."""
    n = len(es)
    specs = tuple((None, bn_s[i] if bn_s else None, bn_t[i] if bn_t else None, eps, momentum) for i in range(n))
    return _KDLoss.apply(kd_p, specs, *es, *ts)


def kd_feature_loss(student_feats, teacher_feats, adapters, kd_p=1):
    """-> (kd_loss, [L_i]): src/util/util.py:273-288 for the features of student and teacher (lists of (B, C, T), as
    ``forward(x, return_skip_connections=True)`` returns them) and the adapters of ``make_adapters``."""
    if not (len(student_feats) == len(teacher_feats) == len(adapters)):
        raise ValueError(f"distillation: {len(student_feats)} student features, {len(teacher_feats)} teacher features "
                         f"and {len(adapters)} adapters")
    if kernel_route(student_feats, teacher_feats, adapters):
        L = kernel_loss(student_feats, teacher_feats, adapters, kd_p)
        return L.mean(), list(L.unbind())
    return fallback_loss(student_feats, teacher_feats, adapters, kd_p)
