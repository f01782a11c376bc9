"""Mamba2 mixer over the HIP kernels (``CleanUMamba(mamba_v2=True)``).

Module contract of mamba-ssm 2.x ``mamba_ssm.modules.mamba2.Mamba2`` as the reference builds it
(src/network/CleanUMamba.py:146-149: ``layer="Mamba2"``, ``headdim = d_model // n_head``, ``use_mem_eff_path=False``):
sub-modules ``in_proj`` (nn.Linear, no bias), ``conv1d`` (depthwise over xBC, with bias), ``norm`` (RMSNormGated, weight
only), ``out_proj`` (nn.Linear, no bias) and the per-head parameters ``dt_bias``, ``A_log``, ``D``; ngroups 1, d_mlp 0.
The arithmetic, restated in tests/mamba2_ref.py:
    zxbcdt = in_proj(u) = [z (d_ssm) | xBC (d_ssm + 2 d_state) | dt (nheads)]
    xBC = silu(causal depthwise conv1d(xBC));  x, B, C = split(xBC)
    y = chunked SSD scan (per head: h_t = exp(dt_t A) h_{t-1} + dt_t x_t B_t^T, y_t = h_t C_t + D x_t)
    out = out_proj(rmsnorm(y * silu(z)) * norm.weight)

Kernels: the projections on the library's GEMMs (_proj, as Mamba1), the conv on cum_causal_conv1d_fwd/bwd, the scan and
the gated norm on csrc/ssd.hip (one autograd node, _Mamba2CoreFn), the streaming step on cum_ssd_step (one launch per
block and token between the two projection GEMMs).
"""
import ctypes
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import hip
from ...causal_conv1d import causal_conv1d_fn
from .mamba_simple import _proj


def _ssd_shape(x, dt, B, C, y, nheads, headdim, dstate):
    """cum_ssd_shape of (batch, len, .) row-strided views (elements within a row contiguous)."""
    s = hip.SsdShape()
    s.batch, s.len = x.shape[0], x.shape[1]
    s.nheads, s.headdim, s.dstate = nheads, headdim, dstate
    s.x_sb, s.x_sl = x.stride(0), x.stride(1)
    s.dt_sb, s.dt_sl = dt.stride(0), dt.stride(1)
    s.B_sb, s.B_sl = B.stride(0), B.stride(1)
    s.C_sb, s.C_sl = C.stride(0), C.stride(1)
    s.y_sb, s.y_sl = y.stride(0), y.stride(1)
    s.io_dtype = hip.dtype_code(x.dtype)
    return s


def _check_core_args(xBC, zxbcdt, nheads, d_ssm, N, final_state):
    """The kernels read x / B / C from xBC and z / dt from zxbcdt with ONE element type and plain (B, L, C) row
    layouts: anything else is refused here instead of being read as garbage."""
    if xBC.dim() != 3 or zxbcdt.dim() != 3 or zxbcdt.shape[:2] != xBC.shape[:2]:
        raise ValueError(f"Mamba2 core: xBC {tuple(xBC.shape)} and zxbcdt {tuple(zxbcdt.shape)} must be (B, L, C) "
                         "with the same B and L")
    if xBC.dtype != zxbcdt.dtype or xBC.dtype not in hip.IO_TYPES:
        raise ValueError(f"Mamba2 core: xBC ({xBC.dtype}) and zxbcdt ({zxbcdt.dtype}) must share one element type "
                         "(float32, float16 or bfloat16)")
    if not (xBC.is_contiguous() and zxbcdt.is_contiguous()):
        raise ValueError("Mamba2 core: xBC and zxbcdt must be contiguous")
    if xBC.shape[2] != d_ssm + 2 * N or N < 1 or zxbcdt.shape[2] != 2 * d_ssm + 2 * N + nheads:
        raise ValueError(f"Mamba2 core: widths xBC {xBC.shape[2]} / zxbcdt {zxbcdt.shape[2]} do not fit "
                         f"{nheads} heads of d_ssm {d_ssm}")
    if final_state is not None and (final_state.dtype != torch.float32 or not final_state.is_contiguous()
                                    or final_state.numel() != xBC.shape[0] * d_ssm * N):
        raise ValueError("Mamba2 core: final_state must be a contiguous f32 (B, nheads, headdim, d_state) tensor")


class _Mamba2CoreFn(torch.autograd.Function):
    """(xBC after the conv, zxbcdt = in_proj output) -> rmsnorm(ssd(x, dt, B, C) * silu(z)) * w, as one autograd node.
    Forward: cum_ssd_fwd (keeps only the chunk-start states) + cum_gated_rmsnorm_fwd (keeps 1 / rms per row).
    Backward: cum_gated_rmsnorm_bwd writes dz straight into d(zxbcdt), cum_ssd_bwd writes d dt there and dx / dB / dC
    into d(xBC).  The xBC columns of d(zxbcdt) are zero: their gradient reaches in_proj through the conv's backward."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, xBC, zxbcdt, dt_bias, A_log, D, norm_w, headdim, eps, save, final_state):
        nheads = A_log.shape[0]
        d_ssm = nheads * headdim
        Bn, L, conv_dim = xBC.shape
        N = (conv_dim - d_ssm) // 2
        _check_core_args(xBC, zxbcdt, nheads, d_ssm, N, final_state)
        lib = hip.lib()
        cd = xBC.dtype
        dev = xBC.device
        dt = zxbcdt[..., d_ssm + conv_dim:]
        z = zxbcdt[..., :d_ssm]
        bias, Al, Dp, w = (t.detach().float().contiguous() for t in (dt_bias, A_log, D, norm_w))
        y = torch.empty(Bn, L, d_ssm, dtype=cd, device=dev)
        states = torch.empty(max(lib.cum_ssd_states_elems(Bn, L, nheads, headdim, N), 1), dtype=torch.float32,
                             device=dev)
        s = _ssd_shape(xBC, dt, xBC[..., d_ssm:], xBC[..., d_ssm + N:], y, nheads, headdim, N)
        out = torch.empty(Bn, L, d_ssm, dtype=cd, device=dev)
        rstd = torch.empty(max(Bn * L, 1), dtype=torch.float32, device=dev) if save else None
        with torch.cuda.device(dev):
            hip.check(lib.cum_ssd_fwd(ctypes.byref(s), hip.ptr(xBC), hip.ptr(dt), hip.ptr(bias), hip.ptr(Al),
                                      hip.ptr(Dp), hip.ptr(xBC[..., d_ssm:]), hip.ptr(xBC[..., d_ssm + N:]), hip.ptr(y),
                                      hip.ptr(states), hip.ptr(final_state), hip.stream_ptr()))
            hip.check(lib.cum_gated_rmsnorm_fwd(s.io_dtype, Bn * L, d_ssm, hip.ptr(y), d_ssm, hip.ptr(z),
                                                zxbcdt.stride(1), hip.ptr(w), float(eps), hip.ptr(out), d_ssm,
                                                hip.ptr(rstd), hip.stream_ptr()))
        if save:
            ctx.save_for_backward(xBC, zxbcdt, y, rstd, states, bias, Al, Dp, w)
        ctx.dims = (nheads, headdim, N, d_ssm)
        ctx.param_dtypes = (dt_bias.dtype, A_log.dtype, D.dtype, norm_w.dtype)
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dout):
        if not ctx.saved_tensors:
            raise RuntimeError("Mamba2 core backward called but the forward saved nothing")
        xBC, zxbcdt, y, rstd, states, bias, Al, Dp, w = ctx.saved_tensors
        nheads, headdim, N, d_ssm = ctx.dims
        lib = hip.lib()
        Bn, L, conv_dim = xBC.shape
        cd, dev = xBC.dtype, xBC.device
        dout = (dout if dout.dtype == cd else dout.to(cd)).contiguous()
        dzx = torch.empty_like(zxbcdt)
        dzx[..., d_ssm:d_ssm + conv_dim].zero_()
        dy = torch.empty_like(y)
        dxBC = torch.empty_like(xBC)
        dw = torch.empty(d_ssm, dtype=torch.float32, device=dev)
        dA_log, dD, dbias = (torch.empty(nheads, dtype=torch.float32, device=dev) for _ in range(3))
        wsn = torch.empty(max(lib.cum_gated_rmsnorm_bwd_workspace_elems(d_ssm), 1), dtype=torch.float32, device=dev)
        ws = torch.empty(max(lib.cum_ssd_bwd_workspace_elems(Bn, L, nheads, headdim, N), 1), dtype=torch.float32,
                         device=dev)
        dt = zxbcdt[..., d_ssm + conv_dim:]
        s = _ssd_shape(xBC, dt, xBC[..., d_ssm:], xBC[..., d_ssm + N:], y, nheads, headdim, N)
        ld = zxbcdt.stride(1)
        with torch.cuda.device(dev):
            hip.check(lib.cum_gated_rmsnorm_bwd(s.io_dtype, Bn * L, d_ssm, hip.ptr(y), d_ssm, hip.ptr(zxbcdt), ld,
                                                hip.ptr(w), hip.ptr(rstd), hip.ptr(dout), d_ssm, hip.ptr(dy), d_ssm,
                                                hip.ptr(dzx), ld, hip.ptr(dw), hip.ptr(wsn), hip.stream_ptr()))
            hip.check(lib.cum_ssd_bwd(ctypes.byref(s), hip.ptr(xBC), hip.ptr(dt), hip.ptr(bias), hip.ptr(Al),
                                      hip.ptr(Dp), hip.ptr(xBC[..., d_ssm:]), hip.ptr(xBC[..., d_ssm + N:]),
                                      hip.ptr(dy), hip.ptr(states), hip.ptr(dxBC), hip.ptr(dzx[..., d_ssm + conv_dim:]),
                                      hip.ptr(dxBC[..., d_ssm:]), dxBC.stride(0), dxBC.stride(1),
                                      hip.ptr(dxBC[..., d_ssm + N:]), dxBC.stride(0), dxBC.stride(1),
                                      hip.ptr(dA_log), hip.ptr(dD), hip.ptr(dbias), hip.ptr(ws), hip.stream_ptr()))
        tb, ta, tD, tw = ctx.param_dtypes
        return dxBC, dzx, dbias.to(tb), dA_log.to(ta), dD.to(tD), dw.to(tw), None, None, None, None


def mamba2_core(xBC, zxbcdt, dt_bias, A_log, D, norm_w, headdim, eps, final_state=None):
    """rmsnorm(ssd(x, dt, B, C) * silu(z)) * w on the HIP kernels (see _Mamba2CoreFn); xBC (B, L, conv_dim) and
    zxbcdt (B, L, d_in_proj) contiguous, same element type (f32, f16 or bf16)."""
    params = (dt_bias, A_log, D, norm_w)
    save = torch.is_grad_enabled() and (xBC.requires_grad or zxbcdt.requires_grad or any(p.requires_grad for p in params))
    return _Mamba2CoreFn.apply(xBC, zxbcdt, dt_bias, A_log, D, norm_w, headdim, eps, save, final_state)


class RMSNormGated(nn.Module):
    """Parameter holder of upstream's RMSNormGated (norm_before_gate=False, group_size = d_ssm): ``weight`` only.  The
    arithmetic runs inside the Mamba2 mixer's kernels."""

    def __init__(self, hidden_size, eps=1e-5, norm_before_gate=False, group_size=None, device=None, dtype=None):
        super().__init__()
        if norm_before_gate or (group_size is not None and group_size != hidden_size):
            raise NotImplementedError("RMSNormGated: only norm_before_gate=False over one group (Mamba2, ngroups 1)")
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(hidden_size, device=device, dtype=dtype))
        self.register_parameter("bias", None)


class Mamba2(nn.Module):
    def __init__(self, d_model, d_state=128, d_conv=4, conv_init=None, expand=2, headdim=64, d_ssm=None, ngroups=1,
                 A_init_range=(1, 16), D_has_hdim=False, rmsnorm=True, norm_before_gate=False, dt_min=0.001,
                 dt_max=0.1, dt_init_floor=1e-4, dt_limit=(0.0, float("inf")), bias=False, conv_bias=True,
                 chunk_size=256, use_mem_eff_path=True, layer_idx=None, device=None, dtype=None):
        factory_kwargs = {"device": device, "dtype": dtype}
        super().__init__()
        if (ngroups != 1 or D_has_hdim or not rmsnorm or norm_before_gate or bias or not conv_bias
                or conv_init is not None or tuple(dt_limit) != (0.0, float("inf"))):
            raise NotImplementedError("Mamba2: only the configuration CleanUMamba builds (ngroups 1, gated RMSNorm after "
                                      "the gate, no projection bias, conv bias, no dt limit)")
        self.d_model = d_model
        self.d_state = d_state
        self.d_conv = d_conv
        self.expand = expand
        self.d_inner = self.expand * self.d_model
        self.headdim = headdim
        self.d_ssm = self.d_inner if d_ssm is None else d_ssm
        assert self.d_ssm % self.headdim == 0
        self.ngroups = ngroups
        self.nheads = self.d_ssm // self.headdim
        self.rmsnorm = rmsnorm
        self.norm_before_gate = norm_before_gate
        self.dt_limit = dt_limit
        self.activation = "silu"
        self.chunk_size = chunk_size
        self.use_mem_eff_path = use_mem_eff_path
        self.layer_idx = layer_idx

        # Order: [z, x, B, C, dt]; parameters and RNG draws in upstream's order (tests/mamba2_ref.py)
        d_in_proj = 2 * self.d_inner + 2 * self.ngroups * self.d_state + self.nheads
        self.in_proj = nn.Linear(self.d_model, d_in_proj, bias=bias, **factory_kwargs)
        conv_dim = self.d_ssm + 2 * self.ngroups * self.d_state
        self.conv1d = nn.Conv1d(conv_dim, conv_dim, d_conv, groups=conv_dim, padding=d_conv - 1, bias=conv_bias,
                                **factory_kwargs)
        self.act = nn.SiLU()
        dt = torch.exp(torch.rand(self.nheads, **factory_kwargs) * (math.log(dt_max) - math.log(dt_min))
                       + math.log(dt_min))
        dt = torch.clamp(dt, min=dt_init_floor)
        self.dt_bias = nn.Parameter(dt + torch.log(-torch.expm1(-dt)))          # inverse softplus
        self.dt_bias._no_weight_decay = True
        A = torch.empty(self.nheads, dtype=torch.float32, device=device).uniform_(*A_init_range)
        self.A_log = nn.Parameter(torch.log(A).to(dtype=dtype))
        self.A_log._no_weight_decay = True
        self.D = nn.Parameter(torch.ones(self.nheads, device=device))
        self.D._no_weight_decay = True
        self.norm = RMSNormGated(self.d_ssm, eps=1e-5, norm_before_gate=False, group_size=self.d_ssm,
                                 **factory_kwargs)
        self.out_proj = nn.Linear(self.d_inner, self.d_model, bias=bias, **factory_kwargs)

    def _dims(self):
        """(d_ssm, nheads, headdim, d_state, conv_dim), read from the tensors (a loaded checkpoint decides them)."""
        nheads = self.A_log.shape[0]
        d_ssm = self.norm.weight.shape[0]
        d_state = (self.in_proj.weight.shape[0] - 2 * d_ssm - nheads) // 2
        return d_ssm, nheads, d_ssm // nheads, d_state, d_ssm + 2 * d_state

    def forward(self, hidden_states, inference_params=None):
        """hidden_states: (B, L, d_model) -> (B, L, d_model)."""
        batch, seqlen, _ = hidden_states.shape
        conv_state, ssm_state = None, None
        if inference_params is not None:
            conv_state, ssm_state = self._get_states_from_cache(inference_params, batch)
            if inference_params.seqlen_offset > 0:
                out, _, _ = self.step(hidden_states, conv_state, ssm_state)
                return out
        if not hidden_states.is_cuda:
            raise RuntimeError("cleanumamba_amd Mamba2: the mixer runs only on a ROCm GPU; there is no CPU fallback")
        d_ssm, nheads, headdim, d_state, conv_dim = self._dims()
        zxbcdt = _proj(hidden_states, self.in_proj.weight)                             # (B, L, d_in_proj)
        if not zxbcdt.is_contiguous():
            zxbcdt = zxbcdt.contiguous()
        xBC = zxbcdt[..., d_ssm:d_ssm + conv_dim].transpose(1, 2)                      # (B, conv_dim, L), channel stride 1
        if conv_state is not None:
            conv_state.copy_(F.pad(xBC, (self.d_conv - xBC.shape[-1], 0)))
        xBC = causal_conv1d_fn(xBC, self.conv1d.weight.squeeze(1), self.conv1d.bias, "silu").transpose(1, 2)
        if not xBC.is_contiguous():
            xBC = xBC.contiguous()
        y = mamba2_core(xBC, zxbcdt, self.dt_bias, self.A_log, self.D, self.norm.weight, headdim, self.norm.eps,
                        final_state=ssm_state)
        return _proj(y, self.out_proj.weight)

    def step(self, hidden_states, conv_state, ssm_state):
        """One token for every stream.  hidden_states: (B, 1, d_model) f32; states updated in place (cum_ssd_step)."""
        assert hidden_states.shape[1] == 1, "step() decodes one token at a time"
        d_ssm, nheads, headdim, d_state, conv_dim = self._dims()
        zxbcdt = _proj(hidden_states.squeeze(1), self.in_proj.weight)
        if zxbcdt.dtype != torch.float32 or zxbcdt.stride(-1) != 1:
            zxbcdt = zxbcdt.float().contiguous()
        S = zxbcdt.shape[0]
        y = torch.empty(S, d_ssm, dtype=torch.float32, device=zxbcdt.device)
        params = [p.detach() for p in (self.conv1d.weight, self.conv1d.bias, self.dt_bias, self.A_log, self.D,
                                       self.norm.weight)]
        if any(p.dtype != torch.float32 or not p.is_contiguous() for p in params):
            raise RuntimeError("Mamba2.step: the step kernel takes contiguous f32 parameters")
        cw, cb, bias, Al, Dp, w = params
        with torch.cuda.device(zxbcdt.device):
            hip.check(hip.lib().cum_ssd_step(S, d_ssm, nheads, d_state, cw.shape[-1], float(self.norm.eps),
                                             hip.ptr(zxbcdt), zxbcdt.stride(0), hip.ptr(conv_state), hip.ptr(cw),
                                             hip.ptr(cb), hip.ptr(bias), hip.ptr(Al), hip.ptr(Dp), hip.ptr(w),
                                             hip.ptr(ssm_state), hip.ptr(y), d_ssm, hip.stream_ptr()))
        out = _proj(y.to(hidden_states.dtype), self.out_proj.weight)
        return out.unsqueeze(1), conv_state, ssm_state

    def allocate_inference_cache(self, batch_size, max_seqlen, dtype=None, **kwargs):
        device = self.out_proj.weight.device
        d_ssm, nheads, headdim, d_state, conv_dim = self._dims()
        conv_state = torch.zeros(batch_size, conv_dim, self.conv1d.weight.shape[-1], device=device, dtype=torch.float32)
        ssm_state = torch.zeros(batch_size, nheads, headdim, d_state, device=device, dtype=torch.float32)
        return conv_state, ssm_state

    def _get_states_from_cache(self, inference_params, batch_size, initialize_states=False):
        assert self.layer_idx is not None
        if self.layer_idx not in inference_params.key_value_memory_dict:
            inference_params.key_value_memory_dict[self.layer_idx] = self.allocate_inference_cache(batch_size, 1)
        conv_state, ssm_state = inference_params.key_value_memory_dict[self.layer_idx]
        if initialize_states:
            conv_state.zero_()
            ssm_state.zero_()
        return conv_state, ssm_state
