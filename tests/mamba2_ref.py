"""f64-capable restatement of mamba-ssm 2.x ``Mamba2`` (the mixer of ``CleanUMamba(mamba_v2=True)``), for tests and the
fixture generator (tools/make_golden_mamba2.py).

Provenance: mamba-ssm's source is not vendored anywhere this project can read (SURVEY section 8c says the same of
Mamba1).  This file restates the PUBLISHED algorithm -- Dao & Gu, "Transformers are SSMs" (2024), section 7 / the
``Mamba2`` module as documented -- and nothing is copied.  The layout was checked against the shipped checkpoint
``Experiment_CleanU_Mamba2.pkl`` (in_proj 296 x 64 = 2 * 128 + 2 * 16 + 8, conv1d 160 channels, dt_bias / A_log / D
per head, norm.weight 128) and by the anchor of DESIGN.md (a wrong z / x split of in_proj moves the model's output far
from its Mamba1 sibling's).  Two details the anchor does NOT resolve rest on upstream's documented semantics:
  * ``xBC`` splits as ``x, B, C`` in that order (d_ssm, d_state, d_state);
  * ``RMSNormGated(norm_before_gate=False)``: out = rmsnorm(y * silu(z)) * w, one group over d_ssm, eps 1e-5.

Per head h (ngroups 1): dt = softplus(dt_raw + dt_bias), A = -exp(A_log),
    h_t = exp(dt_t A) h_{t-1} + dt_t x_t B_t^T      (headdim x d_state),   y_t = h_t C_t + D x_t.
Everything is sequential, plain torch, dtype-agnostic (tests run it in float64 and differentiate through it).
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F


def ssd_ref(x, dt_raw, A_log, B, C, D, dt_bias, h0=None, return_state=False):
    """x: (b, T, H, P); dt_raw: (b, T, H); B, C: (b, T, N); A_log, D, dt_bias: (H,).  Returns y (b, T, H, P)."""
    b, T, H, P = x.shape
    N = B.shape[-1]
    dt = F.softplus(dt_raw + dt_bias)
    A = -torch.exp(A_log)
    h = x.new_zeros(b, H, P, N) if h0 is None else h0
    ys = []
    for t in range(T):
        da = torch.exp(dt[:, t] * A)                                            # (b, H)
        h = h * da[:, :, None, None] + (dt[:, t, :, None] * x[:, t])[..., None] * B[:, t, None, None, :]
        ys.append(torch.einsum("bhpn,bn->bhp", h, C[:, t]) + D[:, None] * x[:, t])
    y = torch.stack(ys, 1) if ys else x.new_zeros(x.shape)
    return (y, h) if return_state else y


def gated_rmsnorm_ref(y, z, w, eps=1e-5):
    g = y * F.silu(z)
    return g * torch.rsqrt(g.pow(2).mean(-1, keepdim=True) + eps) * w


def causal_conv_silu_ref(x, w, b):
    """x: (B, L, C) channels last; w: (C, W); depthwise causal conv + bias + SiLU."""
    W = w.shape[1]
    y = F.conv1d(F.pad(x.transpose(1, 2), (W - 1, 0)), w.unsqueeze(1), b, groups=w.shape[0])
    return F.silu(y).transpose(1, 2)


def mixer_ref(sd, prefix, u, headdim, eps=1e-5):
    """Mamba2.forward from a state dict: u (B, L, d_model) -> (B, L, d_model)."""
    W_in = sd[prefix + "in_proj.weight"]
    nheads = sd[prefix + "A_log"].shape[0]
    d_ssm = nheads * headdim
    N = (W_in.shape[0] - 2 * d_ssm - nheads) // 2
    zxbcdt = u @ W_in.t()
    z, xBC, dt = torch.split(zxbcdt, [d_ssm, d_ssm + 2 * N, nheads], dim=-1)
    xBC = causal_conv_silu_ref(xBC, sd[prefix + "conv1d.weight"].squeeze(1), sd[prefix + "conv1d.bias"])
    x, Bm, Cm = torch.split(xBC, [d_ssm, N, N], dim=-1)
    y = ssd_ref(x.reshape(*x.shape[:2], nheads, headdim), dt, sd[prefix + "A_log"], Bm, Cm, sd[prefix + "D"],
                sd[prefix + "dt_bias"]).reshape(*x.shape[:2], d_ssm)
    y = gated_rmsnorm_ref(y, z, sd[prefix + "norm.weight"], eps)
    return y @ sd[prefix + "out_proj.weight"].t()


def step_ref(zxbcdt, conv_state, ssm_state, conv_w, conv_b, dt_bias, A_log, D, norm_w, eps=1e-5):
    """Mamba2.step between in_proj and out_proj.  zxbcdt: (S, d_in_proj); conv_state (S, conv_dim, W) and ssm_state
    (S, H, P, N) are updated in place; returns the gated-norm output (S, d_ssm)."""
    H, P, N = ssm_state.shape[1:]
    d_ssm = H * P
    z, xBC, dt = torch.split(zxbcdt, [d_ssm, d_ssm + 2 * N, H], dim=-1)
    conv_state.copy_(torch.roll(conv_state, shifts=-1, dims=-1))
    conv_state[:, :, -1] = xBC
    xBC = F.silu((conv_state * conv_w).sum(-1) + conv_b)
    x, Bv, Cv = torch.split(xBC, [d_ssm, N, N], dim=-1)
    dt = F.softplus(dt + dt_bias)
    A = -torch.exp(A_log)
    x = x.reshape(-1, H, P)
    ssm_state.copy_(ssm_state * torch.exp(dt * A)[:, :, None, None]
                    + torch.einsum("bh,bn,bhp->bhpn", dt, Bv, x))
    y = torch.einsum("bhpn,bn->bhp", ssm_state, Cv) + D[:, None] * x
    return gated_rmsnorm_ref(y.reshape(-1, d_ssm), z, norm_w, eps)


class RMSNormGated(nn.Module):
    def __init__(self, hidden_size, eps=1e-5, device=None, dtype=None):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(hidden_size, device=device, dtype=dtype))
        self.register_parameter("bias", None)

    def forward(self, x, z):
        return gated_rmsnorm_ref(x, z, self.weight, self.eps)


class Mamba2(nn.Module):
    """Parameters, their registration order and their RNG draws as upstream's ``Mamba2.__init__`` (ngroups 1,
    rmsnorm, norm_before_gate False, no bias, conv bias, d_mlp 0): in_proj, conv1d, dt_bias, A_log, D, norm, out_proj."""

    def __init__(self, d_model, d_state=128, d_conv=4, expand=2, headdim=64, ngroups=1, A_init_range=(1, 16),
                 dt_min=0.001, dt_max=0.1, dt_init_floor=1e-4, chunk_size=256, use_mem_eff_path=True, layer_idx=None,
                 device=None, dtype=None):
        fk = {"device": device, "dtype": dtype}
        super().__init__()
        assert ngroups == 1
        self.d_model, self.d_state, self.d_conv, self.expand = d_model, d_state, d_conv, expand
        self.d_inner = self.d_ssm = expand * d_model
        self.headdim = headdim
        self.nheads = self.d_ssm // headdim
        self.ngroups = 1
        self.layer_idx = layer_idx
        self.in_proj = nn.Linear(d_model, 2 * self.d_inner + 2 * d_state + self.nheads, bias=False, **fk)
        conv_dim = self.d_ssm + 2 * d_state
        self.conv1d = nn.Conv1d(conv_dim, conv_dim, d_conv, groups=conv_dim, padding=d_conv - 1, bias=True, **fk)
        self.act = nn.SiLU()
        dt = torch.exp(torch.rand(self.nheads, **fk) * (math.log(dt_max) - math.log(dt_min)) + math.log(dt_min))
        dt = torch.clamp(dt, min=dt_init_floor)
        self.dt_bias = nn.Parameter(dt + torch.log(-torch.expm1(-dt)))
        self.dt_bias._no_weight_decay = True
        A = torch.empty(self.nheads, dtype=torch.float32, device=device).uniform_(*A_init_range)
        self.A_log = nn.Parameter(torch.log(A).to(dtype=dtype))
        self.A_log._no_weight_decay = True
        self.D = nn.Parameter(torch.ones(self.nheads, device=device))
        self.D._no_weight_decay = True
        self.norm = RMSNormGated(self.d_ssm, eps=1e-5, **fk)
        self.out_proj = nn.Linear(self.d_inner, d_model, bias=False, **fk)

    def forward(self, u, inference_params=None):
        sd = {k: v for k, v in self.state_dict().items()}
        return mixer_ref(sd, "", u, self.headdim)
