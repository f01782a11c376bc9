"""Fixtures of the Mamba2 bottleneck (CleanUMamba(mamba_v2=True)).  BUILD MACHINE ONLY: it reads the reference checkout.

The reference's CleanUMamba class is imported unmodified through oracle.reference_shim.load_reference().  Before that,
``sys.modules`` stand-ins for mamba-ssm are registered here whose ``create_block`` dispatches on ``ssm_cfg["layer"]``:
"Mamba2" -> the f64 restatement tests/mamba2_ref.py, anything else -> oracle/mamba_ref.py's Mamba1 (the shim only adds
modules that are missing, so these stay in place).  Writes:
  tests/golden/ckpt_mamba2.npz   Experiment_CleanU_Mamba2.pkl in the format of oracle/make_golden.save_ckpt
  tests/golden/e2e_mamba2.npz    reference-class f64 output on fixed inputs (L = 16 000 and 4 099), the anchor input and
                                 the Mamba1 sibling's (442k) output on it, and a seeded small model's initial state dict
  tests/golden/mamba2_ops.npz    op-level vectors: SSD forward + every gradient, one step, at odd shapes
Usage: python tools/make_golden_mamba2.py
"""
import json
import os
import sys
import types
from functools import partial

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import mamba_ref, reference_shim  # noqa: E402
import mamba2_ref as M2  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
CKPTS = os.path.join(reference_shim.REFERENCE_ROOT, "checkpoints", "experiments")
# the seeded-construction check: a small config (the fixture stays a few kB)
INIT_CFG = {"channels_H": 8, "max_H": 16, "encoder_n_layers": 3, "tsfm_d_model": 32, "tsfm_n_head": 2,
            "tsfm_d_inner": 64, "tsfm_n_layers": 2, "mamba_v2": True}
INIT_SEED = 20240607


def create_block(d_model, ssm_cfg=None, norm_epsilon=1e-5, rms_norm=False, residual_in_fp32=False,
                 fused_add_norm=False, layer_idx=None, device=None, dtype=None):
    cfg = dict(ssm_cfg or {})
    if cfg.pop("layer", "Mamba1") != "Mamba2":
        return mamba_ref.create_block(d_model, ssm_cfg=cfg, norm_epsilon=norm_epsilon, rms_norm=rms_norm,
                                      residual_in_fp32=residual_in_fp32, fused_add_norm=fused_add_norm,
                                      layer_idx=layer_idx, device=device, dtype=dtype)
    fk = {"device": device, "dtype": dtype}
    block = mamba_ref.Block(d_model, partial(M2.Mamba2, layer_idx=layer_idx, **cfg, **fk),
                            norm_cls=partial(nn.LayerNorm, eps=norm_epsilon, **fk), fused_add_norm=fused_add_norm,
                            residual_in_fp32=residual_in_fp32)
    block.layer_idx = layer_idx
    return block


def install_stand_ins():
    def _mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
    _mod("mamba_ssm")
    _mod("mamba_ssm.models")
    _mod("mamba_ssm.models.mixer_seq_simple", create_block=create_block, _init_weights=mamba_ref._init_weights)
    _mod("mamba_ssm.utils")
    _mod("mamba_ssm.utils.generation", InferenceParams=mamba_ref.InferenceParams)


def npf(t):
    return t.detach().cpu().numpy()


def load_ckpt(ref, fname):
    ck = torch.load(os.path.join(CKPTS, fname), map_location="cpu", weights_only=False)
    net = ref.CleanUMamba(**ck["network_config"])
    net.load_state_dict(ck["model_state_dict"], strict=True)
    return ck, net.double().eval()


def anchor_input():
    """1 s of a 440 Hz sine plus white noise at 0.3 (fixed seed).  (with a five-harmonic 220 Hz tone the
    z / x swap of in_proj lands as close to the Mamba1 output as the right split; with this input it does not.)"""
    g = torch.Generator().manual_seed(7)
    t = torch.arange(16000, dtype=torch.float64) / 16000
    clean = torch.sin(2 * torch.pi * 440 * t)
    return (clean + 0.3 * torch.randn(16000, generator=g, dtype=torch.float64)).view(1, 1, -1)


def rel(a, b):
    return float((a - b).norm() / b.norm())


def make_ops():
    g = torch.Generator().manual_seed(11)
    out = {}
    for i, (b, T, H, P, N) in enumerate([(2, 37, 3, 16, 16), (1, 70, 2, 32, 64), (3, 5, 2, 64, 32)]):
        x = torch.randn(b, T, H, P, generator=g, dtype=torch.float64, requires_grad=True)
        dt = torch.randn(b, T, H, generator=g, dtype=torch.float64).mul(0.5).sub(1.0).requires_grad_()
        Bm = torch.randn(b, T, N, generator=g, dtype=torch.float64, requires_grad=True)
        Cm = torch.randn(b, T, N, generator=g, dtype=torch.float64, requires_grad=True)
        A_log = torch.log(torch.rand(H, generator=g, dtype=torch.float64) * 15 + 1).requires_grad_()
        D = torch.randn(H, generator=g, dtype=torch.float64, requires_grad=True)
        bias = torch.randn(H, generator=g, dtype=torch.float64).mul(0.5).requires_grad_()
        y = M2.ssd_ref(x, dt, A_log, Bm, Cm, D, bias)
        dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        y.backward(dy)
        for k, v in dict(x=x, dt=dt, B=Bm, C=Cm, A_log=A_log, D=D, dt_bias=bias).items():
            out[f"ssd{i}_{k}"] = npf(v)
            out[f"ssd{i}_d{k}"] = npf(v.grad)
        out[f"ssd{i}_y"], out[f"ssd{i}_dy"] = npf(y), npf(dy)
    # one step: 3 streams, 2 heads of 16, d_state 16, width 4, from non-zero states
    S, H, P, N, W = 3, 2, 16, 16, 4
    d_ssm, conv_dim = H * P, H * P + 2 * N
    t = {"zxbcdt": torch.randn(S, 2 * d_ssm + 2 * N + H, generator=g, dtype=torch.float64),
         "conv_state": torch.randn(S, conv_dim, W, generator=g, dtype=torch.float64),
         "ssm_state": torch.randn(S, H, P, N, generator=g, dtype=torch.float64),
         "conv_w": torch.randn(conv_dim, W, generator=g, dtype=torch.float64) * 0.5,
         "conv_b": torch.randn(conv_dim, generator=g, dtype=torch.float64) * 0.1,
         "dt_bias": torch.randn(H, generator=g, dtype=torch.float64) * 0.5,
         "A_log": torch.log(torch.rand(H, generator=g, dtype=torch.float64) * 15 + 1),
         "D": torch.randn(H, generator=g, dtype=torch.float64),
         "norm_w": 1 + 0.1 * torch.randn(d_ssm, generator=g, dtype=torch.float64)}
    for k, v in t.items():
        out["step_" + k] = npf(v)
    cs, ss = t["conv_state"].clone(), t["ssm_state"].clone()
    out["step_out"] = npf(M2.step_ref(t["zxbcdt"], cs, ss, t["conv_w"], t["conv_b"], t["dt_bias"], t["A_log"], t["D"],
                                      t["norm_w"]))
    out["step_conv_state_out"], out["step_ssm_state_out"] = npf(cs), npf(ss)
    np.savez_compressed(os.path.join(OUT, "mamba2_ops.npz"), **out)


def main():
    install_stand_ins()
    ref = reference_shim.load_reference()
    ck, net = load_ckpt(ref, "Experiment_CleanU_Mamba2.pkl")
    sd = ck["model_state_dict"]
    arrs = {k: v.cpu().numpy() for k, v in sd.items()}
    arrs["__network_config__"] = np.frombuffer(json.dumps(ck["network_config"]).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(OUT, "ckpt_mamba2.npz"), **arrs)

    out = {}
    torch.manual_seed(1234)
    with torch.no_grad():
        for L in (16000, 4099):
            x = 0.1 * torch.randn(1, 1, L, dtype=torch.float64)
            out[f"input_{L}"] = npf(x)
            out[f"out_{L}"] = npf(net(x.clone()))
        xa = anchor_input()
        _, net1 = load_ckpt(ref, "Experiment_CleanU_Mamba.pkl")
        ya2, ya1 = net(xa.clone()), net1(xa.clone())
    out.update(anchor_input=npf(xa), anchor_mamba2=npf(ya2), anchor_mamba1=npf(ya1))
    print(f"anchor: rel-L2(Mamba2, Mamba1) = {rel(ya2, ya1):.3f}, rel-L2(Mamba2, input) = {rel(ya2, xa):.3f}, "
          f"rel-L2(Mamba1, input) = {rel(ya1, xa):.3f}")

    torch.manual_seed(INIT_SEED)
    small = ref.CleanUMamba(**INIT_CFG)
    for k, v in small.state_dict().items():
        out["init." + k] = npf(v)
    out["init_config"] = np.frombuffer(json.dumps(INIT_CFG).encode(), dtype=np.uint8)
    out["init_seed"] = np.int64(INIT_SEED)
    np.savez_compressed(os.path.join(OUT, "e2e_mamba2.npz"), **out)
    make_ops()
    print("done")


if __name__ == "__main__":
    main()
