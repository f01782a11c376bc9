"""create_block / _init_weights with the signatures the reference calls
(src/network/CleanUMamba.py:12, 174-189, 201-206)."""
import math
from functools import partial

import torch
import torch.nn as nn

from ..modules.mamba_simple import Block, Mamba
from ..modules.mamba2 import Mamba2


def create_block(d_model, ssm_cfg=None, norm_epsilon=1e-5, rms_norm=False, residual_in_fp32=False,
                 fused_add_norm=False, layer_idx=None, device=None, dtype=None):
    if rms_norm:
        raise NotImplementedError("rms_norm=True needs the Triton RMSNorm; the reference runs with LayerNorm "
                                  "(src/network/CleanUMamba.py:45)")
    ssm_cfg = {} if ssm_cfg is None else dict(ssm_cfg)    # (one dict serves every layer: pop from a copy)
    layer = ssm_cfg.pop("layer", "Mamba1")
    if layer not in ("Mamba1", "Mamba2"):
        raise NotImplementedError(f"ssm_cfg layer={layer!r}")
    factory_kwargs = {"device": device, "dtype": dtype}
    mixer_cls = partial(Mamba2 if layer == "Mamba2" else Mamba, layer_idx=layer_idx, **ssm_cfg, **factory_kwargs)
    norm_cls = partial(nn.LayerNorm, eps=norm_epsilon, **factory_kwargs)
    block = Block(d_model, mixer_cls, norm_cls=norm_cls, fused_add_norm=fused_add_norm,
                  residual_in_fp32=residual_in_fp32)
    block.layer_idx = layer_idx
    return block


def _init_weights(module, n_layer, initializer_range=0.02, rescale_prenorm_residual=True,
                  n_residuals_per_layer=1):
    if isinstance(module, nn.Linear):
        if module.bias is not None and not getattr(module.bias, "_no_reinit", False):
            nn.init.zeros_(module.bias)
    elif isinstance(module, nn.Embedding):
        nn.init.normal_(module.weight, std=initializer_range)
    if rescale_prenorm_residual:
        # residual-branch output projections: kaiming-uniform then / sqrt(n_layer)
        for name, p in module.named_parameters():
            if name in ["out_proj.weight", "fc2.weight"]:
                nn.init.kaiming_uniform_(p, a=math.sqrt(5))
                with torch.no_grad():
                    p /= math.sqrt(n_residuals_per_layer * n_layer)
