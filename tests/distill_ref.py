"""The teacher branch of the reference's loss_fn (src/util/util.py:272-289) restated in torch ops, at any dtype and on any
device: what cleanumamba_amd/training/distill.py is tested against.  Plain torch; no kernel of the project runs here.

``kd_chain`` is the literal chain on features that are already there; ``embedded_chain`` is the same chain behind the
embed (the kernels' own input); ``cpu_twin`` gives a model of the project a plain-torch CPU copy at any dtype (the Mamba
mixers become oracle/mamba_ref.py's), so that whole steps have an f64 reference."""
import copy

import torch
import torch.nn as nn

from oracle import mamba_ref as M


def kd_chain(student_feats, teacher_feats, adapters, kd_p):
    """src/util/util.py:273-288 -> (kd_loss, [L_i]).  The adapters' BatchNorms move their running statistics."""
    student = [ad["bn_s"](ad["embed"](con)) for ad, con in zip(adapters, student_feats)]
    teacher = [ad["bn_t"](con) for ad, con in zip(adapters, teacher_feats)]
    kd_losses = []
    for f_s_norm, f_t_norm in zip(student, teacher):
        c_diff = f_s_norm - f_t_norm
        c_diff = torch.abs(c_diff)
        c_diff = c_diff.pow(4.0)
        kd_losses.append(torch.log(c_diff.sum()) * kd_p)
    return torch.mean(torch.stack(kd_losses)), kd_losses


def embedded_chain(e, t, kd_p, eps, momentum=0.1):
    """One layer of the chain behind the embed: e, t (B, C, T) -> (L, bn_s, bn_t) through fresh
    ``nn.BatchNorm1d(C, eps, momentum, affine=False)`` modules of the inputs' dtype in training mode."""
    C = e.shape[1]
    bn_s = nn.BatchNorm1d(C, eps=eps, momentum=momentum, affine=False, dtype=e.dtype, device=e.device).train()
    bn_t = nn.BatchNorm1d(C, eps=eps, momentum=momentum, affine=False, dtype=t.dtype, device=t.device).train()
    c_diff = torch.abs(bn_s(e) - bn_t(t)).pow(4.0)
    return torch.log(c_diff.sum()) * kd_p, bn_s, bn_t


def cpu_twin(net, cfg, dtype=torch.float64):
    """A CPU copy of ``net`` (constructor arguments ``cfg``; pruned widths follow the state dict) in ``dtype`` that runs in
    plain torch: torch conv modules instead of the fused conv stack, oracle/mamba_ref.py's Mamba as every mixer."""
    from cleanumamba_amd.network import CleanUMamba
    twin = CleanUMamba(**cfg)
    twin.load_pruned_state_dict({k: v.detach().cpu().clone() for k, v in net.state_dict().items()})
    for layer in twin.tsfm_Mamba_layers:
        m = layer.mixer
        ref = M.Mamba(m.d_model, d_state=m.d_state, d_conv=m.d_conv, expand=m.expand, dt_rank=m.dt_rank,
                      layer_idx=m.layer_idx)
        for name, child in list(ref.named_children()):
            if isinstance(child, (nn.Linear, nn.Conv1d)):
                setattr(ref, name, copy.deepcopy(getattr(m, name)))
        ref.A_log, ref.D = copy.deepcopy(m.A_log), copy.deepcopy(m.D)
        ref.d_inner, ref.d_state, ref.dt_rank = m.d_inner, m.d_state, m.dt_rank
        layer.mixer = ref
    twin.use_fused_convs = False
    return twin.to(dtype).train(net.training)
