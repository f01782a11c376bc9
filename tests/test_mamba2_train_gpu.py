"""Training a Mamba2-bottleneck model (mamba_v2=True) on the GPU: gradients of the bottleneck in f32 / f16 / bf16 and of
one f16-autocast TrainStep of an E8-shaped model against f32 autograd through the f64-capable restatement
(tests/mamba2_ref.py), and the captured train step against the eager one in f32, f16 and bf16."""
import copy

import pytest
import torch
import torch.nn.functional as F

from conftest import load_ckpt, record, rel_l2
from oracle import synth
import mamba2_ref as M2

pytestmark = pytest.mark.gpu

# E8 with the Mamba2 bottleneck: d_model 512, 8 heads -> headdim 64, d_state 64, d_inner 2048 (32 heads)
E8_M2 = dict(channels_input=1, channels_output=1, channels_H=64, max_H=768, encoder_n_layers=8, kernel_size=4,
             stride=2, tsfm_n_layers=3, tsfm_n_head=8, tsfm_d_model=512, tsfm_d_inner=2048, mamba_v2=True)


def _oracle_mixers(net):
    """Replace every Mamba2 mixer's forward by the restatement (plain torch ops in f32, differentiated by autograd)."""
    for blk in net.tsfm_Mamba_layers:
        m = blk.mixer

        def fwd(u, inference_params=None, m=m):
            return M2.mixer_ref(dict(m.named_parameters()), "", u.float(), m.headdim, m.norm.eps)
        m.forward = fwd
    return net


def _e8_pair(cuda):
    from cleanumamba_amd.network import Net
    torch.manual_seed(0)
    net = Net("CleanUMamba", E8_M2).to(cuda).train()
    return net, _oracle_mixers(copy.deepcopy(net))


def _blocks(model, h):
    x, res = h, None
    for blk in model.tsfm_Mamba_layers:
        x, res = blk(x, res)
    return x.float() + res


# per-tensor rel-L2 of the bottleneck gradients against the f32 restatement: f32 is an implementation difference only;
# the 16-bit bounds cover the rounding of every activation the kernels store (x, z, dt, B, C, y in 2^-11 / 2^-8)
BOTTLENECK_TOL = {None: 1e-4, torch.float16: 1e-2, torch.bfloat16: 6e-2}


@pytest.mark.parametrize("dtype", [None, torch.float16, torch.bfloat16])
def test_bottleneck_gradients_vs_restatement(cuda, dtype):
    """The three E8-shaped Mamba2 blocks (pre-norm, mixer, residual) forward + backward on the kernels against the same
    blocks with the restatement as mixer: the input gradient and every parameter gradient, tensor by tensor.  This pins
    the wiring of the mixer's backward: the conv backward into the xBC columns of d(zxbcdt), dz / d dt in their columns,
    dt_bias / A_log / D / norm.weight."""
    net, ref = _e8_pair(cuda)
    g = torch.Generator(device=cuda).manual_seed(1)
    h = torch.randn(2, 625, 512, generator=g, device=cuda)
    gout = torch.randn(2, 625, 512, generator=g, device=cuda)
    got = {}
    for tag, model, ac in (("k", net, dtype), ("r", ref, None)):
        hin = h.clone().requires_grad_(True)
        params = dict(model.tsfm_Mamba_layers.named_parameters())
        with torch.autocast("cuda", dtype=ac or torch.float16, enabled=ac is not None):
            out = _blocks(model, hin)
        grads = torch.autograd.grad(out, [hin] + list(params.values()), gout)
        got[tag] = (out.detach(), dict(zip(["input"] + list(params), grads)))
    tol = BOTTLENECK_TOL[dtype]
    assert record(f"m2_bottleneck[{dtype}].out", rel_l2(got["k"][0], got["r"][0])) < tol
    for name, want in got["r"][1].items():
        have = got["k"][1][name]
        assert have is not None and bool(torch.isfinite(have).all()), name
        assert record(f"m2_bottleneck_grad[{dtype}].{name}", rel_l2(have, want)) < tol, name


def test_train_step_f16_autocast_e8_gradients_vs_restatement(cuda):
    """One f16-autocast TrainStep micro-step (the reference's training mode: loss_fn with L1 + multi-resolution STFT,
    loss scaling, gradients into the flat buffer the optimizer reads) of the E8-shaped Mamba2 model against f32 autograd
    of the same model and loss with the restatement as bottleneck.  The whole gradient's cosine is held to the E8 f16
    bound of test_train_gpu.py (> 0.45; measured 1.00), the bottleneck parameters' to 0.9 (measured 0.999).  The last
    decoder weight's gradient gets 5e-3 (measured 1.7e-3), not the 1.8e-3 of the linear loss there: the L1 term's
    gradient is sign(y - clean), and samples whose error lies within one f16 rounding step of zero flip it -- the
    linear-loss comparison with that test's own bounds is the next test."""
    from cleanumamba_amd.training.train_step import TrainStep
    from cleanumamba_amd.util.util import loss_fn
    net, ref = _e8_pair(cuda)
    step = TrainStep(net, autocast_dtype=torch.float16, use_graph=False)
    clean, noisy = synth.waveform(2, 16000, seed=3)
    clean, noisy = clean.to(cuda), noisy.to(cuda)
    with torch.no_grad():
        step.optimizer.state_vec[3] = 1024.0        # loss scale: no overflow on the first step (scale enters below)
    step.zero_grad()
    step.micro_step(clean, noisy)
    scale = float(step.optimizer.loss_scale)
    names = [n for n, _ in net.named_parameters()]
    lo = {n: p.grad.detach().clone() / scale for n, p in net.named_parameters()}
    kw = {k: v for k, v in step.loss_cfg.items() if k != "stft_config"}
    loss = loss_fn(ref, (clean, noisy), mrstftloss=step.mrstft, **kw)[0]
    want = dict(zip(names, torch.autograd.grad(loss, list(ref.parameters()))))
    for n in names:
        assert bool(torch.isfinite(lo[n]).all()), n
    last = "decoder.7.2.weight"
    assert record("m2_trainstep_f16.last", rel_l2(lo[last], want[last])) < 5e-3
    flat_lo = torch.cat([lo[n].flatten() for n in names]).double()
    flat_want = torch.cat([want[n].flatten() for n in names]).double()
    cos = F.cosine_similarity(flat_lo, flat_want, dim=0).item()
    assert record("m2_trainstep_f16.cos_all", cos) > 0.45
    mix = [n for n in names if ".mixer." in n]
    cos_mix = F.cosine_similarity(torch.cat([lo[n].flatten() for n in mix]).double(),
                                  torch.cat([want[n].flatten() for n in mix]).double(), dim=0).item()
    assert record("m2_trainstep_f16.cos_mixer", cos_mix) > 0.9
    for n in ("tsfm_Mamba_layers.0.mixer.dt_bias", "tsfm_Mamba_layers.0.mixer.A_log", "tsfm_Mamba_layers.0.mixer.D"):
        record(f"m2_trainstep_f16.{n}", rel_l2(lo[n], want[n]))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_autocast_gradients_e8_vs_restatement(cuda, dtype):
    """test_train_gpu.py::test_autocast_gradients_vs_reference for the E8-shaped Mamba2 model, with its bounds: a 16-bit
    autocast forward + backward of the linear loss <y, clean> against f32 autograd with the restatement as bottleneck.
    The last decoder weight (no ReLU behind it) 1.8e-3 f16 / 1.3e-2 bf16, the whole gradient's cosine 0.45 / 0.35."""
    net, ref = _e8_pair(cuda)
    clean, noisy = synth.waveform(2, 16000, seed=5)
    clean, noisy = clean.to(cuda), noisy.to(cuda)
    scale = 1024.0 if dtype == torch.float16 else 1.0      # fp16 activation gradients out of the subnormals
    with torch.autocast("cuda", dtype=dtype):
        y = net(noisy)
    lo = torch.autograd.grad((y.float() * clean).sum() * scale, list(net.parameters()))
    want = torch.autograd.grad((ref(noisy) * clean).sum(), list(ref.parameters()))
    names = [n for n, _ in net.named_parameters()]
    i = names.index("decoder.7.2.weight")
    last_tol, cos_min = {torch.float16: (1.8e-3, 0.45), torch.bfloat16: (1.3e-2, 0.35)}[dtype]
    assert all(bool(torch.isfinite(g).all()) for g in lo)
    assert record(f"m2_autocast_grad_last[{dtype}]", rel_l2(lo[i] / scale, want[i])) < last_tol
    cos = F.cosine_similarity(torch.cat([g.flatten() for g in lo]).double(),
                              torch.cat([g.flatten() for g in want]).double(), dim=0).item()
    assert record(f"m2_autocast_grad_cos[{dtype}]", cos) > cos_min


def _net_m2(cuda):
    from cleanumamba_amd.network import CleanUMamba
    sd, cfg = load_ckpt("mamba2")
    net = CleanUMamba(**cfg)
    net.load_state_dict(sd, strict=True)
    return net.to(cuda).train()


@pytest.mark.parametrize("dtype", [None, torch.float16, torch.bfloat16])
def test_mamba2_graph_replay_equals_eager_steps(cuda, dtype):
    """The captured train step of the Mamba2 checkpoint against the same steps run eagerly, in f32 and both autocast
    types: same parameters step after step, the parameters move (the Mamba2 ones included), losses finite and equal."""
    from cleanumamba_amd.training.train_step import TrainStep
    nets = [_net_m2(cuda), _net_m2(cuda)]
    before = {n: p.detach().clone() for n, p in nets[0].named_parameters()}
    steps = [TrainStep(nets[0], optimization={"n_iters": 200}, autocast_dtype=dtype, use_graph=True),
             TrainStep(nets[1], optimization={"n_iters": 200}, autocast_dtype=dtype, use_graph=False)]
    losses = [[], []]
    for it in range(8):
        clean, noisy = synth.waveform(2, 8000, seed=20 + it)
        for k in range(2):
            loss, gn = steps[k](clean.to(cuda), noisy.to(cuda))
            losses[k].append(float(loss))
    assert steps[0].graph_status == "captured", steps[0].graph_status
    assert steps[1].graph_status == "off"
    for (ka, pa), (kb, pb) in zip(nets[0].named_parameters(), nets[1].named_parameters()):
        assert rel_l2(pa, pb) < 1e-6, ka
    assert all(l == l for l in losses[0])
    assert max(abs(a - b) for a, b in zip(*losses)) < 1e-5 * max(losses[1])
    for n in ("tsfm_Mamba_layers.0.mixer.dt_bias", "tsfm_Mamba_layers.0.mixer.A_log", "tsfm_Mamba_layers.0.mixer.D",
              "tsfm_Mamba_layers.0.mixer.norm.weight", "tsfm_Mamba_layers.0.mixer.conv1d.weight"):
        assert not torch.equal(before[n], dict(nets[0].named_parameters())[n].detach()), n
