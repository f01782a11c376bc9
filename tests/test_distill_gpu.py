"""Teacher / student feature distillation on the GPU (csrc/distill.hip, training/distill.py, TrainStep(distill=...)).

Kernel route against tests/distill_ref.py (src/util/util.py:272-289 in torch ops) in float64 on the same values.  Nothing in
the project fixes the bound, so every case measures it: eps_ref is the error of the literal chain run in float32 on the CPU
against float64 -- absolute for the loss, rel-L2 for d/de -- and the kernels get 8 x eps_ref of that case (a different
reduction order and the extra rounding of a three-pass form).  Half buffers add the final rounding of d/de (2^-11 for f16,
2^-8 for bf16) and run with an upstream gradient of 1024, which keeps d/de out of the f16 subnormals (asserted).  Before
each call every pad column and every row between clips of the row buffers holds NaN: a finite result shows they are not
read into a sum."""
import copy

import pytest
import torch
import torch.nn as nn

from conftest import load_ckpt, record, rel_l2
from oracle import synth

import distill_ref as R

pytestmark = pytest.mark.gpu
EPS = 1e-4

#            B   C    T   mean  std   layout of e / t
CASES = {
    "c13_rows": (2, 13, 37, 0.0, 1.0, "rows", "rows"),          # C not a multiple of 8; row-buffer view with pitch 16
    "c72_chunks": (3, 72, 700, 0.0, 1.0, "rows", "rows"),       # more channels than a wave's lanes; several chunks, partial last
    "one_frame": (2, 8, 1, 0.0, 1.0, "contig", "contig"),       # tsfm_out at one frame; n = 2
    "n2": (1, 13, 2, 0.0, 1.0, "rows", "rows"),                 # smallest batch that still has two values per channel
    "offset": (3, 16, 700, 100.0, 0.1, "rows", "rows"),         # catches a sum-of-squares variance
    "mixed": (2, 13, 37, 0.0, 1.0, "rows", "contig"),           # different strides on the two sides
}
ILL = ("one_frame", "n2")                                        # n = 2: f32 only (BatchNorm's backward nearly cancels)
HALF_ROUND = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
_cache = {}


def _values(name, dtype):
    """(e, t) of the case as CPU tensors (B, C, T), already rounded to ``dtype``."""
    B, C, T, mean, std, _, _ = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    z1, z2 = torch.randn(B, C, T, generator=g), torch.randn(B, C, T, generator=g)
    e, t = (mean + std * z1).to(dtype), (mean + std * (0.6 * z1 + 0.8 * z2)).to(dtype)     # correlated, as s and t are
    return e, t


def _reference(name, dtype, G):
    """f64 chain and the f32 chain's distance to it, once per (case, dtype): (L64, de64, eps_loss, eps_grad)."""
    key = (name, dtype, G)
    if key not in _cache:
        e, t = _values(name, dtype)
        out = {}
        for wide in (torch.float64, torch.float32):
            ev = e.to(wide).requires_grad_(True)
            L, _, _ = R.embedded_chain(ev, t.to(wide), 1.0, EPS)
            (de,) = torch.autograd.grad(L, ev, torch.tensor(float(G), dtype=wide))
            out[wide] = (L.detach(), de)
        L64, de64 = out[torch.float64]
        L32, de32 = out[torch.float32]
        _cache[key] = (L64, de64, abs(float(L32) - float(L64)), rel_l2(de32, de64))
    return _cache[key]


def _lay(x, layout, cuda, fill=float("nan")):
    """CPU (B, C, T) values -> a GPU feature in ``layout``: a view of a conv-stack row buffer whose every other element is
    ``fill`` (NaN for the kernels, which must not read there; 0 as the conv stack leaves it for the embed GEMM, which
    reads whole rows), or the permuted view of a contiguous (B, T, C) tensor (tsfm_out's form)."""
    from cleanumamba_amd.network import convstack as cs
    B, C, T = x.shape
    if layout == "contig":
        return x.to(cuda).transpose(1, 2).contiguous().transpose(1, 2)
    geo = cs.Geo(B, T, C)
    buf = torch.full((geo.R, geo.Cp), fill, dtype=x.dtype, device=cuda)
    geo.rows(buf)[:, :T, :C] = x.to(cuda).transpose(1, 2)
    view = cs.from_rows(buf, geo)
    assert view.stride() == (geo.P * geo.Cp, 1, geo.Cp)
    assert fill == 0.0 or bool(torch.isnan(buf).sum() == buf.numel() - x.numel())
    return view


def _run_kernels(name, dtype, cuda, G, bns=None):
    from cleanumamba_amd.training import distill
    _, _, _, _, _, le, lt = CASES[name]
    e, t = _values(name, dtype)
    eg = _lay(e, le, cuda).requires_grad_(True)
    tg = _lay(t, lt, cuda)
    kw = {} if bns is None else {"bn_s": [bns[0]], "bn_t": [bns[1]]}
    L = distill.embedded_loss([eg], [tg], 1.0, eps=EPS, momentum=0.1, **kw)
    (de,) = torch.autograd.grad(L, eg, torch.tensor([float(G)], device=cuda))
    return L.detach()[0], de


def _params():
    for name in CASES:
        for dtype in (torch.float32, torch.float16, torch.bfloat16):
            if dtype is torch.float32 or name not in ILL:
                yield pytest.param(name, dtype, id=f"{name}-{str(dtype).split('.')[-1]}")


@pytest.mark.parametrize("name,dtype", list(_params()))
def test_kernels_match_the_f64_chain(cuda, name, dtype):
    G = 1.0 if dtype is torch.float32 else 1024.0
    L64, de64, eps_loss, eps_grad = _reference(name, dtype, G)
    L, de = _run_kernels(name, dtype, cuda, G)
    assert de.dtype == dtype and de.shape == de64.shape
    assert bool(torch.isfinite(L)) and bool(torch.isfinite(de).all())
    err_loss, err_grad = abs(float(L) - float(L64)), rel_l2(de, de64)
    tag = f"{name}-{str(dtype).split('.')[-1]}"
    print(f"distill[{tag}] loss err {err_loss:.3e} (eps_ref {eps_loss:.3e}, ratio {err_loss / max(eps_loss, 1e-300):.2f})  "
          f"grad rel-L2 {err_grad:.3e} (eps_ref {eps_grad:.3e}, ratio {err_grad / max(eps_grad, 1e-300):.2f})")
    record(f"distill_loss_ratio[{tag}]", err_loss / max(eps_loss, 1e-300))
    record(f"distill_grad_ratio[{tag}]", err_grad / max(eps_grad, 1e-300))
    if dtype is not torch.float32:
        small = float((de64.abs() < 2.0 ** -14).double().mean())
        print(f"distill[{tag}] share of |d/de| below 2^-14: {small:.4%}")
        assert small <= 0.01
    assert err_loss <= 8 * eps_loss
    assert err_grad <= 8 * eps_grad + HALF_ROUND.get(dtype, 0.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_two_runs_give_the_same_bits(cuda, dtype):
    a = _run_kernels("c72_chunks", dtype, cuda, 1024.0)
    b = _run_kernels("c72_chunks", dtype, cuda, 1024.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("name", ["c13_rows", "c72_chunks", "one_frame"])
def test_running_statistics_follow_batchnorm(cuda, name):
    """Two calls move running_mean / running_var / num_batches_tracked as nn.BatchNorm1d does (the fallback's modules, in
    f64 on the CPU).  Bound 1e-5 relative: both sides blend in one f32 operation; the kernels' batch statistics are
    Welford sums of at most 2 100 f32 values merged in f64."""
    C = CASES[name][1]
    e, t = _values(name, torch.float32)
    bns = [nn.BatchNorm1d(C, eps=EPS, momentum=0.1, affine=False).to(cuda).train() for _ in range(2)]
    ref = [nn.BatchNorm1d(C, eps=EPS, momentum=0.1, affine=False).double().train() for _ in range(2)]
    for _ in range(2):
        _run_kernels(name, torch.float32, cuda, 1.0, bns=bns)
        ref[0](e.double()), ref[1](t.double())
    for mine, want in zip(bns, ref):
        assert int(mine.num_batches_tracked) == int(want.num_batches_tracked) == 2
        torch.testing.assert_close(mine.running_mean.cpu().double(), want.running_mean, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(mine.running_var.cpu().double(), want.running_var, rtol=1e-5, atol=1e-6)


def test_fewer_than_two_values_per_channel_raises(cuda):
    from cleanumamba_amd.training import distill
    x = torch.randn(1, 8, 1, device=cuda)
    with pytest.raises(ValueError):
        distill.embedded_loss([x], [x.clone()], 1.0)


# ------------------------------------------------------------------------------------------- embed + kernels, no torch ops
def _adapters(widths, cuda, seed=3):
    torch.manual_seed(seed)
    return nn.ModuleList(nn.ModuleDict({"embed": nn.Conv1d(a, b, 1), "bn_s": nn.BatchNorm1d(b, eps=EPS, affine=False),
                                        "bn_t": nn.BatchNorm1d(b, eps=EPS, affine=False)}) for a, b in widths)


def test_kernel_route_with_embed_runs_no_torch_conv(cuda, monkeypatch):
    """kd_feature_loss in f32 on row-buffer features (two layers: odd widths 11 -> 13, and 16 -> 24) and a contiguous
    tsfm_out (8 -> 8) with F.conv1d / F.linear / F.batch_norm booby-trapped; the loss and the gradients of s, weight and
    bias against the f64 chain within 8 x the f32 chain's own distance (the rule of the kernel cases above)."""
    dtype = torch.float32
    import torch.nn.functional as F
    from cleanumamba_amd.training import distill
    shapes = [(2, 11, 13, 37, "rows"), (2, 16, 24, 37, "rows"), (2, 8, 8, 5, "contig")]
    ads = _adapters([(a, b) for _, a, b, _, _ in shapes], cuda).train()
    g = torch.Generator().manual_seed(11)
    S = [torch.randn(B, a, T, generator=g).to(dtype) for B, a, _, T, _ in shapes]
    Tt = [torch.randn(B, b, T, generator=g).to(dtype) for B, _, b, T, _ in shapes]

    def chain(wide):
        a2 = copy.deepcopy(ads).to(wide)
        s = [x.to(wide).clone().requires_grad_(True) for x in S]
        kd, _ = R.kd_chain(s, [x.to(wide) for x in Tt], a2, 1.0)
        kd.backward()
        return float(kd), [x.grad for x in s], [p.grad for p in a2.parameters()]
    kd64, ds64, dp64 = chain(torch.float64)
    kd32, ds32, dp32 = chain(torch.float32)

    ads = ads.to(cuda)
    sg = [_lay(x, lay, cuda, fill=0.0).requires_grad_(True) for x, (_, _, _, _, lay) in zip(S, shapes)]
    tg = [_lay(x, lay, cuda) for x, (_, _, _, _, lay) in zip(Tt, shapes)]
    assert distill.kernel_route(sg, tg, ads)

    def boom(*a, **k):
        raise AssertionError("a torch convolution / linear / batch norm ran on the kernel route")
    for fn in ("conv1d", "linear", "batch_norm"):
        monkeypatch.setattr(F, fn, boom)
    kd, per_layer = distill.kd_feature_loss(sg, tg, ads, 1.0)
    kd.backward()
    monkeypatch.undo()
    assert len(per_layer) == 3 and bool(torch.isfinite(kd))
    print(f"embed route: loss err {abs(float(kd) - kd64):.3e} (f32 chain {abs(kd32 - kd64):.3e})")
    assert abs(float(kd) - kd64) <= 8 * abs(kd32 - kd64)
    for i, (mine, w64, w32) in enumerate(zip([x.grad for x in sg], ds64, ds32)):
        err, ref = rel_l2(mine, w64), rel_l2(w32, w64)
        print(f"embed route: d/ds[{i}] rel-L2 {err:.3e} (f32 chain {ref:.3e})")
        assert bool(torch.isfinite(mine).all()) and err <= 8 * ref
    for (n, p), w64, w32 in zip(ads.named_parameters(), dp64, dp32):
        err, ref = rel_l2(p.grad, w64), rel_l2(w32, w64)
        print(f"embed route: d/d{n} rel-L2 {err:.3e} (f32 chain {ref:.3e})")
        assert err <= 8 * ref, n


# ------------------------------------------------------------------------------------------------------- whole steps
def _models(cuda):
    """(teacher, pruned student, adapters, cfg) on the GPU from the 442k checkpoint."""
    from cleanumamba_amd.network import CleanUMamba
    from cleanumamba_amd.pruning import CleanUMambaPrunableChannels, prune
    from cleanumamba_amd.training.distill import make_adapters
    sd, cfg = load_ckpt("442k")
    nets = []
    for _ in range(2):
        net = CleanUMamba(**cfg)
        net.load_state_dict(sd, strict=True)
        nets.append(net.to(cuda).train())
    teacher, student = nets
    groups = CleanUMambaPrunableChannels(student)
    assert groups[0].name == "encode_down_0" and groups[3].name == "encode_down_1"
    prune(groups, {groups[0]: [1, 29], groups[3]: [1, 61]}, None)
    torch.manual_seed(7)
    return teacher, student, make_adapters(student, teacher), cfg


def _named_grads(step, student, adapters):
    step.buckets.flat.settle()              # (lazy zero_grad: the flat gradient is valid only behind settle())
    out = {"student." + n: p.grad.detach().clone() for n, p in student.named_parameters()}
    out.update({"adapters." + n: p.grad.detach().clone() for n, p in adapters.named_parameters()})
    return out


def test_whole_step_kernel_route_against_fallback_route(cuda, monkeypatch):
    """One micro_step (B = 2, 8 000 samples, f32) of TrainStep(distill=...) on the kernel route and on the fallback route:
    every gradient within 2 x the fallback route's own rel-L2 distance to the same step in f64 on the CPU."""
    from cleanumamba_amd.training import distill
    from cleanumamba_amd.training.train_step import DEFAULT_LOSS, TrainStep
    from cleanumamba_amd.util.stft_loss import MultiResolutionSTFTLoss
    from cleanumamba_amd.util.util import loss_fn
    clean, noisy = synth.waveform(2, 8000, seed=41)
    grads, routes = {}, []
    real_route = distill.kernel_route
    for route in ("kernel", "fallback"):
        teacher, student, adapters, cfg = _models(cuda)
        if route == "kernel":
            twins = (R.cpu_twin(student, cfg), R.cpu_twin(teacher, cfg).eval(), copy.deepcopy(adapters).cpu().double())
            monkeypatch.setattr(distill, "kernel_route", lambda *a: routes.append(real_route(*a)) or routes[-1])
        else:
            monkeypatch.setattr(distill, "kernel_route", lambda *a: False)
        step = TrainStep(student, loss_config={"kd_p": 1}, distill=(teacher, adapters), use_graph=False)
        step.zero_grad()
        step.micro_step(clean.to(cuda), noisy.to(cuda))
        grads[route] = _named_grads(step, student, adapters)
        monkeypatch.undo()
    assert routes == [True]
    s64, t64, a64 = twins
    mr = MultiResolutionSTFTLoss(**DEFAULT_LOSS["stft_config"]).double()
    kw = {k: v for k, v in DEFAULT_LOSS.items() if k != "stft_config"}
    loss, _ = loss_fn(s64, (clean.double(), noisy.double()), mrstftloss=mr, kd_p=1, teacher_net=t64,
                      student_teacher_adapter_layers=a64, **kw)
    loss.backward()
    want = {"student." + n: p.grad for n, p in s64.named_parameters()}
    want.update({"adapters." + n: p.grad for n, p in a64.named_parameters()})
    assert set(want) == set(grads["kernel"]) == set(grads["fallback"])
    worst = 0.0
    for n, w in want.items():
        base = rel_l2(grads["fallback"][n], w)
        mine = rel_l2(grads["kernel"][n], grads["fallback"][n])
        worst = max(worst, mine / max(base, 1e-300))
        print(f"step grads {n}: kernel vs fallback {mine:.3e}, fallback vs f64 {base:.3e}")
        assert mine <= 2 * base, n
    record("distill_step_route_worst_ratio", worst)


@pytest.mark.parametrize("dtype", [None, torch.bfloat16])
def test_distill_graph_replay_equals_eager_steps(cuda, dtype):
    """As test_optim_groups_gpu.py::test_adamw_graph_replay_equals_eager_steps, with the teacher's forward, the adapters
    and their running statistics inside the captured step."""
    from cleanumamba_amd.training.train_step import TrainStep
    sets = [_models(cuda), _models(cuda)]
    for (n, p), (_, q) in zip(sets[0][2].named_parameters(), sets[1][2].named_parameters()):
        assert torch.equal(p, q), n
    cfg = {"n_iters": 200}
    steps = [TrainStep(s, optimization=cfg, loss_config={"kd_p": 1}, autocast_dtype=dtype, distill=(t, a), use_graph=g)
             for (t, s, a, _), g in zip(sets, (True, False))]
    losses = [[], []]
    for it in range(8):
        clean, noisy = synth.waveform(2, 8000, seed=20 + it)
        for k in range(2):
            loss, gn = steps[k](clean.to(cuda), noisy.to(cuda))
            losses[k].append(float(loss))
    assert steps[0].graph_status == "captured", steps[0].graph_status
    assert steps[1].graph_status == "off"
    for k in (1, 2):                    # student, adapters
        for (ka, pa), (kb, pb) in zip(sets[0][k].named_parameters(), sets[1][k].named_parameters()):
            assert rel_l2(pa, pb) < 1e-6, ka
    assert max(abs(a - b) for a, b in zip(*losses)) < 1e-5 * max(losses[1])
    for (ka, ba), (kb, bb) in zip(sets[0][2].named_buffers(), sets[1][2].named_buffers()):
        assert torch.equal(ba, bb), ka
        if ka.endswith("num_batches_tracked"):
            assert int(ba) == 8
    for p in sets[0][0].parameters():   # the teacher: frozen, in eval mode, outside the optimizer
        assert not p.requires_grad and p.grad is None
    assert not sets[0][0].training
