"""Channel pruning on the GPU: the importance kernel against an f64 restatement and the reference's fixtures, the loss
scale and lazy zeroing, the flat-buffer compaction (bit-exact, training state kept), and training / inference after a
prune matching a fresh model built from the pruned state dict."""
import numpy as np
import pytest
import torch

from conftest import golden_json, load_ckpt, load_golden, record, rel_l2

pytestmark = pytest.mark.gpu

KEYS = ["weight", "grad", "taylor_individual", "taylor_squared_individual", "taylor_group"]
GRAD_SEED = 4242


def model(key, dev):
    from cleanumamba_amd.network import CleanUMamba
    sd, cfg = load_ckpt(key)
    net = CleanUMamba(**cfg)
    if key == "442k":
        net.load_state_dict(sd, strict=True)
    else:
        net.load_pruned_state_dict(sd)
    return net.to(dev).train(), cfg


def synthetic_grads(net, seed=GRAD_SEED):
    """The gradients of tools/make_golden_pruning.py (same recipe, CPU generator)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for p in net.parameters():
        fan = max(1, p.numel() // p.shape[0])
        out.append(torch.randn(p.shape, generator=g, dtype=torch.float32) * (1e-3 / fan ** 0.5))
    return out


def set_grads(net, grads, mult=1.0):
    with torch.no_grad():
        for p, g in zip(net.parameters(), grads):
            if p.grad is None:
                p.grad = torch.zeros_like(p)
            p.grad.copy_(g.to(p.device) * mult)


def f64_group(group):
    """The reference's channel_importances restated in f64 (transpose, flatten, split at the offset, reshape)."""
    acc, counts = {}, {}
    for pm in group.modules:
        p = pm.param()
        w, g = p.detach().double(), p.grad.double()
        if pm.dim == 1:
            w, g = w.transpose(1, 0), g.transpose(1, 0)
        w = w.flatten(1) if w.dim() > 2 else (w.unsqueeze(1) if w.dim() == 1 else w)
        g = g.flatten(1) if g.dim() > 2 else (g.unsqueeze(1) if g.dim() == 1 else g)
        n = group.n_channels * pm.n_heads
        w = w[pm.channel_offset:pm.channel_offset + n].reshape(group.n_channels, -1)
        g = g[pm.channel_offset:pm.channel_offset + n].reshape(group.n_channels, -1)
        wg = w * g
        vals = {"weight": (w * w).sum(1), "grad": (g * g).sum(1), "taylor_individual": wg.abs().sum(1),
                "taylor_squared_individual": (wg * wg).sum(1), "taylor_group": wg.sum(1).abs(),
                "abs_wg": wg.abs().sum(1)}
        for k, v in vals.items():
            acc[k] = v if k not in acc else (acc[k] * counts[k] + v) / (counts[k] + 1)
            counts[k] = counts.get(k, 0) + 1
    return acc


def check_against_f64(groups, got, tag):
    worst = 0.0
    for g, d in zip(groups, got):
        ref = f64_group(g)
        for k in KEYS:
            a = d[k].double().cpu()
            b = ref[k].cpu()
            if k == "taylor_group":
                err = ((a - b).abs() / ref["abs_wg"].cpu().clamp_min(1e-300)).max().item()
            else:
                err = ((a - b).abs() / b.abs().clamp_min(1e-300)).max().item()
            worst = max(worst, err)
            assert err < 1e-5, (tag, g.name, k, err)
    record(f"prune_importance_f64[{tag}]", worst)


@pytest.mark.parametrize("key", ["442k", "e6_pruned500k"])
def test_importances_against_f64_and_the_reference(cuda, key):
    from cleanumamba_amd.pruning import CleanUMambaPrunableChannels
    from cleanumamba_amd.pruning import device as D
    f = load_golden("pruning_" + key)
    net, _ = model(key, cuda)
    grads = synthetic_grads(net)
    assert abs(sum(float(g.double().abs().sum()) for g in grads) - float(f["grad_checksum"])) < 1e-9 * float(f["grad_checksum"])
    set_grads(net, grads)
    groups = CleanUMambaPrunableChannels(net)
    assert [g.name for g in groups] == golden_json(f["group_names"])
    got = D.group_importances(groups)
    check_against_f64(groups, got, key)
    for g, d, npar, nf in zip(groups, got, f["n_parameters"], f["n_filters"]):
        assert d["n_parameters"] == npar and d["n_filters"] == nf and d["act_var"] is None
        for k in KEYS:                        # the reference's f32 sums: summation order differs, nothing else
            ref = torch.from_numpy(f[f"imp.{g.name}.{k}"]).double()
            tol = 1e-4 * (ref.abs() + (torch.from_numpy(f[f"imp.{g.name}.taylor_individual"]).double()
                                       if k == "taylor_group" else 0))
            assert ((d[k].double().cpu() - ref).abs() <= tol + 1e-30).all(), (g.name, k)
    again = D.group_importances(groups)
    for a, b in zip(got, again):
        for k in KEYS:
            assert torch.equal(a[k], b[k])
    # the per-group call (its own launch) gives the same values as the batched one
    single = groups[-4].channel_importances()
    for k in KEYS:
        assert torch.equal(single[k], got[-4][k])


def test_importances_e8_size(cuda):
    """A seeded model of the E8 configuration (41.4 M parameters): f64 restatement and run-to-run bitwise equality."""
    from cleanumamba_amd.network import CleanUMamba
    from cleanumamba_amd.pruning import CleanUMambaPrunableChannels
    from cleanumamba_amd.pruning import device as D
    torch.manual_seed(5)
    net = CleanUMamba(channels_H=64, max_H=768, encoder_n_layers=8, tsfm_n_layers=3, tsfm_n_head=8, tsfm_d_model=512,
                      tsfm_d_inner=2048).to(cuda)
    g = torch.Generator(device=cuda).manual_seed(9)
    for p in net.parameters():
        p.grad = torch.randn(p.shape, generator=g, device=cuda) * 1e-3
    groups = CleanUMambaPrunableChannels(net)
    got = D.group_importances(groups)
    check_against_f64(groups, got, "e8")
    again = D.group_importances(groups)
    for a, b in zip(got, again):
        for k in KEYS:
            assert torch.equal(a[k], b[k])


def test_loss_scale_and_lazy_zeroing(cuda):
    """Gradients x S under a FlatAdam with device loss scale S give the unscaled importances (bitwise: S is a power of
    two); a view left stale by lazy zeroing counts as zero; a non-finite gradient raises naming its group."""
    from cleanumamba_amd.pruning import CleanUMambaPrunableChannels
    from cleanumamba_amd.pruning import device as D
    from cleanumamba_amd.training.flat_optim import FlatAdam, FlatParams
    ref_net, _ = model("442k", cuda)
    grads = synthetic_grads(ref_net)
    set_grads(ref_net, grads)
    want = D.group_importances(CleanUMambaPrunableChannels(ref_net))

    net, _ = model("442k", cuda)
    flat = FlatParams(net)
    adam = FlatAdam(flat, loss_scaling=True)
    S = float(adam.loss_scale)
    assert S == 65536.0
    set_grads(net, grads, mult=S)
    groups = CleanUMambaPrunableChannels(net)
    got = D.group_importances(groups)
    for a, b in zip(got, want):
        for k in KEYS:
            assert torch.equal(a[k], b[k]), k

    # lazy zeroing: the stale view of tsfm_conv2.weight holds last cycle's values -> counts as zero
    i = flat.index[id(net.tsfm_conv2.weight)]
    flat.stale = {i}
    flat.grad_views[i].fill_(123.0)
    got = D.group_importances(groups)
    assert float(flat.grad_views[i].abs().max()) == 0.0
    with torch.no_grad():
        ref_net.tsfm_conv2.weight.grad.zero_()
    want = D.group_importances(CleanUMambaPrunableChannels(ref_net))
    for a, b in zip(got, want):
        for k in KEYS:
            assert torch.equal(a[k], b[k]), k

    with torch.no_grad():
        net.tsfm_Mamba_layers[1].mixer.dt_proj.weight.grad[3, 1] = float("inf")
    with pytest.raises(FloatingPointError, match="d_inner1"):
        D.group_importances(groups)


def test_loss_scale_after_an_optimizer_step(cuda):
    """After a step whose loss-scale update grew the scale, the gradients still carry the old one: the importances
    divide by the scale the step used (state slot ST_GRAD_SCALE), and by the current one again once a new backward
    starts (scale_loss)."""
    from cleanumamba_amd.pruning import CleanUMambaPrunableChannels
    from cleanumamba_amd.pruning import device as D
    from cleanumamba_amd.training.flat_optim import ST_GRAD_SCALE, ST_SCALE, FlatAdam, FlatParams
    ref_net, _ = model("442k", cuda)
    grads = synthetic_grads(ref_net)
    set_grads(ref_net, grads)
    want = D.group_importances(CleanUMambaPrunableChannels(ref_net))
    net, _ = model("442k", cuda)
    flat = FlatParams(net)
    adam = FlatAdam(flat, lr=0.0, loss_scaling=True, growth_interval=1)     # lr 0: the weights stay as they are
    S = float(adam.loss_scale)
    set_grads(net, grads, mult=S)
    adam.step()
    assert float(adam.loss_scale) == 2 * S and float(adam.state_vec[ST_GRAD_SCALE]) == S
    assert adam.grads_scale_slot == ST_GRAD_SCALE
    got = D.group_importances(CleanUMambaPrunableChannels(net))
    for a, b in zip(got, want):
        for k in KEYS:
            assert torch.equal(a[k], b[k]), k
    adam.scale_loss(torch.ones((), device=cuda))                # a new backward: gradients now carry the grown scale
    assert adam.grads_scale_slot == ST_SCALE
    set_grads(net, grads, mult=2 * S)
    got = D.group_importances(CleanUMambaPrunableChannels(net))
    for a, b in zip(got, want):
        for k in KEYS:
            assert torch.equal(a[k], b[k]), k


def test_flat_prune_without_an_optimizer(cuda):
    """Flat storage with no FlatAdam: parameters and gradients only are gathered (no moment buffers), exactly."""
    from cleanumamba_amd.pruning import CleanUMambaPrunableChannels, prune
    from cleanumamba_amd.training.flat_optim import FlatParams
    f = load_golden("pruning_442k")
    net, _ = model("442k", cuda)
    flat = FlatParams(net)
    set_grads(net, synthetic_grads(net))
    before = {n: (p.detach().clone(), p.grad.clone()) for n, p in net.named_parameters()}
    groups = CleanUMambaPrunableChannels(net)
    prune(groups, _choice(groups, f))
    assert flat.intact()
    for n, p in net.named_parameters():
        idx = [torch.from_numpy(f[f"pruned.{n}.keep{k}"]).long().to(cuda) for k in range(p.dim())]
        for a, b in zip((p.detach(), p.grad), before[n]):
            for k, ix in enumerate(idx):
                b = b.index_select(k, ix)
            assert torch.equal(a, b), n


def _audio(dev, B=2, L=16000, seed=3):
    g = torch.Generator().manual_seed(seed)
    clean = 0.1 * torch.randn(B, 1, L, generator=g)
    return clean.to(dev), (clean + 0.05 * torch.randn(B, 1, L, generator=g)).to(dev)


def _choice(groups, f):
    names = [g.name for g in groups]
    want = golden_json(f["group_names"])
    assert names == want
    chosen = {g: [] for g in groups}
    for gi, ci in zip(f["prune_group"], f["prune_index"]):
        chosen[groups[gi]].append(int(ci))
    return chosen


@pytest.mark.parametrize("autocast", [None, torch.float16])
def test_flat_prune_is_exact_and_training_continues(cuda, autocast):
    from cleanumamba_amd.network import CleanUMamba
    from cleanumamba_amd.pruning import CleanUMambaPrunableChannels, prune
    from cleanumamba_amd.training.train_step import TrainStep
    f = load_golden("pruning_442k")
    net, cfg = model("442k", cuda)
    step = TrainStep(net, autocast_dtype=autocast)
    clean, noisy = _audio(cuda)
    for _ in range(5):                                  # eager warm-up, then captured replays
        step(clean, noisy)
    assert step.graph_status == "captured"
    torch.cuda.synchronize()
    opt, flat = step.optimizer, step.buckets.flat
    names = {id(p): n for n, p in net.named_parameters()}
    before = {names[id(p)]: (p.detach().clone(), p.grad.clone(), opt.exp_avg[o:o + p.numel()].view_as(p).clone(),
                             opt.exp_avg_sq[o:o + p.numel()].view_as(p).clone()) for p, o in zip(flat.params, flat.offsets)}
    state_before = opt.state_vec.clone()
    old_shapes = {n: tuple(t[0].shape) for n, t in before.items()}
    groups = CleanUMambaPrunableChannels(net)
    prune(groups, _choice(groups, f), opt)
    torch.cuda.synchronize()
    assert flat.intact() and step.graph_status == "pending"
    assert torch.equal(opt.state_vec, state_before)
    for p, o in zip(flat.params, flat.offsets):
        n = names[id(p)]
        assert list(p.shape) == f[f"pruned.{n}.shape"].tolist(), n
        idx = [torch.from_numpy(f[f"pruned.{n}.keep{k}"]).long().to(cuda) for k in range(len(old_shapes[n]))]
        mine = (p.detach(), p.grad, opt.exp_avg[o:o + p.numel()].view_as(p), opt.exp_avg_sq[o:o + p.numel()].view_as(p))
        for a, b in zip(mine, before[n]):
            for k, ix in enumerate(idx):
                b = b.index_select(k, ix)
            assert torch.equal(a, b), n
    pad = torch.ones(flat.numel, dtype=torch.bool, device=cuda)
    for p, o in zip(flat.params, flat.offsets):
        pad[o:o + p.numel()] = False
    for buf in (flat.data, flat.grad, opt.exp_avg, opt.exp_avg_sq):
        assert float(buf[pad].abs().max()) == 0.0 if bool(pad.any()) else True

    # a fresh model from the pruned state dict with the sliced Adam state, under a fresh TrainStep at the same iteration
    fresh = CleanUMamba(**cfg).to(cuda).train()
    fresh.load_pruned_state_dict({k: v.clone() for k, v in net.state_dict().items()})
    step2 = TrainStep(fresh, autocast_dtype=autocast, iteration=step.calls)
    step2.optimizer.load_state_dict(opt.state_dict())
    for i in range(4):                                  # three eager steps, then the recaptured graph
        l1, n1 = step(clean, noisy)
        l2, n2 = step2(clean, noisy)
        torch.cuda.synchronize()
        assert abs(float(l1) - float(l2)) <= 1e-6 * abs(float(l2)), i
        assert abs(float(n1) - float(n2)) <= 1e-5 * abs(float(n2)), i
        assert np.isfinite(float(l1))
    assert step.graph_status == "captured" and step2.graph_status == "captured"
    for (n, a), b in zip(net.named_parameters(), fresh.parameters()):
        assert rel_l2(a, b) < 1e-5, n


def test_inference_after_pruning(cuda):
    """forward (caches from before the prune dropped), feed / flush of a model that streamed before, and a stream pool."""
    from cleanumamba_amd.network import CleanUMamba
    from cleanumamba_amd.pruning import CleanUMambaPrunableChannels, prune
    f = load_golden("pruning_e6_pruned500k")
    net, cfg = model("e6_pruned500k", cuda)
    net.eval()
    net.normalize_input = False                          # (streaming == forward needs a fixed input scale)
    x = (0.1 * torch.randn(1, 1, 16000, generator=torch.Generator().manual_seed(2))).to(cuda)
    with torch.no_grad():
        net(x)
        for i in range(0, 16000, 4000):
            net.feed(x[0, :, i:i + 4000])
        net.flush()
        old_pool = net.stream_pool(2)
        busy = old_pool.open(1)
        old_pool.feed(busy, x[0, :, :3000])
    groups = CleanUMambaPrunableChannels(net)
    chosen = _choice(groups, f)
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    with pytest.raises(RuntimeError, match="open slots"):   # a pool slot holds state at the old widths: refused
        prune(groups, chosen)
    assert all(torch.equal(p, before[n]) for n, p in net.named_parameters())
    with torch.no_grad():
        old_pool.close(busy)
    for g, idxs in chosen.items():
        g.prune(idxs)
    fresh = CleanUMamba(**cfg).to(cuda).eval()
    fresh.load_pruned_state_dict({k: v.clone() for k, v in net.state_dict().items()})
    fresh.normalize_input = False
    with torch.no_grad():
        y, want = net(x), fresh(x)
        assert record("prune_forward_vs_fresh", rel_l2(y, want)) < 1e-6
        seq = torch.cat([net.feed(x[0, :, i:i + 1000]) for i in range(0, 16000, 1000)] + [net.flush()], 1)
        seq_f = torch.cat([fresh.feed(x[0, :, i:i + 1000]) for i in range(0, 16000, 1000)] + [fresh.flush()], 1)
        assert rel_l2(seq, seq_f) < 1e-6
        exact = ((net.valid_length(16000) - net.frame_length) // net.total_stride + 1) * net.total_stride
        assert rel_l2(seq[:, :exact], y[0, :, :exact]) < 1e-4
        for pool in (net.stream_pool(2), old_pool):          # a new pool, and the one made before (re-laid out)
            slots = pool.open(1)
            outs = [pool.feed(slots, x[0, :, i:i + 1000])[0] for i in range(0, 16000, 1000)] + [pool.close(slots)[0]]
            got = torch.cat(outs)
            assert got.shape[0] == seq.shape[1] and rel_l2(got, seq[0]) < 1e-5


def test_short_pruning_pipeline(cuda):
    """Three rounds of the reference's loop on the 442K model: accumulate gradients, select, prune, train."""
    from cleanumamba_amd.pruning import CleanUMambaPrunableChannels, get_prune_channels, prune
    from cleanumamba_amd.training.train_step import TrainStep
    net, _ = model("442k", cuda)
    step = TrainStep(net)
    groups = CleanUMambaPrunableChannels(net)
    n0 = sum(p.numel() for p in net.parameters())
    sizes = []
    for r in range(3):
        step.zero_grad()
        for s in range(2):
            clean, noisy = _audio(cuda, seed=10 * r + s)
            step.micro_step(clean, noisy)
        chosen, n_params, minima = get_prune_channels(groups, "taylor_squared_individual*n_filters/n_parameters",
                                                      None, 0.02, 8)
        assert chosen and len(minima) == len(groups)
        prune(groups, chosen, step.optimizer)
        for _ in range(2):
            clean, noisy = _audio(cuda, seed=100 + r)
            loss, _ = step(clean, noisy)
            assert np.isfinite(float(loss))
        sizes.append(sum(p.numel() for p in net.parameters()))
        assert step.buckets.flat.intact()
    assert n0 > sizes[0] > sizes[1] > sizes[2]
