"""Parameter groups and decoupled weight decay in the flat optimizer's one-launch update (cum_optim_adam_groups,
csrc/optim.hip) against ``torch.optim.AdamW`` / ``torch.optim.Adam`` over the same groups -- the classes the reference
builds (src/training/train.py:126-154) -- and through TrainStep: eager, captured, and after pruning.

Bounds: those of test_train_gpu.py::test_flat_adam_matches_torch_adam_clip_and_scaler for the one-group kernel, whose
arithmetic this one repeats term by term: 2e-6 rel-L2 on parameters, 1e-5 on the moments, 1e-5 relative on the norm."""
import pytest
import torch
import torch.nn as nn

from conftest import load_ckpt, record, rel_l2
from oracle import synth

pytestmark = pytest.mark.gpu

P_TOL, M_TOL, NORM_TOL = 2e-6, 1e-5, 1e-5


def _mk(cuda):
    # 2-D and 3-D weights, 1-D tensors, a 1-element bias
    return nn.Sequential(nn.Linear(37, 53), nn.LayerNorm(53), nn.Linear(53, 7), nn.Conv1d(3, 5, 4), nn.Conv1d(5, 1, 1)).to(cuda)


def _twins(cuda, seed=1):
    torch.manual_seed(seed)
    a, b = _mk(cuda), _mk(cuda)
    b.load_state_dict(a.state_dict())
    return a, b


def _groups(net, wd):
    from cleanumamba_amd.training.train_step import decay_groups
    return decay_groups(net, wd)


def _set_grads(a, b, it, cuda, scale=None):
    g = torch.Generator().manual_seed(100 + it)
    for pa, pb in zip(a.parameters(), b.parameters()):
        s = scale if scale is not None else (3.0 if it % 2 else 0.01)           # clipped / unclipped steps
        gr = (torch.randn(pa.shape, generator=g) * s).to(cuda)
        for p in (pa, pb):                      # (a flat-managed twin keeps its gradient VIEW: copy into it)
            if p.grad is None:
                p.grad = gr.clone()
            else:
                p.grad.copy_(gr)


def _compare(tag, a, b, opt_a, opt_b):
    worst = 0.0
    for i, (pa, pb) in enumerate(zip(a.parameters(), b.parameters())):
        err = rel_l2(pa, pb)
        worst = max(worst, err)
        assert err < P_TOL, (tag, i, tuple(pa.shape), err)
    sd, sb = opt_a.state_dict(), opt_b.state_dict()
    assert [g["params"] for g in sd["param_groups"]] == [g["params"] for g in sb["param_groups"]]
    assert sorted(sd["state"]) == sorted(sb["state"])
    for k in sb["state"]:
        assert rel_l2(sd["state"][k]["exp_avg"], sb["state"][k]["exp_avg"]) < M_TOL, (tag, k)
        assert rel_l2(sd["state"][k]["exp_avg_sq"], sb["state"][k]["exp_avg_sq"]) < M_TOL, (tag, k)
    record(f"optim_groups_param_rel_l2[{tag}]", worst)


def _steps_against_torch(cuda, tag, decoupled, wd, base_lrs, steps=6):
    from cleanumamba_amd.training.flat_optim import FlatAdam, FlatParams
    a, b = _twins(cuda)
    flat = FlatParams(a)
    opt_a = FlatAdam(flat, lr=1e-2, max_grad_norm=0.5, groups=_groups(a, wd), decoupled_weight_decay=decoupled)
    opt_b = (torch.optim.AdamW if decoupled else torch.optim.Adam)(_groups(b, wd), lr=1e-2)
    assert len(opt_a.param_groups) == len(opt_b.param_groups) == 2
    for it in range(steps):
        _set_grads(a, b, it, cuda)
        for k in range(2):
            opt_a.param_groups[k]["lr"] = opt_b.param_groups[k]["lr"] = base_lrs[k] / (1 + it)
        norm_b = nn.utils.clip_grad_norm_(b.parameters(), 0.5)
        opt_b.step()
        opt_a.step()
        assert abs(float(opt_a.grad_norm) - float(norm_b)) < NORM_TOL * float(norm_b)
        for i, (pa, pb) in enumerate(zip(a.parameters(), b.parameters())):
            assert rel_l2(pa, pb) < P_TOL, (tag, it, i)
    _compare(tag, a, b, opt_a, opt_b)
    assert float(opt_a.state_vec[5]) == steps and flat.intact()
    return a, b, opt_a, opt_b


@pytest.mark.parametrize("base_lrs", [(1e-2, 1e-2), (1e-2, 3e-3)], ids=["one_lr", "two_lrs"])
def test_adamw_groups_match_torch_adamw(cuda, base_lrs):
    """Six steps, clipped and unclipped, a learning rate that changes every step: decoupled decay 0.1 on the
    dim() >= 2 tensors, none on the rest."""
    _steps_against_torch(cuda, f"adamw_{base_lrs[1]}", True, 0.1, base_lrs)


def test_adam_l2_groups_match_torch_adam(cuda):
    """decoupled_weight_decay=False: Adam's L2 form per group (0.01 and 0) against torch.optim.Adam over the groups."""
    _steps_against_torch(cuda, "adam_l2", False, 0.01, (1e-2, 1e-2))


def test_two_equal_groups_give_the_bits_of_the_one_group_kernel(cuda):
    """All parameters in two groups with the same hyperparameters, L2 form: cum_optim_adam_groups must not differ from
    cum_optim_adam in one bit of p, m or v."""
    from cleanumamba_amd.training.flat_optim import FlatAdam, FlatParams
    a, b = _twins(cuda, seed=3)
    fa, fb = FlatParams(a), FlatParams(b)
    groups = _groups(a, 0.01)
    groups[1]["weight_decay"] = 0.01
    opt_a = FlatAdam(fa, lr=1e-2, max_grad_norm=0.5, groups=groups, decoupled_weight_decay=False)
    opt_b = FlatAdam(fb, lr=1e-2, max_grad_norm=0.5, weight_decay=0.01)
    assert opt_a.grouped and not opt_b.grouped
    assert bool((opt_a.tile_group < 0).any()) and int(opt_a.seg_end.numel()) > 2        # the lane walk is exercised
    for it in range(3):
        _set_grads(a, b, it, cuda)
        lr = 1e-2 / (1 + it)
        for g in opt_a.param_groups + opt_b.param_groups:
            g["lr"] = lr
        opt_a.step()
        opt_b.step()
        assert torch.equal(fa.data, fb.data), it
    assert torch.equal(opt_a.exp_avg, opt_b.exp_avg) and torch.equal(opt_a.exp_avg_sq, opt_b.exp_avg_sq)
    assert float(opt_a.exp_avg.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ layout stress
class _Bag(nn.Module):
    def __init__(self, sizes):
        super().__init__()
        self.ps = nn.ParameterList([nn.Parameter(torch.randn(n)) for n in sizes])


def _stress_sizes(tile, big):
    """Sizes in FLAT order (FlatParams lays parameters out in reverse registration order).  ``big``: a first parameter
    that alone is longer than one pass of the kernel's grid (4096 workgroups of one tile), so that every edge case below
    is met in a later pass of the grid loop."""
    g = torch.Generator().manual_seed(5)
    small = lambda n: [int(x) for x in torch.randint(1, 10, (n,), generator=g)]
    sizes = [4096 * tile + 2 * tile + 5] if big else []
    sizes += small(150)
    off = sum((n + 3) // 4 * 4 for n in sizes)
    sizes.append(2 * tile - off % tile - 4)            # ends 4 elements before a tile edge
    edge = len(sizes)
    sizes.append(3 * tile + 4)                         # starts 4 before the edge, spans it and three whole tiles,
    sizes += [1]                                       # ends exactly on an edge; a 1-element parameter starts the next tile
    sizes += small(150)
    return sizes, edge


@pytest.mark.parametrize("big", [False, True], ids=["small", "beyond_one_grid_pass"])
def test_layout_stress_against_torch_adamw(cuda, big):
    from cleanumamba_amd import hip
    from cleanumamba_amd.training.flat_optim import FlatAdam, FlatParams
    tile = hip.lib().cum_optim_group_tile_elems()
    sizes, edge = _stress_sizes(tile, big)
    torch.manual_seed(11)
    a = _Bag(list(reversed(sizes))).to(cuda)
    b = _Bag(list(reversed(sizes))).to(cuda)
    b.load_state_dict(a.state_dict())
    flat = FlatParams(a)
    assert [p.numel() for p in flat.params] == sizes
    assert (flat.offsets[edge] + 4) % tile == 0 and (flat.offsets[edge] + sizes[edge]) % tile == 0
    assert flat.offsets[edge + 1] % tile == 0 and sizes[edge + 1] == 1
    if big:
        assert flat.numel > 4096 * tile and flat.offsets[1] > 4096 * tile

    def groups(net):                                    # three groups, dealt out in flat order
        ps = list(reversed(list(net.parameters())))
        return [{"params": ps[k::3], "weight_decay": wd, "lr": lr}
                for k, (wd, lr) in enumerate([(0.1, 1e-3), (0.0, 2e-3), (0.03, 5e-4)])]
    opt_a = FlatAdam(flat, lr=1e-3, max_grad_norm=0.5, groups=groups(a), decoupled_weight_decay=True)
    opt_b = torch.optim.AdamW(groups(b), lr=1e-3)
    n_mixed = int((opt_a.tile_group < 0).sum())
    assert n_mixed >= 3 and int((opt_a.tile_group >= 0).sum()) >= 3
    pad = torch.ones(flat.numel, dtype=torch.bool, device=cuda)
    for p, o in zip(flat.params, flat.offsets):
        pad[o:o + p.numel()] = False
    assert int(pad.sum()) > 100
    gen = torch.Generator(device=cuda).manual_seed(9)
    for it in range(2):
        for pa, pb in zip(a.parameters(), b.parameters()):
            gr = torch.randn(pa.shape, generator=gen, device=cuda) * (0.05 if it else 1e-4)
            pa.grad.copy_(gr)
            pb.grad = gr.clone()
        norm_b = nn.utils.clip_grad_norm_(b.parameters(), 0.5)
        opt_b.step()
        opt_a.step()
        assert abs(float(opt_a.grad_norm) - float(norm_b)) < NORM_TOL * float(norm_b)
    # (one comparison of the whole buffers first: 300 small tensors each against its own norm follow)
    theirs = torch.zeros_like(flat.data)
    for pb, o in zip(reversed(list(b.parameters())), flat.offsets):
        theirs[o:o + pb.numel()] = pb.detach()
    assert rel_l2(flat.data, theirs) < P_TOL
    _compare(f"stress_{'big' if big else 'small'}", a, b, opt_a, opt_b)
    for name, buf in (("p", flat.data), ("m", opt_a.exp_avg), ("v", opt_a.exp_avg_sq), ("g", flat.grad)):
        assert float(buf[pad].abs().max()) == 0.0, name


# ------------------------------------------------------------------------------------------------ skipped step, checkpoints
def test_inf_gradient_skips_every_group(cuda):
    from cleanumamba_amd.training.flat_optim import FlatAdam, FlatParams
    a, b = _twins(cuda, seed=4)
    flat = FlatParams(a)
    opt = FlatAdam(flat, lr=1e-2, max_grad_norm=0.5, groups=_groups(a, 0.1), decoupled_weight_decay=True,
                   loss_scaling=True, init_scale=1024.0)
    _set_grads(a, b, 0, cuda, scale=1024.0)
    opt.step()                                                   # a clean step: the moments are not zero afterwards
    assert float(opt.state_vec[5]) == 1 and float(opt.exp_avg.abs().max()) > 0
    keep = [t.clone() for t in (flat.data, opt.exp_avg, opt.exp_avg_sq)]
    _set_grads(a, b, 1, cuda, scale=1024.0)
    victim = opt.param_groups[1]["params"][1]                    # a 1-D tensor of the group that does not decay
    assert victim.dim() == 1
    victim.grad.view(-1)[0] = float("inf")
    opt.step()
    for k, t in zip(keep, (flat.data, opt.exp_avg, opt.exp_avg_sq)):
        assert torch.equal(k, t), "a step with inf gradients must change nothing, the decay included"
    assert float(opt.loss_scale) == 512.0 and float(opt.state_vec[9]) == 1 and float(opt.state_vec[5]) == 1


def test_checkpoints_move_between_flat_adam_and_torch_adamw(cuda):
    from cleanumamba_amd.training.flat_optim import FlatAdam, FlatParams
    a, b, opt_a, opt_b = _steps_against_torch(cuda, "ckpt_before", True, 0.1, (1e-2, 3e-3), steps=2)
    c, d = _mk(cuda), _mk(cuda)
    c.load_state_dict(a.state_dict())
    d.load_state_dict(b.state_dict())
    opt_c = torch.optim.AdamW(_groups(c, 0.5), lr=1.0)           # hyperparameters come from the checkpoint
    opt_c.load_state_dict(opt_a.state_dict())
    opt_d = FlatAdam(FlatParams(d), lr=1.0, max_grad_norm=0.5, groups=_groups(d, 0.5), decoupled_weight_decay=True)
    opt_d.load_state_dict(opt_b.state_dict())
    assert [g["lr"] for g in opt_d.param_groups] == [g["lr"] for g in opt_b.param_groups]
    assert [g["weight_decay"] for g in opt_d.param_groups] == [0.1, 0.0]
    assert [g["weight_decay"] for g in opt_c.param_groups] == [0.1, 0.0]
    assert float(opt_d.state_vec[5]) == 2
    g = torch.Generator().manual_seed(77)
    for ps in zip(a.parameters(), b.parameters(), c.parameters(), d.parameters()):
        gr = (torch.randn(ps[0].shape, generator=g) * 0.01).to(cuda)
        for p in ps:
            if p.grad is None:
                p.grad = gr.clone()
            else:
                p.grad.copy_(gr)
    for net, opt in ((a, opt_a), (b, opt_b), (c, opt_c), (d, opt_d)):
        if isinstance(opt, torch.optim.Optimizer):
            nn.utils.clip_grad_norm_(net.parameters(), 0.5)
        opt.step()
    for i, ps in enumerate(zip(a.parameters(), b.parameters(), c.parameters(), d.parameters())):
        assert rel_l2(ps[2], ps[0]) < P_TOL, ("torch from flat", i)
        assert rel_l2(ps[3], ps[1]) < P_TOL, ("flat from torch", i)
        assert rel_l2(ps[0], ps[1]) < P_TOL, i


# ------------------------------------------------------------------------------------------------ through TrainStep
def _net442k(cuda):
    from cleanumamba_amd.network import CleanUMamba
    sd, cfg = load_ckpt("442k")
    net = CleanUMamba(**cfg)
    net.load_state_dict(sd, strict=True)
    return net.to(cuda).train()


def _adamw_step(cuda, W):
    from cleanumamba_amd.training.train_step import TrainStep
    net = _net442k(cuda)
    step = TrainStep(net, optimization={"optimizer": "adamw", "weight_decay": W, "learning_rate": 1e-3, "n_iters": 100},
                     use_graph=False)
    return net, step


def _decay_lands_where_it_should(cuda, nets, steps, tag):
    """One step of a W = 0.1 and a W = 0 train step from the same state on the same batch: the gradients are equal, so the
    dim() < 2 tensors end equal bit for bit and every other one obeys p_W = p_init (1 - lr W) + (p_0 - p_init)."""
    W = steps[0].optimizer.param_groups[0]["weight_decay"]
    assert W == 0.1 and steps[1].optimizer.param_groups[0]["weight_decay"] == 0
    assert [g["weight_decay"] for g in steps[0].optimizer.param_groups] == [0.1, 0.0]
    lr = steps[0].optimizer.param_groups[0]["lr"]
    assert lr > 0 and lr == steps[1].optimizer.param_groups[0]["lr"]
    init = {n: p.detach().clone() for n, p in nets[0].named_parameters()}
    for n, p in nets[1].named_parameters():
        assert torch.equal(p, init[n]), n
    clean, noisy = synth.waveform(2, 8000, seed=5)
    for s in steps:
        s(clean.to(cuda), noisy.to(cuda))
    worst, moved = 0.0, 0
    for (n, pw), (_, p0) in zip(nets[0].named_parameters(), nets[1].named_parameters()):
        if pw.dim() < 2:
            assert torch.equal(pw, p0), n
        else:
            want = init[n].double() * (1.0 - lr * W) + (p0.double() - init[n].double())
            err = rel_l2(pw, want)
            worst = max(worst, err)
            assert err < P_TOL, (n, err)
            assert not torch.equal(pw, p0), n
        moved += int(not torch.equal(p0, init[n]))
    assert moved > 0.5 * len(init)
    record(f"optim_groups_decay_property[{tag}]", worst)


def test_train_step_adamw_decays_only_the_matrices(cuda):
    from cleanumamba_amd.training.flat_optim import FlatAdam
    pairs = [_adamw_step(cuda, 0.1), _adamw_step(cuda, 0.0)]
    opt = pairs[0][1].optimizer
    assert isinstance(opt, FlatAdam) and opt.grouped and opt.decoupled and len(opt.param_groups) == 2
    assert all(p.dim() >= 2 for p in opt.param_groups[0]["params"])
    assert all(p.dim() < 2 for p in opt.param_groups[1]["params"])
    _decay_lands_where_it_should(cuda, [n for n, _ in pairs], [s for _, s in pairs], "fresh")


@pytest.mark.parametrize("dtype", [None, torch.bfloat16])
def test_adamw_graph_replay_equals_eager_steps(cuda, dtype):
    """As test_train_gpu.py::test_graph_replay_equals_eager_steps, with the grouped update in the captured step: the
    group table is read at replay time, so the changing learning rate reaches it."""
    from cleanumamba_amd.training.train_step import TrainStep
    nets = [_net442k(cuda), _net442k(cuda)]
    cfg = {"n_iters": 200, "optimizer": "adamw", "weight_decay": 0.01}
    steps = [TrainStep(nets[0], optimization=cfg, autocast_dtype=dtype, use_graph=True),
             TrainStep(nets[1], optimization=cfg, autocast_dtype=dtype, use_graph=False)]
    losses = [[], []]
    for it in range(8):
        clean, noisy = synth.waveform(2, 8000, seed=20 + it)
        for k in range(2):
            loss, gn = steps[k](clean.to(cuda), noisy.to(cuda))
            losses[k].append(float(loss))
    assert steps[0].graph_status == "captured", steps[0].graph_status
    assert steps[1].graph_status == "off"
    assert steps[0].optimizer.grouped and float(steps[0].optimizer.state_vec[5]) == 8
    for (ka, pa), (kb, pb) in zip(nets[0].named_parameters(), nets[1].named_parameters()):
        assert rel_l2(pa, pb) < 1e-6, ka
    assert max(abs(a - b) for a, b in zip(*losses)) < 1e-5 * max(losses[1])


def _prune_some(net, optimizer):
    from cleanumamba_amd.pruning import CleanUMambaPrunableChannels, prune
    groups = CleanUMambaPrunableChannels(net)
    assert groups[0].name == "encode_down_0" and groups[3].name == "encode_down_1"
    prune(groups, {groups[0]: [1, 29], groups[3]: [1, 61]}, optimizer)


def test_adamw_groups_survive_pruning(cuda):
    from cleanumamba_amd import hip
    from cleanumamba_amd.training.flat_optim import group_tables
    net, step = _adamw_step(cuda, 0.1)
    opt, flat = step.optimizer, step.buckets.flat
    for it in range(2):
        clean, noisy = synth.waveform(2, 8000, seed=30 + it)
        step(clean.to(cuda), noisy.to(cuda))
    n_before, tables_before = flat.numel, [t.clone() for t in (opt.tile_group, opt.seg_end, opt.seg_group)]
    _prune_some(net, opt)
    assert flat.numel < n_before and flat.intact()
    fresh = group_tables(flat.offsets, [p.numel() for p in flat.params], [0 if p.dim() >= 2 else 1 for p in flat.params],
                         hip.lib().cum_optim_group_tile_elems())
    for mine, want in zip((opt.tile_group, opt.seg_end, opt.seg_group), fresh):
        assert mine.device.type == "cuda" and torch.equal(mine.cpu(), want)
    assert not torch.equal(opt.seg_end.cpu(), tables_before[1].cpu())
    assert int(opt.seg_end[-1]) * 4 == flat.numel
    assert all(p.dim() >= 2 for p in opt.param_groups[0]["params"]) and all(p.dim() < 2 for p in opt.param_groups[1]["params"])
    clean, noisy = synth.waveform(2, 8000, seed=33)
    loss, _ = step(clean.to(cuda), noisy.to(cuda))
    assert bool(torch.isfinite(loss)) and flat.intact() and float(opt.state_vec[5]) == 3
    pad = torch.ones(flat.numel, dtype=torch.bool, device=cuda)
    for p, o in zip(flat.params, flat.offsets):
        pad[o:o + p.numel()] = False
    if bool(pad.any()):
        for buf in (flat.data, opt.exp_avg, opt.exp_avg_sq):
            assert float(buf[pad].abs().max()) == 0.0

    # a twin pair (W = 0.1 and W = 0) pruned identically before its first step: the decay still lands on the matrices only
    pairs = [_adamw_step(cuda, 0.1), _adamw_step(cuda, 0.0)]
    for n, s in pairs:
        _prune_some(n, s.optimizer)
    _decay_lands_where_it_should(cuda, [n for n, _ in pairs], [s for _, s in pairs], "pruned")
