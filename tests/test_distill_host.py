"""Teacher / student feature distillation on the host (no GPU): the torch fallback of training/distill.py and the teacher
branch of util.loss_fn against tests/distill_ref.py (src/util/util.py:272-289 in torch ops) in float64, the BatchNorm side
effects, the adapters' widths and the refusals."""
import copy

import pytest
import torch
import torch.nn as nn

from conftest import load_ckpt
from oracle import synth

import distill_ref as R


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _adapters(cs_, ct_, dtype=torch.float64, seed=0):
    torch.manual_seed(seed)
    return nn.ModuleList(nn.ModuleDict({"embed": nn.Conv1d(a, b, 1), "bn_s": nn.BatchNorm1d(b, eps=1e-4, affine=False),
                                        "bn_t": nn.BatchNorm1d(b, eps=1e-4, affine=False)})
                         for a, b in zip(cs_, ct_)).to(dtype)


def test_fallback_is_the_literal_chain_in_f64():
    """(B, C, T) = (2, 13, 37) on the teacher's side, 11 and 13 channels on the student's: loss and every gradient to
    1e-12 relative (the same arithmetic in f64)."""
    from cleanumamba_amd.training.distill import kd_feature_loss, kernel_route
    g = torch.Generator().manual_seed(5)
    S = [torch.randn(2, c, 37, generator=g, dtype=torch.float64) for c in (11, 13)]
    T = [torch.randn(2, 13, 37, generator=g, dtype=torch.float64) for _ in range(2)]
    ads = _adapters((11, 13), (13, 13))
    got = {}
    for tag, fn in (("mine", kd_feature_loss), ("ref", R.kd_chain)):
        a = copy.deepcopy(ads)
        s = [x.clone().requires_grad_(True) for x in S]
        assert not kernel_route(s, T, a)
        kd, per = fn(s, T, a, 0.7)
        kd.backward()
        got[tag] = (kd.detach(), [l.detach() for l in per], [x.grad for x in s] + [p.grad for p in a.parameters()])
    assert _rel(got["mine"][0], got["ref"][0]) < 1e-12
    for a, b in zip(got["mine"][1], got["ref"][1]):
        assert _rel(a, b) < 1e-12
    assert len(got["mine"][2]) == 2 + 4
    for a, b in zip(got["mine"][2], got["ref"][2]):
        assert _rel(a, b) < 1e-12


def _teacher_and_pruned_student(prune_skip=False):
    from cleanumamba_amd.network import CleanUMamba
    from cleanumamba_amd.pruning import CleanUMambaPrunableChannels, prune
    sd, cfg = load_ckpt("442k")
    nets = []
    for _ in range(2):
        net = CleanUMamba(**cfg)
        net.load_state_dict(sd, strict=True)
        nets.append(net)
    teacher, student = nets
    groups = CleanUMambaPrunableChannels(student)
    assert groups[0].name == "encode_down_0" and groups[3].name == "encode_down_1" and groups[2].name == "skip_conn_0"
    sel = {groups[0]: [1, 29], groups[3]: [1, 61]}
    if prune_skip:
        sel[groups[2]] = [0, 5, 9]
    prune(groups, sel, None)
    return teacher, student, cfg


@pytest.fixture(scope="module")
def twins():
    teacher, student, cfg = _teacher_and_pruned_student()
    return R.cpu_twin(teacher, cfg).eval(), R.cpu_twin(student, cfg).train()


def test_loss_fn_with_a_teacher_equals_the_chain_in_f64(twins):
    from cleanumamba_amd.training.distill import make_adapters
    from cleanumamba_amd.util.util import loss_fn
    t64, s64 = twins
    ads = make_adapters(s64, t64)
    assert len(ads) == 9 and all(p.dtype == torch.float64 for p in ads.parameters())
    clean, noisy = (x.double() for x in synth.waveform(2, 8000, seed=3))
    ref_ads = copy.deepcopy(ads)
    loss, dic = loss_fn(s64, (clean, noisy), teacher_net=t64, student_teacher_adapter_layers=ads, kd_p=0.5)
    with torch.no_grad():
        _, sf = s64(noisy, return_skip_connections=True)
        _, tf = t64(noisy, return_skip_connections=True)
        kd, per = R.kd_chain(sf, tf, ref_ads, 0.5)
        base, base_dic = loss_fn(s64, (clean, noisy))
    assert len(dic["kd_losses"]) == 9 and not dic["kd_loss"].requires_grad
    assert _rel(dic["kd_loss"], kd) < 1e-12
    for a, b in zip(dic["kd_losses"], per):
        assert not a.requires_grad and _rel(a, b) < 1e-12
    assert _rel(loss.detach(), kd + base) < 1e-12
    for k in base_dic:
        assert _rel(dic[k], base_dic[k]) < 1e-12
    loss.backward()
    assert all(p.grad is not None for p in ads.parameters())
    assert all(p.grad is None for p in t64.parameters())
    for a, b in zip(ads.buffers(), ref_ads.buffers()):          # the BatchNorms moved as the chain's did
        assert torch.equal(a, b)


def test_running_statistics_after_two_calls_are_batchnorms():
    from cleanumamba_amd.training.distill import kd_feature_loss
    g = torch.Generator().manual_seed(8)
    ads = _adapters((5,), (7,))
    bn_s, bn_t = (nn.BatchNorm1d(7, eps=1e-4, affine=False).double() for _ in range(2))
    for _ in range(2):
        s, t = torch.randn(3, 5, 9, generator=g, dtype=torch.float64), torch.randn(3, 7, 9, generator=g, dtype=torch.float64)
        kd_feature_loss([s], [t], ads, 1)
        with torch.no_grad():
            bn_s(ads[0]["embed"](s)), bn_t(t)
    for mine, want in ((ads[0]["bn_s"], bn_s), (ads[0]["bn_t"], bn_t)):
        assert int(mine.num_batches_tracked) == 2 == int(want.num_batches_tracked)
        assert _rel(mine.running_mean, want.running_mean) < 1e-12 and _rel(mine.running_var, want.running_var) < 1e-12


def test_make_adapters_follows_the_pruned_student_and_refuses_mismatches():
    from cleanumamba_amd.network import CleanUMamba
    from cleanumamba_amd.training.distill import check_adapters, feature_channels, kd_feature_loss, make_adapters
    teacher, student, cfg = _teacher_and_pruned_student(prune_skip=True)
    assert feature_channels(teacher) == [64] * 7 + [32, 64]
    assert feature_channels(student) == [64] * 7 + [29, 64]
    ads = make_adapters(student, teacher, eps=1e-3, momentum=0.2)
    assert isinstance(ads, nn.ModuleList) and len(ads) == 9
    for ad, a, b in zip(ads, feature_channels(student), feature_channels(teacher)):
        assert isinstance(ad, nn.ModuleDict) and tuple(ad["embed"].weight.shape) == (b, a, 1)
        for k in ("bn_s", "bn_t"):
            assert type(ad[k]) is nn.BatchNorm1d and ad[k].num_features == b and not ad[k].affine
            assert ad[k].eps == 1e-3 and ad[k].momentum == 0.2
    check_adapters(student, ads)
    with pytest.raises(ValueError, match="after pruning"):
        check_adapters(teacher, ads)                            # (an un-pruned student no longer fits them)
    shallow = CleanUMamba(**dict(cfg, encoder_n_layers=6))
    with pytest.raises(ValueError, match="encoder_n_layers"):
        make_adapters(shallow, teacher)
    one = _adapters((4,), (4,))
    with pytest.raises(ValueError):                             # n < 2, as torch's BatchNorm
        kd_feature_loss([torch.randn(1, 4, 1, dtype=torch.float64)], [torch.randn(1, 4, 1, dtype=torch.float64)], one, 1)
    with pytest.raises(ValueError):
        kd_feature_loss([torch.randn(2, 4, 3)], [], one, 1)


def test_cross_entropy_still_raises_and_the_plain_loss_is_unchanged(twins):
    from cleanumamba_amd.util.util import loss_fn
    _, s64 = twins
    clean, noisy = (x.double() for x in synth.waveform(1, 4000, seed=9))
    with pytest.raises(NotImplementedError):
        loss_fn(s64, (clean, noisy), cross_entropy=True)
    with pytest.raises(ValueError):
        loss_fn(s64, (clean, noisy), teacher_net=s64)           # a teacher without adapters
    with torch.no_grad():
        loss, dic = loss_fn(s64, (clean, noisy), ell_p=1, ell_p_lambda=1, stft_lambda=1)
        den = s64(noisy)
    assert set(dic) == {"reconstruct", "stft_sc", "stft_mag"}
    want_l1 = torch.nn.functional.l1_loss(den, clean)
    assert torch.equal(dic["reconstruct"], want_l1)
    assert torch.equal(loss, want_l1 * 1 + (dic["stft_sc"] + dic["stft_mag"]))


def test_train_step_distill_on_the_host_keeps_the_teacher_out(twins):
    """TrainStep(distill=...) without a GPU (torch optimizer): the adapters train, the teacher does not, and an adapter
    that no longer fits the student raises."""
    from cleanumamba_amd.training.distill import make_adapters
    from cleanumamba_amd.training.train_step import TrainStep
    t64, s64 = (copy.deepcopy(m) for m in twins)
    ads = make_adapters(s64, t64)
    t64.train()
    step = TrainStep(s64, loss_config={"kd_p": 1}, distill=(t64, ads))
    assert not t64.training and not any(p.requires_grad for p in t64.parameters())
    owned = {id(p) for g in step.optimizer.param_groups for p in g["params"]}
    assert owned == {id(p) for p in s64.parameters()} | {id(p) for p in ads.parameters()}
    before = [p.detach().clone() for p in ads.parameters()]
    clean, noisy = (x.double() for x in synth.waveform(2, 4000, seed=2))
    loss, _ = step(clean, noisy)
    assert bool(torch.isfinite(loss)) and any(not torch.equal(a, b) for a, b in zip(before, ads.parameters()))
    with pytest.raises(ValueError, match="after pruning"):
        TrainStep(twins[0], distill=(t64, make_adapters(_teacher_and_pruned_student(prune_skip=True)[1], t64)))
