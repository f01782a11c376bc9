"""Layer-wise pruning calibration on the GPU: the in-place trial mask (cum_prune_mask) zeroes exactly what a prune
removes and restores bit-exact; a masked trial measures the loss of the physically pruned model; get_calibration and
the calibrated selection against the reference's own calibration (tests/golden/calibration_*.npz); a TrainStep's
training state survives a gather; live streams are refused."""
import itertools

import numpy as np
import pytest
import torch

from conftest import golden_json, load_ckpt, load_golden, record

pytestmark = pytest.mark.gpu

GATHER_METRIC = "n_parameters*taylor_squared_individual"
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


def e8_model(dev):
    from cleanumamba_amd.network import CleanUMamba
    torch.manual_seed(5)
    return CleanUMamba(channels_H=64, max_H=768, encoder_n_layers=8, tsfm_n_layers=3, tsfm_n_head=8, tsfm_d_model=512,
                       tsfm_d_inner=2048).to(dev).train()


def batches(f, dev, name="a"):
    clean, noisy = f[f"batches_{name}.clean"], f[f"batches_{name}.noisy"]
    return [(torch.from_numpy(c).to(dev), torch.from_numpy(n).to(dev)) for c, n in zip(clean, noisy)]


def loss_fn(net, X):
    from cleanumamba_amd.util.util import loss_fn as lf
    return lf(net, X)


def trial_indices(group, seed=0):
    """About a fifth of the group's channels (at least one, never all), first and last included when there is room."""
    n = group.n_channels
    k = max(1, min(n - 1, n // 5))
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed + n)).tolist()
    pick = set(perm[:k])
    if k >= 3:
        pick = set(perm[:k - 2]) | {0, n - 1}
    return sorted(pick)


@pytest.mark.parametrize("key", ["442k", "e6_pruned500k", "e8"])
def test_mask_zeroes_exactly_the_removed_rows_and_restores_bitwise(cuda, key):
    from cleanumamba_amd.pruning import CleanUMambaPrunableChannels
    from cleanumamba_amd.pruning.device import TrialMask
    from cleanumamba_amd.training.flat_optim import FlatParams
    net = e8_model(cuda) if key == "e8" else model(key, cuda)[0]
    flat = FlatParams(net)
    where = {id(p): (o, p) for p, o in zip(flat.params, flat.offsets)}
    before = flat.data.clone()
    groups = CleanUMambaPrunableChannels(net)
    seen_xproj_state = False
    for gi, group in enumerate(groups):
        idxs = trial_indices(group, gi)
        want = before.clone()
        for pm in group.modules:
            rows = torch.tensor(pm.removed_rows(idxs, group.n_channels), dtype=torch.long, device=cuda)
            for t, dim in ((pm.param(), pm.dim), (pm.bias(), 0)):
                if t is None:
                    continue
                o, p = where[id(t)]
                want[o:o + p.numel()].view_as(p).index_fill_(dim, rows, 0.0)
            if pm.module is getattr(net.tsfm_Mamba_layers[0].mixer, "x_proj", None) and pm.dim == 0 and pm.n_heads == 2:
                seen_xproj_state = True
                assert pm.channel_offset == net.tsfm_Mamba_layers[0].mixer.dt_proj.weight.shape[1]
        mask = TrialMask(group, idxs)
        mask.mask()
        assert torch.equal(flat.data, want), group.name
        mask.restore()
        assert torch.equal(flat.data, before), group.name
    assert seen_xproj_state


@pytest.mark.parametrize("key", ["442k", "e6_pruned500k"])
def test_masked_trial_equals_the_physically_pruned_model(cuda, key):
    """Every group but d_model: the loss with the selection zeroed in place equals the loss of a copy pruned through
    prune(); and it moved away from the baseline (stale packed weights would report the baseline)."""
    from cleanumamba_amd.pruning import CleanUMambaPrunableChannels
    from cleanumamba_amd.pruning.layerwise_calibration import calibrate_prune_groups
    f = load_golden("calibration_" + key)
    data = batches(f, cuda)
    out = {}
    for physical in (False, True):
        net, _ = model(key, cuda)
        t = {}
        rows = calibrate_prune_groups(net, CleanUMambaPrunableChannels(net), [0.2], loss_fn, GATHER_METRIC, data,
                                      loss_samples=4, physical=physical, timings=t)
        out[physical] = (rows, t["baseline_loss"])
    (rm, bm), (rp, bp) = out[False], out[True]
    assert bm == bp and len(rm) == len(rp) > 0
    tol = 1e-5
    worst, moved = 0.0, 0
    for a, b in zip(rm, rp):
        assert a["group"] == b["group"] and a["total_importance"] == b["total_importance"]
        la, lb = a["loss_change"] + bm, b["loss_change"] + bp
        err = abs(la - lb) / abs(lb)
        if a["group"] != "d_model":
            worst = max(worst, err)
            assert err <= tol, (a["group"], la, lb)
        if abs(b["loss_change"]) > tol * abs(lb):
            assert abs(a["loss_change"]) > tol * abs(la), (a["group"], a["loss_change"])
            moved += 1
    assert moved >= len(rm) - 2
    record(f"calibration_masked_vs_physical[{key}]", worst)


def _ref_rows(f, tag):
    names = golden_json(f["group_names"])
    rows = []
    for j, g in enumerate(f[f"{tag}.group"]):
        a, b = f[f"{tag}.index_start"][j], f[f"{tag}.index_start"][j + 1]
        sa, sb = f[f"{tag}.scores_start"][j], f[f"{tag}.scores_start"][j + 1]
        rows.append({"group": names[g], "index": sorted(f[f"{tag}.index"][a:b].tolist()),
                     "scores": f[f"{tag}.scores"][sa:sb].astype(np.float64),
                     **{k: f[f"{tag}.{k}"][j].item() for k in ("prune_percentage", "mean_importance", "total_importance",
                                                               "loss_change", "prune_parameters", "prune_groups")}})
    return rows


def _scale_bound(fn, args, tols):
    """Largest change of fn over the corners of the box args +- tols (the propagated bound of a scale)."""
    base = fn(*args)
    worst = 0.0
    for signs in itertools.product((-1, 1), repeat=len(args)):
        worst = max(worst, abs(fn(*[a + s * t for a, s, t in zip(args, signs, tols)]) - base))
    return worst


@pytest.mark.parametrize("key", ["442k", "e6_pruned500k"])
@pytest.mark.parametrize("tag", ["one", "two"])
def test_get_calibration_against_the_reference(cuda, key, tag):
    from cleanumamba_amd.pruning import CleanUMambaPrunableChannels
    from cleanumamba_amd.pruning.layerwise_calibration import get_calibration
    f = load_golden("calibration_" + key)
    net, _ = model(key, cuda)
    groups = CleanUMambaPrunableChannels(net)
    assert [g.name for g in groups] == golden_json(f["group_names"])
    scales, offsets, rows = get_calibration(net, groups, loss_fn, GATHER_METRIC, batches(f, cuda), two_point=(tag == "two"),
                                            batch_size=2, loss_samples=4)
    ref = _ref_rows(f, tag)
    baseline = float(f["baseline_loss"])
    assert [r["group"] for r in rows] == [r["group"] for r in ref]
    worst_d, worst_i, same = 0.0, 0.0, {}
    for r, q in zip(rows, ref):
        # the channels the trial pruned: equal, but for channels whose score is within 1e-4 of the selection's cutoff
        chosen = set(q["index"])
        cutoff = max(q["scores"][i] for i in chosen)
        near = {i for i in range(len(q["scores"])) if abs(q["scores"][i] - cutoff) <= 1e-4 * abs(cutoff)}
        mine = set(r["index"])
        assert (mine ^ chosen) <= near, (r["group"], sorted(mine ^ chosen))
        same[(r["group"], r["prune_percentage"])] = mine == chosen
        if mine != chosen:
            continue
        for k in ("prune_percentage", "prune_parameters", "prune_groups"):
            assert r[k] == q[k], (r["group"], k)
        err_i = abs(r["total_importance"] - q["total_importance"]) / abs(q["total_importance"])
        assert err_i <= 1e-3, (r["group"], r["total_importance"], q["total_importance"])
        worst_i = max(worst_i, err_i)
        d, dr = r["loss_change"], q["loss_change"]
        assert abs(d - dr) <= 1e-5 * baseline + 1e-3 * abs(dr), (r["group"], d, dr)
        worst_d = max(worst_d, abs(d - dr) / (1e-5 * baseline + 1e-3 * abs(dr)))
    record(f"calibration_loss_change_vs_ref[{key},{tag}]", worst_d)
    record(f"calibration_total_importance_vs_ref[{key},{tag}]", worst_i)
    names = golden_json(f["group_names"])
    want = {names[g]: s for g, s in zip(f[f"{tag}.scale_groups"], f[f"{tag}.scales"])}
    assert set(scales) == set(want)
    tol_of = lambda r: (1e-5 * baseline + 1e-3 * abs(r["loss_change"]), 1e-3 * abs(r["total_importance"]))  # noqa: E731
    same_row = lambda r: same.get((r["group"], r["prune_percentage"]), False)  # noqa: E731

    def two(dl, il, dh, ih):
        off = il - dl * (ih - il) / (dh - dl)
        return dh / (ih - off)
    low, checked = ref[0], 0
    for r in ref:                    # the reference's pairing: the last row under 15 % (of any group) is the low point
        if tag == "two" and r["prune_percentage"] < 0.15:
            low = r
            continue
        if tag == "two" and not 0.35 <= r["prune_percentage"] <= 0.45:
            continue
        if not same_row(r) or (tag == "two" and not same_row(low)):
            continue
        if tag == "one":
            bound = _scale_bound(lambda d, i: d / i, (r["loss_change"], r["total_importance"]), tol_of(r))
        else:
            bound = _scale_bound(two, (low["loss_change"], low["total_importance"], r["loss_change"],
                                       r["total_importance"]), tol_of(low) + tol_of(r))
        g = r["group"]
        assert abs(scales[g] - want[g]) <= bound + 1e-12 * abs(want[g]), (g, scales[g], want[g], bound)
        checked += 1
    assert checked >= len(want) // 2
    assert all(np.isfinite(list(offsets.values())))


@pytest.mark.parametrize("key", ["442k", "e6_pruned500k"])
def test_calibrated_selection_matches_the_reference(cuda, key):
    from cleanumamba_amd.pruning import CleanUMambaPrunableChannels, get_prune_channels
    from cleanumamba_amd.pruning.layerwise_calibration import calibrator
    f = load_golden("calibration_" + key)
    names = golden_json(f["group_names"])
    net, _ = model(key, cuda)
    g = torch.Generator().manual_seed(GRAD_SEED)            # the gradients of tools/make_golden_pruning.py
    with torch.no_grad():
        for p in net.parameters():
            fan = max(1, p.numel() // p.shape[0])
            p.grad = (torch.randn(p.shape, generator=g, dtype=torch.float32) * (1e-3 / fan ** 0.5)).to(cuda)
    cal = calibrator(0.5)
    cal.scales = {names[i]: float(s) for i, s in zip(f["cal_log.groups"], f["cal_log.scales"])}
    groups = CleanUMambaPrunableChannels(net)
    chosen, params, _ = get_prune_channels(groups, "taylor_squared_individual*n_filters/n_parameters", None, 0.02, 8,
                                           calibrator_container=cal)
    got = sorted((names.index(e["group"].name), int(e["index"])) for e in chosen)
    want = sorted(zip(f["cal_sel.group"].tolist(), f["cal_sel.index"].tolist()))
    assert got == want
    assert params == int(f["cal_sel.params"])
    # without the calibrator the selection differs (the scales take part)
    plain, _, _ = get_prune_channels(groups, "taylor_squared_individual*n_filters/n_parameters", None, 0.02, 8)
    assert sorted((names.index(e["group"].name), int(e["index"])) for e in plain) != want


def _audio(dev, B=2, L=16000, seed=3):
    g = torch.Generator().manual_seed(seed)
    clean = 0.1 * torch.randn(B, 1, L, generator=g)
    return clean.to(dev), (clean + 0.05 * torch.randn(B, 1, L, generator=g)).to(dev)


def test_gather_keeps_the_training_state(cuda):
    """TrainStep (fp16 autocast: loss scaling on) after two steps: gather leaves the parameters bitwise, the Adam
    moments and the state vector (step count, loss scale) as they were, and zero gradients; the following steps --
    eager, captured, replayed, and a replay after a second gather -- equal those of a twin that was never calibrated."""
    from cleanumamba_amd.pruning import CleanUMambaPrunableChannels
    from cleanumamba_amd.pruning.layerwise_calibration import calibrator
    from cleanumamba_amd.training.train_step import TrainStep
    f = load_golden("calibration_442k")
    data = batches(f, cuda)
    nets = [model("442k", cuda)[0] for _ in range(2)]
    steps = [TrainStep(n, autocast_dtype=torch.float16) for n in nets]
    clean, noisy = _audio(cuda)
    for _ in range(2):
        for s in steps:
            s(clean, noisy)
    cal = calibrator(0.5)
    groups = CleanUMambaPrunableChannels(nets[0])

    def gather_and_check():
        st = steps[0]
        opt, flat = st.optimizer, st.buckets.flat
        torch.cuda.synchronize()
        snap = [t.clone() for t in (flat.data, opt.exp_avg, opt.exp_avg_sq, opt.state_vec)]
        cal.gather(nets[0], groups, loss_fn, "taylor_squared_individual", data, 2, 4, 42)
        torch.cuda.synchronize()
        for a, b in zip((flat.data, opt.exp_avg, opt.exp_avg_sq, opt.state_vec), snap):
            assert torch.equal(a, b)
        flat.settle()
        assert float(flat.grad.abs().max()) == 0.0
        assert flat.intact()

    gather_and_check()
    assert len(cal.scales) > 0
    for i in range(4):                        # step 3 eager, step 4 captured, steps 5-6 replayed
        (l1, n1), (l2, n2) = steps[0](clean, noisy), steps[1](clean, noisy)
        torch.cuda.synchronize()
        assert float(l1) == float(l2) and float(n1) == float(n2), i
    assert steps[0].graph_status == "captured" and steps[1].graph_status == "captured"
    gather_and_check()
    (l1, n1), (l2, n2) = steps[0](clean, noisy), steps[1](clean, noisy)
    assert float(l1) == float(l2) and float(n1) == float(n2)
    for a, b in zip(nets[0].parameters(), nets[1].parameters()):
        assert torch.equal(a, b)


def test_refusals(cuda):
    from cleanumamba_amd.pruning import CleanUMambaPrunableChannels
    from cleanumamba_amd.pruning.layerwise_calibration import get_calibration
    f = load_golden("calibration_e6_pruned500k")
    data = batches(f, cuda)
    net, _ = model("e6_pruned500k", cuda)
    groups = CleanUMambaPrunableChannels(net)
    before = [p.detach().clone() for p in net.parameters()]
    x = (0.1 * torch.randn(1, 1, 16000, generator=torch.Generator().manual_seed(2))).to(cuda)
    net.eval()
    with torch.no_grad():
        net.feed(x[0, :, :6000])
    with pytest.raises(RuntimeError, match="live stream"):
        get_calibration(net, groups, loss_fn, GATHER_METRIC, data, loss_samples=4)
    with torch.no_grad():
        net.flush()
        pool = net.stream_pool(2)
        slots = pool.open(1)
        pool.feed(slots, x[0, :, :3000])
    with pytest.raises(RuntimeError, match="open slots"):
        get_calibration(net, groups, loss_fn, GATHER_METRIC, data, loss_samples=4)
    assert all(torch.equal(a, b) for a, b in zip(net.parameters(), before))
    assert all(p.grad is None for p in net.parameters())
    with torch.no_grad():
        pool.close(slots)
    scales, _, rows = get_calibration(net, groups, loss_fn, GATHER_METRIC, data, loss_samples=4)
    assert rows and all(np.isfinite(r["loss_change"]) for r in rows)
    assert all(torch.equal(a, b) for a, b in zip(net.parameters(), before))
