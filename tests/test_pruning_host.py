"""Channel pruning on the host (no GPU): groups, selection and the pruned shapes against fixtures made with the
reference's own src/pruning code (tools/make_golden_pruning.py), and the refusals that must leave a model untouched."""
import numpy as np
import pytest
import torch

from conftest import golden_json, load_ckpt, load_golden

MODELS = ["442k", "e6_pruned500k"]
METRIC = "taylor_squared_individual*n_filters/n_parameters"
KEYS = ["weight", "grad", "taylor_individual", "taylor_squared_individual", "taylor_group"]


def cpu_model(key):
    from cleanumamba_amd.network import CleanUMamba
    sd, cfg = load_ckpt(key)
    net = CleanUMamba(**cfg)
    if key == "442k":
        net.load_state_dict(sd, strict=True)
    else:
        net.load_pruned_state_dict(sd)
    return net, sd, cfg


def fixture(key):
    f = load_golden("pruning_" + key)
    return f, golden_json(f["group_names"])


@pytest.mark.parametrize("key", MODELS)
def test_groups_match_the_reference(key):
    from cleanumamba_amd.pruning import CleanUMambaPrunableChannels
    f, names = fixture(key)
    net, _, _ = cpu_model(key)
    groups = CleanUMambaPrunableChannels(net)
    assert [g.name for g in groups] == names
    assert [g.n_channels for g in groups] == f["n_channels"].tolist()
    for g, npar, nf in zip(groups, f["n_parameters"], f["n_filters"]):
        g.check()
        n = sum(pm.n_heads * (pm.param().numel() // pm.param().shape[pm.dim]) for pm in g.modules)
        assert n == npar, g.name
        assert len(g.modules) == nf


def _h(cfg, i):
    return min(cfg["channels_H"] * 2 ** i, cfg["max_H"])


@pytest.mark.parametrize("cfg_name", ["e8", "e6"])
def test_full_size_groups_on_meta_device(cfg_name):
    """The E8 / E6 configs, built on the meta device: group widths and parameter counts from the config alone."""
    from cleanumamba_amd.network import CleanUMamba
    from cleanumamba_amd.pruning import CleanUMambaPrunableChannels
    cfg = {"channels_H": 64, "max_H": 768, "encoder_n_layers": 8 if cfg_name == "e8" else 6, "kernel_size": 4,
           "stride": 2, "tsfm_n_layers": 3, "tsfm_n_head": 8, "tsfm_d_model": 512, "tsfm_d_inner": 2048}
    net = CleanUMamba(**cfg, device="meta")
    groups = CleanUMambaPrunableChannels(net)
    L, K, dm, di = cfg["encoder_n_layers"], cfg["kernel_size"], cfg["tsfm_d_model"], cfg["tsfm_d_inner"]
    ds, dr = dm // cfg["tsfm_n_head"], -(-dm // 16)
    want = []
    for i in range(L):
        H, Hin = _h(cfg, i), (1 if i == 0 else _h(cfg, i - 1))
        want.append((f"encode_down_{i}", H, Hin * K + 2 * H))
        want.append((f"decode_mix_{i}", H, 2 * H + Hin * K))
        tail = 2 * dm if i == L - 1 else 2 * _h(cfg, i + 1) * K
        want.append((f"skip_conn_{i}", H, 2 * H + 2 * H + tail))
    want.append(("d_model", dm, 2 * _h(cfg, L - 1) + 1 + cfg["tsfm_n_layers"] * (1 + 3 * di)))
    for i in range(cfg["tsfm_n_layers"]):
        want.append((f"d_inner{i}", di, 2 * dm + dm + K + dr + 2 * ds + dr + ds + 1))
        want.append((f"d_state{i}", ds, 2 * di + di))
        want.append((f"dt_rank{i}", dr, di + di))
    got = []
    for g in groups:
        n = 0
        for pm in g.modules:
            w = pm.param()
            n += pm.n_heads * (w.numel() // w.shape[pm.dim])
        got.append((g.name, g.n_channels, n))
    assert got == want


@pytest.mark.parametrize("key", MODELS)
def test_selection_matches_the_reference(key):
    """select_prune_channels on the fixture's importances gives the reference's picks at every recorded setting (the
    multiple-of-8 d_inner rule and the importance cap included)."""
    from cleanumamba_amd.pruning import CleanUMambaPrunableChannels, select_prune_channels
    f, names = fixture(key)
    net, _, _ = cpu_model(key)
    groups = CleanUMambaPrunableChannels(net)
    imps = []
    for g, npar, nf in zip(groups, f["n_parameters"], f["n_filters"]):
        d = {k: torch.from_numpy(f[f"imp.{g.name}.{k}"].copy()) for k in KEYS}
        d.update(act_var=None, n_parameters=int(npar), n_filters=int(nf))
        imps.append(d)
    for s, (n, perc, minc, maxi) in enumerate(golden_json(f["settings"])):
        chosen, params, minima = select_prune_channels(groups, [dict(d) for d in imps], METRIC, n, perc, minc, maxi)
        assert [names.index(e["group"].name) for e in chosen] == f[f"sel{s}.group"].tolist(), s
        assert [int(e["index"]) for e in chosen] == f[f"sel{s}.index"].tolist(), s
        np.testing.assert_array_equal(np.array([float(e["importance"]) for e in chosen], dtype=np.float32),
                                      f[f"sel{s}.importance"])
        assert params == int(f[f"sel{s}.params"])
        np.testing.assert_array_equal(np.array([float(minima[nm]) for nm in names], dtype=np.float32), f[f"sel{s}.min"])


def tag_parameters(net):
    """Every element of every parameter becomes its own flat index (exact in f64)."""
    net.double()
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.arange(p.numel(), dtype=torch.float64).view_as(p))


def kept_from_tags(t, old_shape):
    idx = np.unravel_index(t.reshape(-1).round().long().numpy(), old_shape)
    return [np.unique(c) for c in idx]


@pytest.mark.parametrize("key", MODELS)
@pytest.mark.parametrize("batched", [False, True])
def test_prune_cpu_model_with_adam(key, batched):
    """Pruning with a torch.optim.Adam after two steps: shapes and kept indices of every parameter as the reference's
    group.prune left them; gradients and moments follow; the pruned state dict loads strictly into a fresh model."""
    from cleanumamba_amd.network import CleanUMamba
    from cleanumamba_amd.pruning import CleanUMambaPrunableChannels, prune
    f, names = fixture(key)
    net, _, cfg = cpu_model(key)
    tag_parameters(net)
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    g = torch.Generator().manual_seed(0)
    saved = {n: p.detach().clone() for n, p in net.named_parameters()}
    for _ in range(2):
        for p in net.parameters():
            p.grad = torch.randn(p.shape, generator=g, dtype=torch.float64)
        opt.step()
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.copy_(saved[n])
            p.grad = saved[n].clone()
            opt.state[p]["exp_avg"].copy_(saved[n])
            opt.state[p]["exp_avg_sq"].copy_(saved[n])
    old_shapes = {n: tuple(p.shape) for n, p in net.named_parameters()}
    groups = CleanUMambaPrunableChannels(net)
    chosen = {}
    for gi, ci in zip(f["prune_group"], f["prune_index"]):
        chosen.setdefault(names[gi], []).append(int(ci))
    if batched:
        prune(groups, {g: chosen.get(g.name, []) for g in groups}, opt)
    else:
        for grp in groups:
            grp.prune(chosen.get(grp.name, []), opt)
    assert [g.n_channels for g in groups] == f["pruned_n_channels"].tolist()
    for grp in groups:
        grp.check()
    for n, p in net.named_parameters():
        assert list(p.shape) == f[f"pruned.{n}.shape"].tolist(), n
        for k, kl in enumerate(kept_from_tags(p.detach(), old_shapes[n])):
            np.testing.assert_array_equal(kl, f[f"pruned.{n}.keep{k}"], err_msg=n)
        for t in (p.grad, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]):
            assert torch.equal(t, p.detach()), n
    for block in net.tsfm_Mamba_layers:
        mx = block.mixer
        assert mx.d_inner == mx.in_proj.weight.shape[0] // 2 == mx.conv1d.groups
        assert mx.d_state == mx.A_log.shape[1] and mx.dt_rank == mx.dt_proj.weight.shape[1]
        assert mx.d_model == mx.in_proj.in_features == net.tsfm_conv1.out_channels
    fresh = CleanUMamba(**cfg).double()
    fresh.load_pruned_state_dict(net.state_dict())
    for (n, a), b in zip(fresh.state_dict().items(), net.state_dict().values()):
        assert torch.equal(a, b), n


def _snapshot(net):
    return {n: (p.data_ptr(), tuple(p.shape), p.detach().clone()) for n, p in net.named_parameters()}


def _unchanged(net, snap):
    return all(p.data_ptr() == snap[n][0] and tuple(p.shape) == snap[n][1] and torch.equal(p.detach(), snap[n][2])
               for n, p in net.named_parameters())


def test_refusals_leave_the_model_untouched():
    from cleanumamba_amd.pruning import CleanUMambaPrunableChannels, PruningModule, prune
    net, _, _ = cpu_model("442k")
    groups = CleanUMambaPrunableChannels(net)
    by = {g.name: g for g in groups}
    snap = _snapshot(net)
    n_before = [g.n_channels for g in groups]
    cases = [
        (IndexError, lambda: by["d_model"].prune([0, by["d_model"].n_channels])),
        (IndexError, lambda: by["encode_down_0"].prune([-1])),
        (ValueError, lambda: by["d_state0"].prune([3, 3])),
        (ValueError, lambda: by["dt_rank1"].prune(list(range(by["dt_rank1"].n_channels)))),
        (ValueError, lambda: by["skip_conn_1"].prune([0.5])),
        # a batched prune refused in its last group changes nothing in the first ones
        (ValueError, lambda: prune(groups, {groups[0]: [0, 1], groups[-1]: list(range(groups[-1].n_channels))})),
    ]
    for exc, fn in cases:
        with pytest.raises(exc):
            fn()
        assert _unchanged(net, snap)
        assert [g.n_channels for g in groups] == n_before
    with pytest.raises(NotImplementedError, match="forward hooks"):
        CleanUMambaPrunableChannels(net, statistics=True)
    with pytest.raises(NotImplementedError, match="forward hooks"):
        PruningModule(net.tsfm_conv1, statistics=True)
    # importances of a CPU model: no CPU fallback
    for p in net.parameters():
        p.grad = torch.zeros_like(p)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        by["d_model"].channel_importances()
    assert _unchanged(net, snap)


def test_prune_refused_under_a_gradient_exchange():
    """World > 1: every rank would have to prune the same channels; refused before anything changes."""
    from cleanumamba_amd.pruning import CleanUMambaPrunableChannels
    from cleanumamba_amd.training.train_distributed import GradBuckets
    net, _, _ = cpu_model("442k")
    buckets = GradBuckets(net)
    buckets.world, buckets.exchanging = 2, True            # as an initialised two-rank group would set them
    groups = CleanUMambaPrunableChannels(net)
    snap = _snapshot(net)
    with pytest.raises(NotImplementedError, match="several ranks"):
        groups[0].prune([0])
    assert _unchanged(net, snap) and buckets.flat.intact()


def test_plain_data_assignment_still_orphans_a_flat_parameter():
    """Pruning's own path re-points views; a bare ``p.data = ...`` is still refused at the next step."""
    from cleanumamba_amd.training.flat_optim import FlatParams
    net, _, _ = cpu_model("442k")
    flat = FlatParams(net)
    net.tsfm_conv1.weight.data = net.tsfm_conv1.weight.data[:-1].clone()
    with pytest.raises(RuntimeError, match="re-allocated"):
        flat.require_intact()


def test_whole_model_save_after_flat_storage():
    """A model holding GradBuckets / FlatParams with a FlatAdam still saves whole (the reference's pruning loop does
    torch.save({'model': model, ...})); the back-references are dropped from the pickle, nothing else."""
    import io
    from cleanumamba_amd.training.flat_optim import FlatAdam
    from cleanumamba_amd.training.train_distributed import GradBuckets
    net, _, _ = cpu_model("442k")
    net.grad_buckets = GradBuckets(net)
    adam = FlatAdam(net.grad_buckets.flat)
    assert net.grad_buckets.flat.optimizer() is adam and net.grad_buckets.flat.buckets() is net.grad_buckets
    buf = io.BytesIO()
    torch.save(net, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=False)
    assert back.grad_buckets.flat.optimizer is None and back.grad_buckets.flat.buckets is None
    for a, b in zip(back.state_dict().values(), net.state_dict().values()):
        assert torch.equal(a, b)
