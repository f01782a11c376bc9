"""Fixtures of structured channel pruning (cleanumamba_amd/pruning/).  BUILD MACHINE ONLY: it reads the reference checkout.

The reference's ``src/pruning/pruninggroup.py`` and ``src/pruning/importance.py`` are imported unmodified.  Before that,
``sys.modules`` stand-ins are registered for what ``src/pruning/util.py`` imports and this machine lacks (wandb,
torchprofile, the dataset loader and validate); the model class is the reference's own, through
oracle.reference_shim.load_reference().  Two models: the 442K experiment checkpoint and CleanUMamba-3N-E6_pruned-500k (odd
widths: d_model 301, d_inner 8 / 8 / 40, d_state 13 in the last block).  Every parameter gets a seeded synthetic gradient
(``synthetic_grads``: the tests regenerate it).  Writes tests/golden/pruning_<model>.npz with
  * every group's name, n_channels, n_parameters, n_filters and importance dict (f32, as the reference computes them);
  * get_prune_channels of the shipped metric at a few perc / max_importance / min_channels settings (group, index,
    importance per entry, prunable_params);
  * after two Adam steps and ``group.prune(idxs, adam)`` of channels 1 and n - 3 of every group: the new shape and the kept
    indices per dimension of every parameter (parameter, gradient and both moments verified to agree here).
Usage: python tools/make_golden_pruning.py
"""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import reference_shim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
REF = reference_shim.REFERENCE_ROOT
MODELS = {"442k": "checkpoints/experiments/Experiment_CleanU_Mamba.pkl",
          "e6_pruned500k": "checkpoints/pruned/CleanUMamba-3N-E6_pruned-500k.pkl"}
METRIC = "taylor_squared_individual*n_filters/n_parameters"
# (n_prune_channels, perc_prune_channels_per_iter, min_channels_per_group, max_prune_importance_per_iter)
SETTINGS = [(None, 0.005, 8, None), (None, 0.02, 8, None), (None, 0.01, 4, 3e-13), (None, 0.05, 16, 1e-9),
            (40, None, 2, None)]
GRAD_SEED = 4242
METRICS = ["weight", "grad", "taylor_individual", "taylor_squared_individual", "taylor_group"]


def synthetic_grads(model, seed=GRAD_SEED):
    """Seeded gradients, one tensor per parameter in registration order: N(0, 1) times 1e-3 / sqrt(fan), so that the
    Taylor sums land near the shipped absolute threshold's scale."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for p in model.parameters():
        fan = max(1, p.numel() // p.shape[0])
        out.append(torch.randn(p.shape, generator=g, dtype=torch.float32) * (1e-3 / fan ** 0.5))
    return out


def install_stand_ins():
    def _mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
    _mod("wandb")
    _mod("torchprofile", profile_macs=lambda *a, **k: 0)
    _mod("src.util.dataset", load_CleanNoisyPairDataset=None)
    _mod("src.util.denoise_eval", validate=None)


def load_model(ref, rel):
    ck = torch.load(os.path.join(REF, rel), map_location="cpu", weights_only=False)
    if "network_config" in ck:
        net = ref.CleanUMamba(**ck["network_config"])
        net.load_state_dict(ck["model_state_dict"], strict=True)
        return net.float(), ck["network_config"]
    net = ck["model"] if "model" in ck else ck
    raise RuntimeError(f"unexpected checkpoint layout {type(net)}")


def load_pruned(ref, rel):
    ck = torch.load(os.path.join(REF, rel), map_location="cpu", weights_only=False)
    cfg = ck["network_config"]
    net = ref.CleanUMamba(**cfg)
    net.load_pruned_state_dict(ck["model_state_dict"])
    return net.float(), cfg


def prune_choice(groups):
    """Channels pruned for the shape / kept-index fixture: 1 and n - 3 of every group of at least 4 channels, so that
    every group (the x_proj offset of d_state / dt_rank and the two-head rows included) takes part."""
    return {gr.name: (sorted({1, gr.n_channels - 3}) if gr.n_channels >= 4 else []) for gr in groups}


def kept_per_dim(tags_new, old_shape):
    """Kept indices per dimension from a tensor whose elements were their own flat index before pruning."""
    flat = tags_new.reshape(-1).round().long()
    coords = np.unravel_index(flat.numpy(), old_shape)
    kept = []
    for k, c in enumerate(coords):
        kept.append(np.unique(c))
    grid = np.ravel_multi_index(np.meshgrid(*kept, indexing="ij"), old_shape).reshape(-1)
    assert np.array_equal(grid, flat.numpy()), "pruned tensor is not a product of per-dimension selections"
    return kept


def main():
    install_stand_ins()
    ref = reference_shim.load_reference()
    pg = importlib.import_module("src.pruning.pruninggroup")
    imp = importlib.import_module("src.pruning.importance")
    for key, rel in MODELS.items():
        net, cfg = (load_model if key == "442k" else load_pruned)(ref, rel)
        net.train()
        out = {"config": np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8), "grad_seed": np.int64(GRAD_SEED)}
        for p, g in zip(net.parameters(), synthetic_grads(net)):
            p.grad = g.clone()
        out["grad_checksum"] = np.float64(sum(float(g.double().abs().sum()) for g in synthetic_grads(net)))
        groups = pg.CleanUMambaPrunableChannels(net, statistics=False)
        names = [gr.name for gr in groups]
        out["group_names"] = np.frombuffer(json.dumps(names).encode(), dtype=np.uint8)
        out["n_channels"] = np.array([gr.n_channels for gr in groups], dtype=np.int64)
        nparam, nfilt = [], []
        for gr in groups:
            d = gr.channel_importances()
            nparam.append(d["n_parameters"])
            nfilt.append(d["n_filters"])
            for m in METRICS:
                out[f"imp.{gr.name}.{m}"] = d[m].detach().float().numpy()
        out["n_parameters"] = np.array(nparam, dtype=np.int64)
        out["n_filters"] = np.array(nfilt, dtype=np.int64)
        for s, (n, perc, minc, maxi) in enumerate(SETTINGS):
            prunable, params, mins = imp.get_prune_channels(groups, METRIC, n, perc, minc, maxi)
            out[f"sel{s}.group"] = np.array([names.index(p["group"].name) for p in prunable], dtype=np.int64)
            out[f"sel{s}.index"] = np.array([int(p["index"]) for p in prunable], dtype=np.int64)
            out[f"sel{s}.importance"] = np.array([float(p["importance"]) for p in prunable], dtype=np.float32)
            out[f"sel{s}.params"] = np.int64(params)
            out[f"sel{s}.min"] = np.array([float(mins[nm]) for nm in names], dtype=np.float32)
        out["settings"] = np.frombuffer(json.dumps(SETTINGS).encode(), dtype=np.uint8)

        # pruning with Adam state: parameters, gradients and moments are replaced by their own flat indices (exact in
        # f64) after two real Adam steps, so that what survives names the kept elements
        tagnet = net.double()
        opt = torch.optim.Adam(tagnet.parameters(), lr=1e-4)
        for _ in range(2):
            for p, g in zip(tagnet.parameters(), synthetic_grads(tagnet)):
                p.grad = g.double()
            opt.step()
        pnames = [n for n, _ in tagnet.named_parameters()]
        old_shapes = {}
        with torch.no_grad():
            for n, p in tagnet.named_parameters():
                tags = torch.arange(p.numel(), dtype=torch.float64).view_as(p)
                old_shapes[n] = tuple(p.shape)
                p.copy_(tags)
                p.grad = tags.clone()
                opt.state[p]["exp_avg"].copy_(tags)
                opt.state[p]["exp_avg_sq"].copy_(tags)
        groups = pg.CleanUMambaPrunableChannels(tagnet, statistics=False)
        by_name = {gr.name: gr for gr in groups}
        chosen = prune_choice(groups)
        for gr in groups:
            by_name[gr.name].prune(chosen[gr.name], opt)
        out["prune_group"] = np.array([names.index(nm) for nm in names for _ in chosen[nm]], dtype=np.int64)
        out["prune_index"] = np.array([i for nm in names for i in chosen[nm]], dtype=np.int64)
        for n, p in tagnet.named_parameters():
            for t in (p.grad, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]):
                assert torch.equal(t, p.data), n
            kept = kept_per_dim(p.detach(), old_shapes[n])
            out[f"pruned.{n}.shape"] = np.array(p.shape, dtype=np.int64)
            for k, kl in enumerate(kept):
                out[f"pruned.{n}.keep{k}"] = kl.astype(np.int32)
        out["param_names"] = np.frombuffer(json.dumps(pnames).encode(), dtype=np.uint8)
        out["pruned_n_channels"] = np.array([gr.n_channels for gr in groups], dtype=np.int64)
        path = os.path.join(OUT, f"pruning_{key}.npz")
        np.savez_compressed(path, **out)
        print(f"{path}: {os.path.getsize(path)} bytes, {len(groups)} groups, {len(out['prune_index'])} channels pruned")


if __name__ == "__main__":
    main()
