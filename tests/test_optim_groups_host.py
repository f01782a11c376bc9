"""Parameter groups of the train step's optimizer, host side (no GPU): the "optimizer" key of TrainStep's
``optimization`` dict (reference: src/training/train.py:126-154), the membership tables of cum_optim_adam_groups
against a per-element map, FlatAdam's checkpoint layout with groups, and the entry's argument checks."""
import ctypes
import random

import pytest
import torch
import torch.nn as nn

from conftest import load_ckpt


def _net442k():
    from cleanumamba_amd.network import CleanUMamba
    sd, cfg = load_ckpt("442k")
    net = CleanUMamba(**cfg)
    net.load_state_dict(sd, strict=True)
    return net.train()


def test_train_step_reads_the_optimizer_key():
    from cleanumamba_amd.training.train_step import TrainStep
    net = _net442k()
    cfg = {"weight_decay": 0.01, "learning_rate": 1e-3, "n_iters": 100}
    step = TrainStep(net, optimization=dict(cfg, optimizer="adamw"), flat_optimizer=False, use_graph=False)
    opt = step.optimizer
    assert type(opt) is torch.optim.AdamW and len(opt.param_groups) == 2
    named = [p for _, p in net.named_parameters() if p.requires_grad]
    want = [[p for p in named if p.dim() >= 2], [p for p in named if p.dim() < 2]]
    assert want[0] and want[1]
    for g, w, wd in zip(opt.param_groups, want, (0.01, 0.0)):
        assert len(g["params"]) == len(w) and all(a is b for a, b in zip(g["params"], w))
        assert g["weight_decay"] == wd
    # the reference's rule, not upstream's _no_weight_decay marks: A_log (2-D) decays, D and dt_bias do not
    by_name = dict(net.named_parameters())
    decays = {id(p) for p in opt.param_groups[0]["params"]}
    for n, p in by_name.items():
        if n.endswith("A_log"):
            assert id(p) in decays, n
        if n.endswith(".D") or n.endswith("dt_proj.bias") or n.endswith("dt_bias"):
            assert id(p) not in decays, n
    with pytest.raises(ValueError, match="Optimizer not supported"):
        TrainStep(_net442k(), optimization=dict(cfg, optimizer="sgd"), flat_optimizer=False, use_graph=False)
    plain = TrainStep(_net442k(), optimization=cfg, flat_optimizer=False, use_graph=False).optimizer
    assert type(plain) is torch.optim.Adam and len(plain.param_groups) == 1
    assert plain.param_groups[0]["weight_decay"] == 0.01


# ------------------------------------------------------------------------------------------------ membership tables
def _layout(numels):
    offsets, off = [], 0
    for n in numels:
        offsets.append(off)
        off += (n + 3) // 4 * 4
    return offsets, off


def _brute_force(numels, gids):
    """Group of every ELEMENT of the flat buffer, padding included (it belongs to the parameter before it)."""
    out = []
    for n, k in zip(numels, gids):
        out += [k] * ((n + 3) // 4 * 4)
    return out


def _walk(tables, tile_elems, total):
    """What the kernel does with the tables, element by element, with its bounds checked."""
    tile_group, seg_end, seg_group = (t.tolist() for t in tables)
    tile4 = tile_elems // 4
    assert len(tile_group) == max(1, (total // 4 + tile4 - 1) // tile4)
    assert len(seg_end) == len(seg_group) >= 1 and seg_end[-1] == total // 4
    assert all(a < b for a, b in zip(seg_end, seg_end[1:]))
    out = []
    for i4 in range(total // 4):
        code = tile_group[i4 // tile4]
        if code >= 0:
            k = code
        else:
            s = -code - 1
            assert 0 <= s < len(seg_end)
            assert s == 0 or seg_end[s - 1] <= i4 // tile4 * tile4, "the walk must start at or before the tile's first float4"
            while seg_end[s] <= i4:
                s += 1
            k = seg_group[s]
        out += [k] * 4
    return out, tile_group


def _check(numels, gids, tile_elems):
    from cleanumamba_amd.training.flat_optim import group_tables
    offsets, total = _layout(numels)
    tables = group_tables(offsets, numels, gids, tile_elems)
    assert all(t.dtype == torch.int32 for t in tables)
    got, tile_group = _walk(tables, tile_elems, total)
    assert got == _brute_force(numels, gids)
    return tile_group, tables


@pytest.mark.parametrize("tile", [1024, 16])
def test_membership_tables_hand_made_layouts(tile):
    T = tile
    # a 1-element parameter; one ending exactly on a tile edge; one starting 4 elements before a tile edge; one spanning
    # more than three tiles; three groups interleaved
    numels = [1, T - 4, 5, T - 12, 7, 3 * T + 4, 2, T - 8 - 4, 4, 9, 1]
    offsets, _ = _layout(numels)
    assert offsets[2] == T                          # parameter 1 ends exactly on a tile edge
    assert (offsets[4] + 4) % T == 0                # parameter 4 starts 4 elements before one
    gids = [0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1]
    tile_group, (_, seg_end, seg_group) = _check(numels, gids, tile)
    assert sum(1 for c in tile_group if c >= 0) >= 2 and any(c < 0 for c in tile_group)
    assert len(seg_end) == len(numels)
    # neighbours of one group merge into one segment; a single group makes every tile uniform
    _, (_, seg_end, _) = _check([3, 5, T, 1], [1, 1, 0, 0], tile)
    assert len(seg_end) == 2
    tile_group, (_, seg_end, _) = _check(numels, [0] * len(numels), tile)
    assert all(c == 0 for c in tile_group) and len(seg_end) == 1
    tile_group, _ = _check([1], [3], tile)          # less than one tile in all
    assert tile_group == [3]
    tile_group, _ = _check([T, T], [0, 1], tile)    # segment edges on tile edges: no mixed tile
    assert tile_group == [0, 1]


def test_membership_tables_random_layouts():
    rng = random.Random(7)
    for trial in range(40):
        tile = rng.choice([16, 64, 1024])
        ngroups = rng.randint(1, 5)
        numels = [rng.choice([1, 2, 3, 4, 5, 9, tile - 4, tile, tile + 1, 3 * tile + 4, rng.randint(1, 4 * tile)])
                  for _ in range(rng.randint(1, 60))]
        gids = [rng.randrange(ngroups) for _ in numels]
        _check(numels, gids, tile)


def test_membership_tables_refuse_a_layout_with_gaps():
    from cleanumamba_amd.training.flat_optim import group_tables
    with pytest.raises(ValueError):
        group_tables([0, 8], [3, 5], [0, 1], 1024)          # 3 elements pad to 4, not 8
    with pytest.raises(ValueError):
        group_tables([0, 4], [3, 5], [0, 1], 1022)


# ------------------------------------------------------------------------------------------------ FlatAdam with groups
def _small():
    return nn.Sequential(nn.Linear(6, 5), nn.LayerNorm(5), nn.Linear(5, 3), nn.Conv1d(3, 2, 4))


def _groups(net, wd=0.1):
    from cleanumamba_amd.training.train_step import decay_groups
    return decay_groups(net, wd)


def test_flat_adam_groups_checkpoint_layout_matches_torch_adamw():
    from cleanumamba_amd.training import flat_optim as fo
    torch.manual_seed(0)
    a, b = _small(), _small()
    b.load_state_dict(a.state_dict())
    ref = torch.optim.AdamW(_groups(b), lr=1e-3)
    for p in b.parameters():
        p.grad = torch.randn_like(p)
    ref.step()
    flat = fo.FlatParams(a)
    opt = fo.FlatAdam(flat, lr=1e-3, groups=_groups(a), decoupled_weight_decay=True)
    assert len(opt.param_groups) == 2 and [g["weight_decay"] for g in opt.param_groups] == [0.1, 0.0]
    assert all(set(g) == {"params", "lr", "betas", "eps", "weight_decay"} for g in opt.param_groups)
    sd, sr = opt.state_dict(), ref.state_dict()
    assert [g["params"] for g in sd["param_groups"]] == [g["params"] for g in sr["param_groups"]] == [[0, 1, 2], [3, 4, 5, 6, 7]]
    assert list(sd["state"]) == list(sr["state"])
    for k, ent in sr["state"].items():
        assert set(sd["state"][k]) == set(ent) == {"step", "exp_avg", "exp_avg_sq"}
        assert sd["state"][k]["exp_avg"].shape == ent["exp_avg"].shape
        assert sd["state"][k]["exp_avg_sq"].shape == ent["exp_avg_sq"].shape
    assert "flat_state" in sd and sd["loss_scaling"] is False

    # round trip: the step count, the moments (numbered through the groups, not in registration order) and each group's
    # lr and weight decay
    c = _small()
    opt_c = fo.FlatAdam(fo.FlatParams(c), lr=5e-2, groups=_groups(c, 0.3), decoupled_weight_decay=True)
    opt_c.load_state_dict(sr)
    assert float(opt_c.state_vec[fo.ST_STEP]) == 1
    assert [g["lr"] for g in opt_c.param_groups] == [1e-3, 1e-3]
    assert [g["weight_decay"] for g in opt_c.param_groups] == [0.1, 0.0]
    back = opt_c.state_dict()
    for k, ent in sr["state"].items():
        assert torch.equal(back["state"][k]["exp_avg"], ent["exp_avg"]), k
        assert torch.equal(back["state"][k]["exp_avg_sq"], ent["exp_avg_sq"]), k
    decay_c = [p for p in c.parameters() if p.dim() >= 2]
    o = opt_c.flat.offsets[opt_c.flat.index[id(decay_c[1])]]          # checkpoint id 1 = the second decaying tensor
    assert torch.equal(opt_c.exp_avg[o:o + decay_c[1].numel()], sr["state"][1]["exp_avg"].reshape(-1))
    sr2 = ref.state_dict()
    sr2["param_groups"][1]["lr"], sr2["param_groups"][0]["weight_decay"] = 7e-4, 0.25
    opt_c.load_state_dict(sr2)
    assert [g["lr"] for g in opt_c.param_groups] == [1e-3, 7e-4]
    assert [g["weight_decay"] for g in opt_c.param_groups] == [0.25, 0.0]

    # another group count is refused, both ways
    one = torch.optim.Adam(b.parameters(), lr=1e-3).state_dict()
    with pytest.raises(ValueError, match="group"):
        opt_c.load_state_dict(one)
    d = _small()
    with pytest.raises(ValueError, match="group"):
        fo.FlatAdam(fo.FlatParams(d), lr=1e-3).load_state_dict(sr)


def test_flat_adam_refuses_bad_groups():
    from cleanumamba_amd.training import flat_optim as fo
    net = _small()
    flat = fo.FlatParams(net)
    ps = list(net.parameters())
    with pytest.raises(ValueError, match=r"in no group"):
        fo.FlatAdam(flat, groups=[{"params": ps[:-1]}])
    with pytest.raises(ValueError, match="more than one group"):
        fo.FlatAdam(flat, groups=[{"params": ps}, {"params": ps[:1]}])
    with pytest.raises(ValueError, match=r"not a parameter of the FlatParams"):
        fo.FlatAdam(flat, groups=[{"params": ps + [nn.Parameter(torch.zeros(3))]}])
    with pytest.raises(ValueError, match="betas"):
        fo.FlatAdam(flat, groups=[{"params": ps[:2]}, {"params": ps[2:], "betas": (0.8, 0.999)}])
    with pytest.raises(ValueError, match="eps"):
        fo.FlatAdam(flat, groups=[{"params": ps[:2]}, {"params": ps[2:], "eps": 1e-6}])
    # the message names the parameter
    with pytest.raises(ValueError, match=r"\(3, 5\)"):
        fo.FlatAdam(flat, groups=[{"params": [p for p in ps if tuple(p.shape) != (3, 5)]}])
    with pytest.raises(ValueError, match="at most"):
        fo.FlatAdam(flat, groups=[{"params": ps}] + [{"params": []} for _ in range(16)])
    ok = fo.FlatAdam(flat, lr=3e-3, weight_decay=0.2, groups=[{"params": ps[:2], "lr": 1e-2}, {"params": ps[2:]}])
    assert [g["lr"] for g in ok.param_groups] == [1e-2, 3e-3]
    assert [g["weight_decay"] for g in ok.param_groups] == [0.2, 0.2]


def test_flat_adam_without_groups_keeps_its_checkpoint_layout():
    """groups=None: one group, registration-order numbering, the keys of before."""
    from cleanumamba_amd.training import flat_optim as fo
    net = _small()
    opt = fo.FlatAdam(fo.FlatParams(net), lr=1e-3, weight_decay=0.01)
    assert not opt.grouped and len(opt.param_groups) == 1 and opt.param_groups[0]["params"] is opt.flat.params
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups", "flat_state", "loss_scaling"}
    assert len(sd["param_groups"]) == 1
    g = sd["param_groups"][0]
    assert set(g) == {"params", "lr", "betas", "eps", "weight_decay"} and g["params"] == list(range(8))
    assert g["weight_decay"] == 0.01 and g["lr"] == 1e-3
    for i, p in enumerate(net.parameters()):                     # id i = i-th parameter in registration order
        assert sd["state"][i]["exp_avg"].shape == p.shape and sd["state"][i]["exp_avg_sq"].shape == p.shape
    assert sorted(sd["state"]) == list(range(8))
    assert not hasattr(opt, "group_hyper")


def test_write_lr_fills_the_group_table():
    from cleanumamba_amd.training import flat_optim as fo
    net = _small()
    opt = fo.FlatAdam(fo.FlatParams(net), lr=1e-3, groups=_groups(net, 0.1), decoupled_weight_decay=True)
    before = opt.group_hyper.data_ptr()
    opt.write_lr()
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
    assert opt.group_hyper.tolist() == [[f32(1e-3), f32(0.1), f32(1.0 - 1e-3 * 0.1), 0.0], [f32(1e-3), 0.0, 1.0, 0.0]]
    opt.param_groups[0]["lr"], opt.param_groups[1]["lr"] = 2e-3, 5e-4          # as a scheduler does
    opt.param_groups[0]["weight_decay"] = 0.05
    opt.write_lr()
    assert opt.group_hyper.tolist() == [[f32(2e-3), f32(0.05), f32(1.0 - 2e-3 * 0.05), 0.0], [f32(5e-4), 0.0, 1.0, 0.0]]
    assert opt.group_hyper.data_ptr() == before                  # a fixed address: a captured graph keeps reading it


# ------------------------------------------------------------------------------------------------ the C entry
def test_adam_groups_entry_rejects_bad_arguments_before_any_launch():
    from cleanumamba_amd import hip
    lib = hip.lib()
    assert lib.cum_optim_group_tile_elems() == 1024 and lib.cum_optim_max_groups() == 16
    ok = ctypes.c_void_p(4096)                                   # never dereferenced: every call below is refused

    def call(p=ok, g=ok, m=ok, v=ok, n=64, state=ok, hyper=ok, ngroups=2, tiles=ok, ends=ok, gids=ok, nseg=1):
        return lib.cum_optim_adam_groups(p, g, m, v, n, state, 0.9, 0.999, 1e-8, 1, hyper, ngroups, tiles, ends, gids,
                                         nseg, None)
    for name in ("p", "g", "m", "v", "state", "hyper", "tiles", "ends", "gids"):
        assert call(**{name: None}) == -1, name
        assert b"null pointer" in lib.cum_last_error(), name
    assert call(hyper=None) == -1 and b"group_hyper" in lib.cum_last_error()
    assert call(state=None) == -1 and b"state" in lib.cum_last_error()
    assert call(ngroups=0) == -1 and b"ngroups" in lib.cum_last_error()
    assert call(ngroups=17) == -1 and b"ngroups" in lib.cum_last_error()
    assert call(n=-1) == -1 and b"n must be" in lib.cum_last_error()
    assert call(nseg=0) == -1 and b"nseg" in lib.cum_last_error()
    assert call(m=ctypes.c_void_p(4100)) == -1 and b"aligned" in lib.cum_last_error()
    assert call(n=0) == 0                                        # nothing to do: no launch either
