"""Layer-wise pruning calibration on the host: the calibrator's arithmetic (EMA, floor, default scale, in-place log) and
the scale / offset formulas against the reference's recorded values (tests/golden/calibration_*.npz from
tools/make_golden_calibration.py), data handling, and the argument checks of cum_prune_mask (no GPU needed)."""
import ctypes

import pytest
import torch

from conftest import golden_json, load_golden

MODELS = ["442k", "e6_pruned500k"]


def _rows(f, tag):
    names = golden_json(f["group_names"])
    return [{"group": names[g], "prune_percentage": float(p), "total_importance": float(t), "loss_change": float(d)}
            for g, p, t, d in zip(f[f"{tag}.group"], f[f"{tag}.prune_percentage"], f[f"{tag}.total_importance"],
                                  f[f"{tag}.loss_change"])]


def _scales(f, prefix, key="scales"):
    names = golden_json(f["group_names"])
    return {names[g]: float(s) for g, s in zip(f[f"{prefix}.groups" if key == "scales" and f"{prefix}.groups" in f
                                                 else f"{prefix}.scale_groups"], f[f"{prefix}.{key}"])}


@pytest.mark.parametrize("key", MODELS)
@pytest.mark.parametrize("tag", ["one", "two"])
def test_scales_and_offsets_from_the_reference_rows(key, tag):
    from cleanumamba_amd.pruning.layerwise_calibration import scales_from_results
    f = load_golden("calibration_" + key)
    scales, offsets = scales_from_results(_rows(f, tag), two_point=(tag == "two"))
    assert scales == _scales(f, tag, "scales")
    assert offsets == _scales(f, tag, "offsets")
    assert len(scales) > 0


def test_normalize_scales_is_in_place():
    from cleanumamba_amd.pruning.layerwise_calibration import normalize_scales
    s = {"a": 2.0, "b": 8.0, "c": -4.0}
    out, top = normalize_scales(s)
    assert out is s and top == 8.0 and s == {"a": 0.25, "b": 1.0, "c": -0.5}


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(4, 4)

    def forward(self, x):
        return self.lin(x)


def _tiny_loss(model, X):
    clean, noisy = X
    return ((model(noisy) - clean) ** 2).mean(), {}


@pytest.mark.parametrize("key", MODELS)
def test_calibrator_ema_floor_default_and_log(monkeypatch, key):
    """Two gathers (EMA 0.5, min_scale floor) and one log() reproduce the reference calibrator's recorded state; gather
    zeroes the gradients; an unknown group gets the default factor 36."""
    from cleanumamba_amd.pruning import layerwise_calibration as LC
    f = load_golden("calibration_" + key)
    measured = [_scales(f, "one", "scales"), _scales(f, "raw_b", "scales")]
    calls = []

    def fake(model, groups, loss_fn, metric, root, two_point, batch_size, loss_samples, seed):
        calls.append(metric)
        return dict(measured[len(calls) - 1]), {}, []

    monkeypatch.setattr(LC, "get_calibration", fake)
    model = _Tiny()
    cal = LC.calibrator(0.5)
    for tag in ("cal_a", "cal_b"):
        model.lin.weight.grad = torch.ones(4, 4)
        cal.gather(model, [], _tiny_loss, "taylor_squared_individual", None, 2, 4, 42)
        assert model.lin.weight.grad is None or float(model.lin.weight.grad.abs().sum()) == 0.0
        assert cal.scales == _scales(f, tag, "scales")
    assert calls == ["n_parameters*taylor_squared_individual"] * 2
    assert min(cal.scales.values()) >= cal.min_scale
    log = cal.log({})
    assert log["Prune/calibration_scales/max_scale"] == float(f["cal_log.max_scale"])
    assert cal.scales == _scales(f, "cal_log", "scales")            # normalised in place
    for g, s in cal.scales.items():
        assert log[f"Prune/calibration_scales/{g}"] == s

    class G:
        name = "no_such_group"
    assert torch.equal(cal.scale(torch.tensor([1.0, 2.0]), G()), torch.tensor([36.0, 72.0]))
    G.name = next(iter(cal.scales))
    assert torch.equal(cal.scale(torch.tensor([2.0]), G()), torch.tensor([2.0]) * cal.scales[G.name])


def test_string_root_raises():
    from cleanumamba_amd.pruning.layerwise_calibration import get_calibration
    with pytest.raises(NotImplementedError, match="path"):
        get_calibration(_Tiny(), [], _tiny_loss, "n_parameters*taylor_squared_individual", "/datasets/DNS-Challenge")


def test_callable_root_is_called_once_per_pass_and_stops_at_loss_samples():
    from cleanumamba_amd.pruning.layerwise_calibration import calibrate_prune_groups
    g = torch.Generator().manual_seed(0)
    batches = [(torch.randn(2, 4, generator=g), torch.randn(2, 4, generator=g)) for _ in range(4)]
    calls, seen = [], []

    def root():
        calls.append(1)
        for b in batches:
            seen.append(b)
            yield b

    timings = {}
    model = _Tiny()
    rows = calibrate_prune_groups(model, [], [0.2], _tiny_loss, "n_parameters*taylor_squared_individual", root,
                                  loss_samples=3, timings=timings)
    assert rows == [] and len(calls) == 1
    assert len(seen) == 2                          # 2 + 2 clips reach loss_samples = 3: the pass stops there
    with torch.no_grad():
        want = sum(float(_tiny_loss(model, b)[0]) for b in batches[:2]) / 2
    assert abs(timings["baseline_loss"] - want) < 1e-6
    assert model.lin.weight.grad is not None       # the baseline's gradients stay for the caller
    with pytest.raises(ValueError, match="no batch"):
        calibrate_prune_groups(model, [], [0.2], _tiny_loss, "x", [])


def _desc(hip, w, numel, rows, n_rows, first, row_stride=1, n0=1, s0=0):
    d = hip.PruneMaskDesc()
    d.w, d.numel, d.rows, d.n_rows, d.first = w, numel, rows, n_rows, first
    d.row_stride, d.n0, d.s0, d.n1, d.s1 = row_stride, n0, s0, 1, 0
    return d


def test_prune_mask_argument_checks():
    """Descriptors are validated on the host before anything is uploaded or launched (no GPU needed)."""
    from cleanumamba_amd import hip
    lib = hip.lib()
    base = 1 << 20                                   # fake device addresses: nothing is dereferenced before the checks
    descs = (hip.PruneMaskDesc * 2)(_desc(hip, base, 12, 3, 2, 0, row_stride=4, n0=4, s0=1),
                                    _desc(hip, base + 64, 5, 5, 1, 2))
    assert lib.cum_prune_mask_save_elems(descs, 2) == 2 * 4 + 1
    assert lib.cum_prune_mask_workspace_bytes(2, 3) > 0

    def run(idx, ds=descs, n=2, n_save=9):
        arr = (ctypes.c_int32 * len(idx))(*idx)
        return lib.cum_prune_mask(ds, n, arr, len(idx), None, n_save, 0, None, 0, None)

    for idx, msg in (([0, 3, 1], b"row list"), ([2, 1, 4], b"row list"), ([1, 1, 4], b"row list"),
                     ([0, 2, 5], b"row list")):
        assert run(idx) != 0 and msg in lib.cum_last_error(), idx
    assert run([0, 2, 4], n_save=8) != 0 and b"save buffer" in lib.cum_last_error()
    over = (hip.PruneMaskDesc * 2)(_desc(hip, base, 12, 3, 1, 0, row_stride=4, n0=4, s0=1),
                                   _desc(hip, base + 40, 5, 5, 1, 1))
    assert run([0, 1], ds=over) != 0 and b"overlapping" in lib.cum_last_error()
    past = (hip.PruneMaskDesc * 1)(_desc(hip, base, 11, 3, 1, 0, row_stride=4, n0=4, s0=1))
    assert run([0], ds=past, n=1) != 0 and b"past its tensor" in lib.cum_last_error()
    assert run([0, 2, 4], n_save=9) != 0 and b"save" in lib.cum_last_error()     # valid tables, NULL save buffer
