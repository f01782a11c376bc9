"""The full-size f64 scan restatement (tests/scan_ref64.py) against the autograd oracle, on the CPU."""
import pytest
import torch

import scan_ref64 as S
from oracle import mamba_ref as M


def _rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


@pytest.mark.parametrize("shape,opts,group", [
    ((3, 7, 5, 19), "plain", 2),               # ragged D, N, L; groups 2 + 1
    ((4, 13, 11, 33), "plain", 3),             # groups 3 + 1
    ((2, 9, 16, 17), "no_z", None),
    ((3, 6, 3, 8), "no_D", 2),
    ((2, 5, 8, 23), "no_bias", 1),
    ((2, 10, 9, 12), "no_softplus", None),
    ((5, 4, 6, 11), "bare", 2),                # no z, no D, no bias, no softplus
    ((3, 11, 7, 21), "a_log", 2),              # A given as A_log
    ((2, 8, 4, 15), "a_log_no_z", 1),
    ((1, 1, 1, 1), "plain", None),
])
def test_scan_ref64_matches_autograd_oracle(shape, opts, group):
    bsz, dim, N, L = shape
    gen = torch.Generator().manual_seed(sum(shape) + len(opts))
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    a_log = opts.startswith("a_log")
    t = dict(u=rn(bsz, L, dim).transpose(1, 2), delta=0.5 * rn(bsz, L, dim).transpose(1, 2),
             A=(0.5 * rn(dim, N)) if a_log else -torch.exp(0.5 * rn(dim, N)),
             B=rn(bsz, L, N).transpose(1, 2), C=rn(bsz, L, N).transpose(1, 2), D=rn(dim),
             z=rn(bsz, L, dim).transpose(1, 2), delta_bias=0.5 * rn(dim))
    softplus = opts not in ("no_softplus", "bare")
    drop = {"no_z": ("z",), "no_D": ("D",), "no_bias": ("delta_bias",), "bare": ("z", "D", "delta_bias"),
            "a_log_no_z": ("z",)}.get(opts, ())
    if not softplus:
        t["delta"] = t["delta"].abs()
    for k in drop:
        t[k] = None
    # a few entries past the softplus threshold exercise its identity branch
    t["delta"][0, 0, 0] = 25.0
    dout = rn(bsz, L, dim).transpose(1, 2)
    ref = {k: (v.detach().clone().requires_grad_(True) if v is not None else None) for k, v in t.items()}
    A_eff = -torch.exp(ref["A"]) if a_log else ref["A"]
    yr, lastr = M.selective_scan_ref(ref["u"], ref["delta"], A_eff, ref["B"], ref["C"], ref["D"], z=ref["z"],
                                     delta_bias=ref["delta_bias"], delta_softplus=softplus, return_last_state=True)
    (yr * dout).sum().backward()
    kw = dict(D=t["D"], z=t["z"], delta_bias=t["delta_bias"], delta_softplus=softplus, a_is_log=a_log)
    y, last = S.selective_scan64(t["u"], t["delta"], t["A"], t["B"], t["C"], return_last_state=True, **kw)
    assert _rel(y, yr) < 1e-12 and _rel(last, lastr) < 1e-12
    g = S.selective_scan64_bwd(dout, t["u"], t["delta"], t["A"], t["B"], t["C"], group=group, **kw)
    assert _rel(g["out"], yr) < 1e-12 and _rel(g["last"], lastr) < 1e-12
    ypre = M.selective_scan_ref(t["u"], t["delta"], A_eff.detach(), t["B"], t["C"], t["D"], z=None,
                                delta_bias=t["delta_bias"], delta_softplus=softplus)
    assert _rel(g["y_pre"], ypre) < 1e-12
    names = dict(u="du", delta="ddelta", A="dA", B="dB", C="dC", D="dD", z="dz", delta_bias="ddelta_bias")
    for k, gk in names.items():
        if t[k] is None:
            assert g[gk] is None, gk
            continue
        assert g[gk].shape == ref[k].grad.shape, gk
        assert _rel(g[gk], ref[k].grad) < 1e-12, gk


def test_scan_ref64_group_split_is_exact_and_f32_close():
    """Grouping only changes the order of the batch sums; the f32 form (the yardstick for full-size kernel bounds) stays
    close to f64."""
    bsz, dim, N, L = 5, 12, 7, 40
    gen = torch.Generator().manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    args = (rn(bsz, dim, L), rn(bsz, L, dim).transpose(1, 2), 0.3 * rn(dim, N), rn(bsz, N, L), rn(bsz, N, L))
    kw = dict(D=rn(dim), z=rn(bsz, dim, L), delta_bias=0.3 * rn(dim), delta_softplus=True, a_is_log=True)
    dout = rn(bsz, dim, L)
    whole = S.selective_scan64_bwd(dout, *args, **kw)
    for grp in (1, 2, 4):
        part = S.selective_scan64_bwd(dout, *args, group=grp, **kw)
        for k, v in whole.items():
            assert _rel(part[k], v) < 1e-14, (grp, k)
    f32 = S.selective_scan64_bwd(dout, *args, dtype=torch.float32, **kw)
    for k, v in whole.items():
        assert f32[k].dtype == torch.float32
        assert _rel(f32[k].double(), v) < 1e-5, k
    # the state budget picks the group size: 2 clips' states of (L + 1) x dim x N doubles
    small = S.selective_scan64_bwd(dout, *args, state_bytes=2 * (L + 1) * dim * N * 8, **kw)
    for k, v in whole.items():
        assert _rel(small[k], v) < 1e-14, k
