"""cum_gated_rmsnorm_fwd / _bwd (csrc/ssd.hip) called directly, against mamba2_ref.gated_rmsnorm_ref in float64 and its
autograd, every element of out, dy, dz and dw inside its own bound (tests/block_bounds.py).

y and z are column slices of a wider row, as the Mamba2 mixer passes them (ld > dim), the rest of each row NaN; so are the
gradient rows.  The forward gives a wave a row (lanes stride the width by 64); the backward gives a workgroup
rows_per_block = ceil(rows / 256) rows, its four waves every fourth of them: 257 rows make that 2 with a last block of
one row, 1030 rows 5 with 206 blocks."""
import pytest
import torch

import block_bounds as bb
import mamba2_ref
from conftest import record, rel_l2

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
TOL = {F32: 1e-5, BF16: 4e-3, F16: 5e-4}
NAN = float("nan")
EPS = 1e-5


def _sliced(vals, col0, ld, cuda):
    """vals [rows, D] -> columns col0 .. col0 + D of a NaN-filled [rows + 1, ld] buffer: (buffer, view)."""
    rows, D = vals.shape
    buf = torch.full((rows + 1, ld), NAN, dtype=vals.dtype, device=cuda)
    view = buf[:rows, col0:col0 + D]
    view.copy_(vals.to(cuda))
    return buf, view


def _run(cuda, rows, D, dt, with_rstd=True):
    from cleanumamba_amd import hip
    lib = hip.lib()
    g = torch.Generator().manual_seed(rows * 7 + D)
    rn = lambda *s: torch.randn(*s, generator=g)
    y, z, dout, w = rn(rows, D).to(dt), rn(rows, D).to(dt), rn(rows, D).to(dt), 1 + 0.1 * rn(D)
    yd, zd, wd = (t.double().requires_grad_(True) for t in (y, z, w))
    od = mamba2_ref.gated_rmsnorm_ref(yd, zd, wd, EPS)
    od.backward(dout.double())
    ref = bb.gated_rmsnorm(y, z, w, EPS, dt, dout)
    for name, t in (("out", od.detach()), ("dy", yd.grad), ("dz", zd.grad), ("dw", wd.grad.view(1, D))):
        assert float((ref[name][0] - t).abs().max()) <= 1e-11 * (1 + float(t.abs().max())), name
        ref[name] = (t, ref[name][1])

    ld = 2 * D + 24                                   # one row holds [8 | y | 8 | z | 8], like the mixer's zxbcdt
    zeros = torch.zeros(rows, D, dtype=dt)
    (ybuf, yv), (zbuf, zv) = _sliced(y, 8, ld, cuda), _sliced(z, D + 16, ld, cuda)
    (obuf, ov), (gbuf, gv) = _sliced(zeros, 8, D + 16, cuda), _sliced(dout, 0, D + 8, cuda)
    (dybuf, dyv), (dzbuf, dzv) = _sliced(zeros, 8, ld, cuda), _sliced(zeros, D + 16, ld, cuda)
    wv = w.to(cuda)
    rstd = torch.full((rows + 64,), NAN, device=cuda)
    dw = torch.full((D + 64,), NAN, device=cuda)
    ws = torch.full((max(lib.cum_gated_rmsnorm_bwd_workspace_elems(D), 1),), NAN, device=cuda)
    dc = hip.dtype_code(dt)
    with torch.cuda.device(cuda):
        if not with_rstd:      # the inference form keeps no statistics
            o2buf, o2 = _sliced(zeros, 8, D + 16, cuda)
            hip.check(lib.cum_gated_rmsnorm_fwd(dc, rows, D, hip.ptr(yv), ld, hip.ptr(zv), ld, hip.ptr(wv), EPS, hip.ptr(o2),
                                                D + 16, None, hip.stream_ptr()))
        hip.check(lib.cum_gated_rmsnorm_fwd(dc, rows, D, hip.ptr(yv), ld, hip.ptr(zv), ld, hip.ptr(wv), EPS, hip.ptr(ov),
                                            D + 16, hip.ptr(rstd), hip.stream_ptr()))
        hip.check(lib.cum_gated_rmsnorm_bwd(dc, rows, D, hip.ptr(yv), ld, hip.ptr(zv), ld, hip.ptr(wv), hip.ptr(rstd),
                                            hip.ptr(gv), D + 8, hip.ptr(dyv), ld, hip.ptr(dzv), ld, hip.ptr(dw), hip.ptr(ws),
                                            hip.stream_ptr()))
    torch.cuda.synchronize()
    if not with_rstd:
        assert torch.equal(o2, ov)
    got = {"out": ov, "rstd": rstd[:rows].view(rows, 1), "dy": dyv, "dz": dzv, "dw": dw[:D].view(1, D)}
    tag = f"[{rows}x{D}:{dt}]"
    worst = 0.0
    for name, t in got.items():
        worst = max(worst, bb.check(t.cpu(), *ref[name], f"gated_rmsnorm{tag}.{name}"))
        assert rel_l2(t.float(), ref[name][0]) < (TOL[dt] if name in ("out", "dy", "dz") else 1e-5), name
    record(f"gated_rmsnorm{tag}.elem", worst)
    # nothing outside the slices was written
    assert bool(torch.isnan(rstd[rows:]).all()) and bool(torch.isnan(dw[D:]).all())
    for buf, col0 in ((obuf, 8), (dybuf, 8), (dzbuf, D + 16)):
        m = torch.ones_like(buf, dtype=torch.bool)
        m[:rows, col0:col0 + D] = False
        assert bool(torch.isnan(buf[m].float()).all())


@pytest.mark.parametrize("dt", [F32, F16, BF16])
@pytest.mark.parametrize("D", [1, 63, 64, 65, 96, 1000, 4096])
def test_widths(cuda, D, dt):
    _run(cuda, 5, D, dt, with_rstd=D != 96)


@pytest.mark.parametrize("dt", [F32, F16, BF16])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 255, 256, 257, 625, 1030])
def test_rows(cuda, rows, dt):
    _run(cuda, rows, 96, dt)
