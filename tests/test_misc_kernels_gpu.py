"""Small C-ABI entry points against their torch equivalents (GPU): operand gather, hipFFT wrappers, the waveform-end
kernels of csrc/loss.hip (time-domain loss term, per-clip std, input / output framing), the streaming glue of
csrc/stream.hip (window update on every path, overlap-add)."""
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("src_dt,dst_dt", [(torch.float32, torch.bfloat16), (torch.float32, torch.float32),
                                           (torch.bfloat16, torch.float32), (torch.bfloat16, torch.bfloat16),
                                           (torch.float32, torch.float16), (torch.float16, torch.float32),
                                           (torch.float16, torch.float16)])
@pytest.mark.parametrize("n", [1, 7, 8, 1000, 100003])
def test_gather_with_zero_padding(cuda, src_dt, dst_dt, n):
    from cleanumamba_amd.network import convstack as cs
    g = torch.Generator().manual_seed(n)
    src = torch.randn(5000, generator=g).to(src_dt)
    idx = torch.randint(-1, 5000, (n,), generator=g, dtype=torch.int32)
    out = cs.gather(src.to(cuda), idx.to(cuda), dst_dt)
    want = torch.where(idx >= 0, src[idx.clamp_min(0).long()].float(), torch.zeros(n)).to(dst_dt)
    assert out.dtype == dst_dt and torch.equal(out.cpu(), want)      # pure data movement + one rounding: bit-exact


@pytest.mark.parametrize("n_fft", [512, 1024, 2048])
def test_rfft_irfft_match_torch_fft(cuda, n_fft):
    """Real transforms through caller-owned plans (cum_fft_plan_create / cum_fft_exec: hipFFT, unnormalised, inputs may be
    overwritten, work area passed in) vs torch.fft on a copy."""
    from cleanumamba_amd import hip
    batch = 37
    x = torch.randn(batch, n_fft, generator=torch.Generator().manual_seed(n_fft)).to(cuda)
    want = torch.fft.rfft(x.clone(), dim=-1)
    spec = torch.empty(batch, n_fft // 2 + 1, dtype=torch.complex64, device=cuda)
    scratch = x.clone()
    hip.fft(hip.FFT_R2C, n_fft, batch, scratch, torch.view_as_real(spec))
    assert rel_l2(torch.view_as_real(spec), torch.view_as_real(want)) < 1e-6
    back_want = torch.fft.irfft(want.clone(), n=n_fft, dim=-1, norm="forward")
    back = torch.empty(batch, n_fft, device=cuda)
    z = want.clone()
    hip.fft(hip.FFT_C2R, n_fft, batch, torch.view_as_real(z), back)
    assert rel_l2(back, back_want) < 1e-6
    assert rel_l2(back / n_fft, x) < 1e-5                            # round trip


@pytest.mark.parametrize("n", [256, 1024])
def test_cfft_matches_torch_fft(cuda, n):
    """Complex plan (hipFFT c2c, in place, unnormalised both ways) against torch.fft in float64."""
    from cleanumamba_amd import hip
    g = torch.Generator().manual_seed(n)
    z = torch.randn(37, n, 2, generator=g)
    ref = torch.fft.fft(torch.view_as_complex(z.double()))
    buf = z.to(cuda).contiguous()
    with torch.cuda.device(cuda):
        hip.fft(hip.FFT_C2C, n, 37, buf, buf)
    got = torch.view_as_complex(buf.double().cpu())
    assert float((got - ref).abs().max() / ref.abs().max()) < 2e-6
    with torch.cuda.device(cuda):
        hip.fft(hip.FFT_C2C, n, 37, buf, buf, inverse=True)
    back = buf.cpu() / n
    assert float((back - z).abs().max()) < 1e-5


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16])
def test_stream_window_update_and_tail_rows(cuda, dt):
    """The streaming encoder glue against plain slicing: window <- cat(window[n_new:], new rows) with `fresh` either a
    whole recomputed window or only the new rows; tail_rows copies the newest rows into a compact clip buffer."""
    from cleanumamba_amd import hip
    S, rows, n_new, Cp, pitch = 5, 22, 8, 24, 24
    g = torch.Generator().manual_seed(3)
    window = torch.randn(S, pitch, Cp, generator=g).to(dt).to(cuda)
    full = torch.randn(S, pitch, Cp, generator=g).to(dt).to(cuda)
    want = torch.cat([window[:, n_new:rows], full[:, rows - n_new:rows]], 1)
    lib, dc = hip.lib(), hip.dtype_code(dt)
    for compact in (False, True):
        w = window.clone()
        fresh = full[:, rows - n_new:rows].contiguous() if compact else full
        tmp = torch.empty(S * rows * Cp, dtype=dt, device=cuda)
        with torch.cuda.device(cuda):
            nxt = torch.zeros(S, n_new + 4, Cp, dtype=dt, device=cuda)
            hip.check(lib.cum_stream_window_update(dc, S, rows, n_new, Cp, hip.ptr(w), hip.ptr(fresh), pitch,
                                                   n_new if compact else pitch, rows - n_new if compact else 0,
                                                   hip.ptr(tmp), hip.ptr(nxt) if compact else None, n_new + 4,
                                                   hip.stream_ptr()))
        assert torch.equal(w[:, :rows], want)
        assert torch.equal(w[:, rows:], window[:, rows:])                 # rows beyond the window are untouched
        if compact:       # the next layer's compact input: the n_new + 2 newest rows of the updated window
            assert torch.equal(nxt[:, :n_new + 2], want[:, rows - n_new - 2:]) and float(nxt[:, n_new + 2:].abs().max()) == 0
    dst = torch.zeros(S, 12, Cp, dtype=dt, device=cuda)
    with torch.cuda.device(cuda):
        hip.check(lib.cum_stream_tail_rows(dc, S, 10, Cp, hip.ptr(window), pitch, rows - 10, hip.ptr(dst), 12,
                                           hip.stream_ptr()))
    assert torch.equal(dst[:, :10], window[:, rows - 10:rows]) and float(dst[:, 10:].abs().max()) == 0.0
    with pytest.raises(RuntimeError):
        hip.check(lib.cum_stream_tail_rows(dc, S, 10, Cp, hip.ptr(window), pitch, rows, hip.ptr(dst), 12,
                                           hip.stream_ptr()))                # source rows out of range


@pytest.mark.parametrize("rows,cols", [(114, 85), (85, 114), (300, 1000), (7, 3)])
def test_small_linear_matches_torch(cuda, rows, cols):
    """cum_small_linear (one workgroup per stream; LDS-staged matrix when it is small, wave-per-row otherwise)."""
    from cleanumamba_amd import hip
    g = torch.Generator().manual_seed(rows)
    x, W, b = torch.randn(37, cols, generator=g), torch.randn(rows, cols, generator=g) / cols ** 0.5, torch.randn(rows, generator=g)
    out = torch.empty(37, rows, device=cuda)
    xd, Wd, bd = x.to(cuda), W.to(cuda), b.to(cuda)
    with torch.cuda.device(cuda):
        hip.check(hip.lib().cum_small_linear(37, rows, cols, hip.ptr(xd), cols, hip.ptr(Wd), hip.ptr(bd), hip.ptr(out), rows,
                                             hip.stream_ptr()))
    ref = x.double() @ W.double().t() + b.double()
    assert rel_l2(out, ref) < 1e-6


@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 1, 4099), (16, 1, 160000)])
def test_lp_loss_matches_torch_and_replays_in_a_graph(cuda, p, shape):
    """cum_lp_loss_fwd / _bwd (F.l1_loss / F.mse_loss of src/util/util.py:262-268) against torch in f64, and the value
    a captured graph returns on NEW data against the eager value -- the ATen reduction it replaces returned a stale sum
    from the second replay of the train-step graph on (tools/debug_graph_e8.py)."""
    import torch.nn.functional as F
    from cleanumamba_amd.network.convstack import LpLoss
    g = torch.Generator().manual_seed(sum(shape) + p)
    y = torch.randn(*shape, generator=g).to(cuda).requires_grad_(True)
    c = torch.randn(*shape, generator=g).to(cuda)
    if y.numel() > 10:
        with torch.no_grad():
            y[0, 0, 3] = c[0, 0, 3]                               # an exact tie: gradient 0, as torch.sgn
    loss = LpLoss.apply(y, c, p)
    (loss * 3.0).backward()
    yd = y.detach().double().requires_grad_(True)
    want = (F.l1_loss if p == 1 else F.mse_loss)(yd, c.double())
    (want * 3.0).backward()
    assert abs(float(loss) - float(want)) < 2e-6 * abs(float(want)) + 1e-12
    assert rel_l2(y.grad, yd.grad) < 1e-6
    two = LpLoss.apply(y.detach(), c, p)
    assert torch.equal(two, loss.detach())                         # fixed summation order: bit-reproducible
    ys, cs_ = y.detach().clone(), c.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = LpLoss.apply(ys, cs_, p)
    for it in range(3):
        ys.copy_(torch.randn(*shape, generator=g).to(cuda))
        cs_.copy_(torch.randn(*shape, generator=g).to(cuda))
        graph.replay()
        assert torch.equal(out, LpLoss.apply(ys, cs_, p)), it


@pytest.mark.parametrize("shape", [(1, 2), (3, 777), (16, 160000), (2, 480000)])
def test_clip_std_and_framing(cuda, shape):
    """cum_clip_std against torch.std (f64) -- `noisy_audio.std(dim=2, keepdim=True) + 1e-3`, src/network/CleanUMamba.py:
    260-262 -- on signals with a large offset (one-pass Welford must not cancel); cum_frame_rows / cum_unframe_rows
    against the torch construction of the row buffer."""
    from cleanumamba_amd.network import convstack as cs
    B, L = shape
    g = torch.Generator().manual_seed(L)
    x = (0.05 * torch.randn(B, 1, L, generator=g) + torch.linspace(-3, 3, B).view(B, 1, 1)).to(cuda)
    std = cs.clip_std(x, 1e-3)
    want = x.double().std(dim=2, keepdim=True) + 1e-3
    assert std.shape == (B, 1, 1) and rel_l2(std, want) < 2e-6
    assert torch.equal(std, cs.clip_std(x, 1e-3))
    T = L + 5
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        geo = cs.Geo(B, T, 1)
        buf = cs.frame_input(x, std, T, dt)
        ref = cs.to_rows(torch.nn.functional.pad(x / std, (0, T - L)), geo, dt)
        assert buf.shape == ref.shape and torch.equal(buf, ref)
        y = cs.Unframe.apply(buf.clone().requires_grad_(True), std, geo, L)
        assert torch.equal(y, cs.from_rows(ref, geo).float()[:, :, :L] * std)
        leaf = buf.clone().float().requires_grad_(True)
        dy = torch.randn(B, 1, L, generator=g).to(cuda)
        (cs.Unframe.apply(leaf.to(dt), std, geo, L) * dy).sum().backward()
        wleaf = ref.clone().float().requires_grad_(True)
        ((cs.from_rows(wleaf.to(dt), geo).float()[:, :, :L] * std) * dy).sum().backward()
        assert rel_l2(leaf.grad, wleaf.grad) < (1e-6 if dt == torch.float32 else 4e-3)


# ---- streaming glue (csrc/stream.hip): pure data movement and single IEEE additions, so every assertion is torch.equal
def _window_case(cuda, dt, S, rows, n_new, Cp, tail, compact):
    from cleanumamba_amd import hip
    pitch = rows + 3
    g = torch.Generator().manual_seed(rows * 31 + n_new)
    window = torch.randn(S, pitch, Cp, generator=g).to(dt).to(cuda)
    full = torch.randn(S, pitch, Cp, generator=g).to(dt).to(cuda)
    want = torch.cat([window[:, n_new:rows], full[:, rows - n_new:rows]], 1)
    w = window.clone()
    fresh = full[:, rows - n_new:rows].contiguous() if compact else full
    fresh0 = fresh.clone()
    tmp = torch.empty(S * rows * Cp, dtype=dt, device=cuda)
    nxt = torch.full((S, n_new + 4, Cp), 7.0, dtype=dt, device=cuda) if tail else None
    with torch.cuda.device(cuda):
        hip.check(hip.lib().cum_stream_window_update(hip.dtype_code(dt), S, rows, n_new, Cp, hip.ptr(w), hip.ptr(fresh), pitch,
                                                     n_new if compact else pitch, rows - n_new if compact else 0,
                                                     hip.ptr(tmp), hip.ptr(nxt), n_new + 4, hip.stream_ptr()))
    assert torch.equal(w[:, :rows], want)
    assert torch.equal(w[:, rows:], window[:, rows:])           # the rows of the pitch behind the window are untouched
    assert torch.equal(fresh, fresh0)
    if tail:          # the n_new + 2 newest rows, and the sentinel rows behind them
        assert torch.equal(nxt[:, :n_new + 2], want[:, rows - n_new - 2:])
        assert bool((nxt[:, n_new + 2:] == 7.0).all())


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("dt,S,rows,n_new,Cp,tail", [
    (torch.float32, 5, 300, 4, 128, True),      # keep = 296: six chunks of 6 vectors, the last holds two
    (torch.float32, 5, 22, 22, 24, False),      # n_new == rows: nothing is kept
    (torch.bfloat16, 5, 22, 22, 24, False),
    (torch.float32, 5, 10, 8, 24, True),        # keep == 2: the carried rows of tail_dst are all that is kept
    (torch.float16, 5, 10, 8, 24, True),
    (torch.bfloat16, 3, 2052, 4, 8, True),      # keep = 2048: the most the in-place kernel holds (8 vectors a thread)
    (torch.float16, 3, 2053, 4, 8, False),      # keep = 2049: the two-launch path through tmp
    (torch.bfloat16, 5, 22, 8, 20, False),      # 40-byte rows: the two-launch path through alignment
    (torch.float32, 5, 22, 8, 6, False),        # 24-byte rows
])
def test_stream_window_update_paths(cuda, dt, S, rows, n_new, Cp, tail, compact):
    """cum_stream_window_update against slicing on every path: the in-place kernel with several channel chunks and a
    ragged last one, with nothing kept, with exactly the two carried rows, at its register limit; the shift + store pair
    beyond that limit and on rows that are not 16-byte multiples."""
    _window_case(cuda, dt, S, rows, n_new, Cp, tail, compact)


def _overlap_add(cuda, dt, y, tail, bias, skip, S, L2, Cp, C, relu):
    """One hop through cum_stream_overlap_add; -> (out buffer with two sentinel rows per stream, the tail it left) and
    the same from the formula in the header of csrc/stream.hip, in f32 from the stored values, rounded once."""
    from cleanumamba_amd import hip
    out = torch.full((S, L2 + 2, Cp), 7.0, dtype=dt, device=cuda)
    t_new = tail.clone()
    with torch.cuda.device(cuda):
        hip.check(hip.lib().cum_stream_overlap_add(hip.dtype_code(dt), S, L2, Cp, C, hip.ptr(y), y.shape[1], hip.ptr(t_new),
                                                   hip.ptr(bias), hip.ptr(skip), 0 if skip is None else skip.shape[1],
                                                   hip.ptr(out), L2 + 2, relu, hip.stream_ptr()))
    o = y[:, :L2].float().clone()
    o[:, :2] += tail.float()
    if relu:
        o = o.clamp_min(0)
    if skip is not None:
        o = o + skip[:, :L2].float()
    live = (torch.arange(Cp, device=cuda) < C).view(1, 1, Cp)
    zero = torch.zeros((), device=cuda)
    want = torch.where(live, o, zero).to(dt)
    b = torch.zeros(Cp, device=cuda)
    if bias is not None:
        b[:C] = bias[:C]
    want_tail = torch.where(live, y[:, L2:L2 + 2].float() - b, zero).to(dt)
    return out, t_new, want, want_tail


@pytest.mark.parametrize("L2", [2, 4, 256])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16])
def test_stream_overlap_add(cuda, dt, relu, L2):
    """out = act(y + old tail on the first two rows) + skip, tail = the frame's last two rows minus the bias, with C < Cp
    (pad channels of out and tail are exact zeros whatever y, skip and the old tail hold there), pitches larger than
    needed (sentinel rows stay) and skip / bias present or null."""
    S, Cp, C = 3, 24, 20
    g = torch.Generator().manual_seed(L2 + relu)
    rn = lambda *s: torch.randn(*s, generator=g)
    y = rn(S, L2 + 5, Cp).to(dt).to(cuda)
    skip_t = rn(S, L2 + 1, Cp).to(dt).to(cuda)
    bias_t = rn(Cp).to(cuda)
    tail = rn(S, 2, Cp).to(dt).to(cuda)
    y0, tail0, skip0 = y.clone(), tail.clone(), skip_t.clone()
    for skip in (skip_t, None):
        for bias in (bias_t, None):
            out, t_new, want, want_tail = _overlap_add(cuda, dt, y, tail, bias, skip, S, L2, Cp, C, relu)
            assert torch.equal(out[:, :L2], want) and torch.equal(t_new, want_tail)
            assert bool((out[:, L2:] == 7.0).all())
            assert float(out[:, :L2, C:].abs().max()) == 0.0 and float(t_new[:, :, C:].abs().max()) == 0.0
            assert torch.equal(y, y0) and torch.equal(tail, tail0) and torch.equal(skip_t, skip0)


def test_stream_overlap_add_two_hops_and_the_grid_stride_pass(cuda):
    """Two consecutive hops: the tail the first writes is what the second adds to its first two rows.  37 streams of
    L2 = 256 at Cp = 128 are 1 221 888 elements, more than 4096 workgroups of 256 threads: the second pass of the
    grid-stride loop."""
    for dt, S, L2, Cp, C in ((torch.bfloat16, 3, 4, 24, 20), (torch.float32, 37, 256, 128, 128), (torch.float16, 37, 256, 128, 100)):
        g = torch.Generator().manual_seed(S)
        rn = lambda *s: torch.randn(*s, generator=g)
        bias = rn(Cp).to(cuda)
        tail = torch.zeros(S, 2, Cp, dtype=dt, device=cuda)
        for hop in range(2):
            y, skip = rn(S, L2 + 2, Cp).to(dt).to(cuda), rn(S, L2, Cp).to(dt).to(cuda)
            out, t_new, want, want_tail = _overlap_add(cuda, dt, y, tail, bias, skip, S, L2, Cp, C, 1)
            assert torch.equal(out[:, :L2], want) and torch.equal(t_new, want_tail), (dt, hop)
            if hop == 1:      # the first hop's tail was consumed: without it the first two rows differ
                assert not torch.equal(_overlap_add(cuda, dt, y, torch.zeros_like(tail), bias, skip, S, L2, Cp, C, 1)[0][:, :2],
                                       out[:, :2])
            tail = t_new
