"""Block denoising with carried Mamba state (network/blockdenoise.py: model.denoise_long, model.block_denoiser) against
``forward`` on the whole signal (GPU).  Bound: E2E_TOL, the project's 1e-4 (also the bound for stream == forward)."""
import pytest
import torch

from conftest import golden_json, load_ckpt, load_golden, record, rel_l2
from oracle import synth

pytestmark = pytest.mark.gpu
T = torch.from_numpy
E2E_TOL = 1e-4
_cache = {}


def _net(name, cuda, pruned=False):
    from cleanumamba_amd.network import CleanUMamba
    if name not in _cache:
        sd, cfg = load_ckpt(name)
        net = CleanUMamba(**cfg)
        if pruned:
            net.load_pruned_state_dict(sd)
        else:
            net.load_state_dict(sd, strict=True)
        _cache[name] = net.to(cuda).float().eval()
    net = _cache[name]
    net.normalize_input = True
    return net


def _whole(name, cuda, pruned):
    """forward on the golden input, once per checkpoint: (input, normalised output, raw padded output)."""
    key = "whole_" + name
    if key not in _cache:
        net = _net(name, cuda, pruned)
        x = T(load_golden("e2e_" + name)["input"]).to(cuda)
        with torch.no_grad():
            y = net(x)
            net.normalize_input = False
            yraw = net(x)
            net.normalize_input = True
        _cache[key] = (x, y, yraw)
    return _cache[key]


@pytest.mark.parametrize("block_hops", [2, 7, 16, 61])
@pytest.mark.parametrize("name,pruned", [("442k", False), ("pruned500k", True)])
def test_denoise_long_equals_forward_on_checkpoints(cuda, name, pruned, block_hops):
    from cleanumamba_amd.network.blockdenoise import block_schedule
    net = _net(name, cuda, pruned)
    x, y, yraw = _whole(name, cuda, pruned)
    g = load_golden("e2e_" + name)
    out = net.denoise_long(x, block_hops=block_hops)
    assert out.shape == y.shape == (2, 1, 16000)
    assert record(f"block_vs_forward_{name}_{block_hops}", rel_l2(out, y)) < E2E_TOL
    assert rel_l2(out, g["out_norm"]) < E2E_TOL
    # per seam: a click at a block edge must not be averaged away
    hop, F = net.total_stride, net.frame_length
    sched = block_schedule(16000, block_hops, F, hop)
    assert sum(w.tau1 - w.tau0 for w in sched) == 61
    whole_rms = y.double().square().mean().sqrt().item()
    for w in sched[1:]:
        s = w.emit_lo
        d = (out[..., s - 512:s + 512].double() - y[..., s - 512:s + 512].double()).square().mean().sqrt().item()
        assert d <= 1e-4 * whole_rms, (s, d, whole_rms)
    # without input normalisation: the padded length, as forward returns it
    net.normalize_input = False
    try:
        raw = net.denoise_long(x, block_hops=block_hops)
    finally:
        net.normalize_input = True
    assert raw.shape == yraw.shape == (2, 1, 16126)
    assert rel_l2(raw, yraw) < E2E_TOL


def _synth_net(name, cuda):
    from cleanumamba_amd.network import CleanUMamba
    if name not in _cache:
        g = load_golden("e2e_" + name)
        meta = golden_json(g["meta"])
        net = CleanUMamba(**meta["cfg"])
        sd = synth.fill_state_dict(dict(zip(meta["keys"], meta["shapes"])), seed=meta["seed"])
        net.load_state_dict(sd, strict=True)
        _, noisy = synth.waveform(2, meta["L"], seed=meta["wave_seed"])
        _cache[name] = (net.to(cuda).eval(), noisy.to(cuda))
    return _cache[name]


@pytest.mark.parametrize("name", ["e8_synth", "e6_synth"])
def test_denoise_long_full_width_f32_and_autocast(cuda, name):
    """d_state 64, 768 channels.  f32: the block route equals forward.  Under autocast both routes are the same
    arithmetic with different tiling: the block route may be at most 1.25x as far from the f32 forward as the whole-signal
    route under the same autocast (the margin absorbs summation order)."""
    net, noisy = _synth_net(name, cuda)
    with torch.no_grad():
        y32 = net(noisy)
        out = net.denoise_long(noisy, block_hops=8)
        assert out.shape == y32.shape
        assert record(f"block_vs_forward_{name}", rel_l2(out, y32)) < E2E_TOL
        for dt in (torch.float16, torch.bfloat16):
            with torch.autocast("cuda", dtype=dt):
                yw = net(noisy)
                yb = net.denoise_long(noisy, block_hops=8)
            dw = record(f"autocast_whole_{name}_{dt}", rel_l2(yw.float(), y32))
            db = record(f"autocast_block_{name}_{dt}", rel_l2(yb.float(), y32))
            print(name, dt, "whole", dw, "block", db)
            assert db <= 1.25 * dw, (dt, db, dw)


@pytest.mark.parametrize("block_hops", [2, 3])
@pytest.mark.parametrize("L", [1, 300, 767, 4099])
def test_denoise_long_ragged_lengths(cuda, L, block_hops):
    net = _net("442k", cuda)
    x = (0.1 * torch.randn(3, 1, L, generator=torch.Generator().manual_seed(L))).to(cuda)
    if L == 1:
        net.normalize_input = False            # std of a single sample is undefined
    try:
        with torch.no_grad():
            y = net(x)
        out = net.denoise_long(x, block_hops=block_hops)
    finally:
        net.normalize_input = True
    assert out.shape == y.shape
    assert rel_l2(out, y) < E2E_TOL


def test_push_cuts_do_not_change_the_bits_and_host_in_gives_host_out(cuda):
    from cleanumamba_amd.network import convstack as cs
    net = _net("442k", cuda)
    x, y, _ = _whole("442k", cuda, False)
    x2 = x[:, 0]
    std = cs.clip_std(x, 1e-3).view(2, 1)
    one = net.block_denoiser(2, std=std, block_hops=7)
    a = torch.cat([one.push(x2), one.finish()], 1)
    assert a.shape == (2, 16000) and rel_l2(a, y[:, 0]) < E2E_TOL
    cut = net.block_denoiser(2, std=std, block_hops=7)
    outs, pos, sizes, i = [], 0, (1000, 37, 5000, 1, 2999), 0
    while pos < 16000:
        n = sizes[i % len(sizes)]
        outs.append(cut.push(x2[:, pos:pos + n]))
        pos, i = pos + n, i + 1
    outs.append(cut.finish())
    assert torch.equal(torch.cat(outs, 1), a)
    # host tensor in, host tensor out, the device route's bits
    h = net.denoise_long(x.cpu(), block_hops=7)
    d = net.denoise_long(x, block_hops=7)
    assert not h.is_cuda and d.is_cuda
    assert rel_l2(h, d) < 1e-6                 # the host std pass sums in f64: the std may differ in its last bit
    assert rel_l2(h, y) < E2E_TOL
    hs = net.block_denoiser(2, std=std, block_hops=7)
    hp = torch.cat([hs.push(x2.cpu()), hs.finish(device="cpu")], 1)
    assert not hp.is_cuda and torch.equal(hp, a.cpu())


def test_host_std_pass_agrees_with_clip_std(cuda):
    from cleanumamba_amd.network import convstack as cs
    from cleanumamba_amd.network.blockdenoise import host_clip_std
    x = 0.1 * torch.randn(3, 50001, generator=torch.Generator().manual_seed(3)) + 0.05
    want = cs.clip_std(x.to(cuda).unsqueeze(1), 1e-3).cpu()
    got = host_clip_std(x, 1e-3, piece=7001)
    assert got.shape == want.shape == (3, 1, 1)
    assert ((got - want).abs() / want).max().item() < 1e-6


def test_denoise_long_leaves_a_running_feed_stream_alone(cuda):
    net = _net("442k", cuda)
    x = T(load_golden("e2e_442k")["input"]).to(cuda)
    a, other = x[0], x[1:2]                    # (1, 16000) each
    with torch.no_grad():
        net.reset_stream()
        want = torch.cat([net.feed(a[:, :3000]), net.feed(a[:, 3000:]), net.flush()], 1)
        net.reset_stream()
        head = net.feed(a[:, :3000])
        net.denoise_long(other, block_hops=7)
        got = torch.cat([head, net.feed(a[:, 3000:]), net.flush()], 1)
    assert torch.equal(got, want)


def test_device_memory_does_not_grow_with_length(cuda):
    """442k, 16 columns per block, host-resident input and output: 40 blocks may take at most one block's input + output
    buffers more than 4 blocks -- the shapes allocated per block are identical, so allocated bytes cannot grow."""
    net = _net("442k", cuda)
    hop, bh = net.total_stride, 16
    gen = torch.Generator().manual_seed(5)
    peaks = {}
    net.denoise_long(0.1 * torch.randn(1, 4 * bh * hop, generator=gen), block_hops=bh)        # warm-up
    for blocks in (4, 40):
        x = 0.1 * torch.randn(1, blocks * bh * hop, generator=gen)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = net.denoise_long(x, block_hops=bh)
        torch.cuda.synchronize()
        peaks[blocks] = torch.cuda.max_memory_allocated() - base
        assert not out.is_cuda and out.shape == (1, 1, x.shape[1])
    record("block_denoise_peak_bytes_4", peaks[4])
    record("block_denoise_peak_bytes_40", peaks[40])
    assert peaks[40] <= peaks[4] + 2 * bh * hop * 4, peaks


def test_declined_models_and_block_sizes(cuda):
    from cleanumamba_amd.network import CleanUMamba
    _, cfg = load_ckpt("mamba2")
    m2 = CleanUMamba(**cfg).to(cuda).eval()
    with pytest.raises(NotImplementedError, match="Mamba2"):
        m2.denoise_long(torch.zeros(1, 4000, device=cuda))
    with pytest.raises(NotImplementedError, match="Mamba2"):
        m2.block_denoiser(1)
    net = _net("442k", cuda)
    with pytest.raises(ValueError):
        net.denoise_long(torch.zeros(1, 4000, device=cuda), block_hops=1)
    with pytest.raises(ValueError):
        net.block_denoiser(1, std=torch.ones(1, 1), block_hops=1)
    with pytest.raises(ValueError):
        net.denoise_long(torch.zeros(1, 4000, device=cuda), block_size=net.total_stride)
