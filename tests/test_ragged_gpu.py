"""Ragged inference batches on the GPU (csrc/ragged.hip, the ragged entries of csrc/dech.hip / csrc/dec7.hip,
network/ragged.py): every kernel against its per-clip counterpart, and ``denoise_batch`` / ``forward_ragged`` against the
f64-capable oracle run on every clip ALONE -- on the whole clip and on its tail window, where a missing row mask shows
(DESIGN.md 7f).  Reference call sites: src/network/CleanUMamba.py:260-264, 319 (std, padding, crop), :121-130 (decoder),
src/examples/denoise.py:42-60 (one file per forward)."""
import pytest
import torch

import mamba2_ref as M2
from conftest import load_ckpt, record, rel_l2
from oracle import cleanumamba_ref as R
from oracle import synth

pytestmark = pytest.mark.gpu
E2E_TOL = 1e-4
LENGTHS = [300, 766, 767, 1500, 2047, 1022, 1023, 2]     # the seven-clip batch of the issue + a 2-sample clip
_cache = {}


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _pcm_rows(lengths, pitch, seed, cuda):
    """(B, pitch) int16 rows with a large offset per clip (one-pass Welford must not cancel) + the f32 rows of the same
    samples; what lies behind a clip's length is junk the kernels must not read into a result."""
    g = torch.Generator().manual_seed(seed)
    B = len(lengths)
    x = (1500 * torch.randn(B, pitch, generator=g) + torch.linspace(-20000, 20000, B).view(B, 1)).clamp(-32768, 32767)
    x = x.to(torch.int16)
    return x.to(cuda), (x.float() / 32768.0).to(cuda)


@pytest.mark.parametrize("src", ["int16", "f32"])
def test_clip_std_ragged_against_f64_and_batch_independent(cuda, src):
    from cleanumamba_amd.network import ragged as rg
    Lmax = 1000
    lengths = [2, 7, 8, 9, 255, 257, Lmax]
    xi, xf = _pcm_rows(lengths, 1000, 11, cuda)
    x = xi if src == "int16" else xf
    lens = torch.tensor(lengths, dtype=torch.int32, device=cuda)
    std = rg.clip_std_ragged(x, lens, 1e-3)
    want = torch.stack([xf[b, :n].double().std() + 1e-3 for b, n in enumerate(lengths)])
    assert std.shape == (7,) and record(f"clip_std_ragged[{src}]", rel_l2(std, want)) < 2e-6
    assert torch.equal(std, rg.clip_std_ragged(x, lens, 1e-3))
    # the same clips in another batch: other mates, other order, a longer batch, rows OFF the 16-byte boundary (pitch 2059
    # elements: the element loads instead of the 16-byte ones) -- the same bits
    order = [6, 0, 5, 3]
    y = torch.full((5, 2059), 77, dtype=x.dtype, device=cuda)
    for r, b in enumerate(order):
        y[r, :lengths[b]] = x[b, :lengths[b]]
    y[4, :2059] = x[6, :1].expand(2059)
    lens2 = torch.tensor([lengths[b] for b in order] + [2059], dtype=torch.int32, device=cuda)
    std2 = rg.clip_std_ragged(y, lens2, 1e-3)
    assert torch.equal(_bits(std2[:4]), _bits(std[order]))


@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
@pytest.mark.parametrize("src", ["int16", "f32"])
def test_frame_rows_ragged_is_frame_input_of_every_clip_alone(cuda, dt, src):
    from cleanumamba_amd.network import convstack as cs
    from cleanumamba_amd.network import ragged as rg
    lengths = [2, 7, 8, 9, 255, 257, 1000]
    T = 1022
    for pitch in (1000, 1003):                             # 16-byte rows and rows off the boundary
        xi, xf = _pcm_rows(lengths, pitch, 5, cuda)
        x = (xi if src == "int16" else xf)[:, :1000]
        lens = torch.tensor(lengths, dtype=torch.int32, device=cuda)
        std = rg.clip_std_ragged(x, lens, 1e-3)
        geo = cs.Geo(7, T, 1)
        buf = rg.frame_input_ragged(x, lens, std, T, dt)
        assert buf.shape == (geo.R, 8) and buf.dtype == dt
        rows = geo.rows(buf)
        for b, n in enumerate(lengths):
            lone = cs.frame_input(xf[b:b + 1, None, :n].contiguous(), std[b:b + 1].view(1, 1, 1), T, dt)
            assert torch.equal(_bits(rows[b]), _bits(cs.Geo(1, T, 1).rows(lone)[0])), (b, n)
            assert float(rows[b, n:].float().abs().max()) == 0.0
        assert float(buf[0].float().abs().max()) == 0.0 and float(buf[1 + geo.M:].float().abs().max()) == 0.0
        assert float(buf[:, 1:].float().abs().max()) == 0.0
        # scale = NULL: the samples themselves
        raw = geo.rows(rg.frame_input_ragged(x, lens, None, T, dt))
        for b, n in enumerate(lengths):
            assert torch.equal(raw[b, :n, 0], xf[b, :n].to(dt)) and float(raw[b, n:].float().abs().max()) == 0.0


@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("C", [1, 35, 64])
def test_rows_zero_tail_touches_only_the_tail(cuda, dt, C):
    from cleanumamba_amd.network import convstack as cs
    for B, T, valid in ((4, 37, [0, 17, 37, 36]), (3, 1300, [1, 1299, 640])):
        geo = cs.Geo(B, T, C)
        g = torch.Generator(device=cuda).manual_seed(C)
        buf = torch.randn(geo.R, geo.Cp, generator=g, device=cuda).to(dt)
        before = buf.clone()
        cs.rows_zero_tail(buf, geo, torch.tensor(valid, dtype=torch.int32, device=cuda))
        rows, rows0 = geo.rows(buf), geo.rows(before)
        for b, v in enumerate(valid):
            assert float(rows[b, v:T].float().abs().max()) == 0.0 if v < T else True
            assert torch.equal(_bits(rows[b, :v]), _bits(rows0[b, :v]))
            assert torch.equal(_bits(rows[b, T:]), _bits(rows0[b, T:]))          # the clip's two closing rows
        assert torch.equal(_bits(buf[0]), _bits(before[0])) and torch.equal(_bits(buf[1 + geo.M:]), _bits(before[1 + geo.M:]))


@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
def test_unframe_rows_ragged_is_unframe_of_every_clip(cuda, dt):
    from cleanumamba_amd.network import convstack as cs
    from cleanumamba_amd.network import ragged as rg
    lengths = [2, 7, 8, 9, 255, 257, 1001]
    for Lmax, T in ((1001, 1022), (1004, 1022)):           # output rows off / on the 16-byte boundary
        geo = cs.Geo(7, T, 1)
        g = torch.Generator(device=cuda).manual_seed(Lmax)
        buf = torch.randn(geo.R, 8, generator=g, device=cuda).to(dt)        # junk everywhere: nothing behind a length may leave
        std = torch.rand(7, generator=g, device=cuda) + 0.5
        lens = torch.tensor(lengths, dtype=torch.int32, device=cuda)
        y = rg.unframe_ragged(buf, geo, lens, std, Lmax)
        assert y.shape == (7, 1, Lmax) and y.dtype == torch.float32
        for b, n in enumerate(lengths):
            one = buf[b * geo.P:1 + (b + 1) * geo.P + geo.slack].clone()     # clip b as a batch of one (row 0 = any row)
            want = cs.Unframe.apply(one, std[b:b + 1], cs.Geo(1, T, 1), n)
            assert torch.equal(_bits(y[b, 0, :n]), _bits(want[0, 0])), (b, n)
            assert float(y[b, 0, n:].abs().max()) == 0.0 if n < Lmax else True
        raw = rg.unframe_ragged(buf, geo, lens, None, Lmax)
        assert torch.equal(raw[6, 0, :1001], geo.rows(buf)[6, :1001, 0].float())


# ------------------------------------------------------------------------------------------------ whole model, f32
def _net(name, cuda):
    from cleanumamba_amd.network import CleanUMamba
    if name not in _cache:
        sd, cfg = load_ckpt(name)
        net = CleanUMamba(**cfg)
        net.load_pruned_state_dict(sd) if "pruned" in name else net.load_state_dict(sd, strict=True)
        _cache[name] = (net.to(cuda).float().eval(), {k: v.double() for k, v in sd.items()}, cfg)
    return _cache[name]


def _clips(lengths, seed=7):
    g = torch.Generator().manual_seed(seed)
    return [0.1 * torch.randn(n, generator=g) + 0.02 for n in lengths]


def _alone(sd, cfg, clip, monkeypatch):
    """The oracle on one clip alone, in f64 (the Mamba2 checkpoint: its mixer from tests/mamba2_ref.py)."""
    if cfg.get("mamba_v2"):
        hd = cfg["tsfm_d_model"] // cfg["tsfm_n_head"]
        monkeypatch.setattr(R, "mamba_mixer", lambda s, p, h, eps_unused=None: M2.mixer_ref(s, p, h, hd))
    with torch.no_grad():
        return R.forward_ref(sd, clip.double().view(1, 1, -1))[0, 0]


def _tail(hop, E, n):
    from cleanumamba_amd.network.ragged import level_rows
    return hop * (level_rows(n, E)[E] - 1)


@pytest.mark.parametrize("name", ["442k", "pruned500k", "mamba2"])
def test_denoise_batch_equals_every_clip_alone(cuda, name, monkeypatch):
    net, sd, cfg = _net(name, cuda)
    E, hop = net.encoder_n_layers, net.total_stride
    clips = _clips(LENGTHS)
    with torch.no_grad():
        outs = net.denoise_batch([c.to(cuda) for c in clips], max_waste=1.0)        # one batch of eight
        assert all(r.endswith("zero_tail") for r in net.ragged_dispatch) and len(net.ragged_dispatch) == E
        planned = net.denoise_batch(clips)                                           # host clips, the planner's batches
        padded = torch.nn.utils.rnn.pad_sequence(clips, batch_first=True).to(cuda)
        y = net.forward_ragged(padded, LENGTHS)
        # lengths as a device i32 tensor, the batch as (B, 1, Lmax): the same bits
        assert torch.equal(y, net.forward_ragged(padded.unsqueeze(1), torch.tensor(LENGTHS, dtype=torch.int32, device=cuda)))
    assert y.shape == (8, 1, 2047)
    for b, (n, c) in enumerate(zip(LENGTHS, clips)):
        ref = _alone(sd, cfg, c, monkeypatch)
        t0 = _tail(hop, E, n)
        for tag, got in (("batch", outs[b]), ("planned", planned[b]), ("forward_ragged", y[b, 0, :n])):
            assert got.shape == (n,) and got.dtype == torch.float32 and got.is_cuda
            whole, tail = rel_l2(got, ref), rel_l2(got[t0:], ref[t0:])
            record(f"ragged_{name}_{tag}[{n}]", whole)
            record(f"ragged_{name}_{tag}_tail[{n}]", tail)
            print(name, tag, n, "whole", whole, "tail", tail)
            assert whole < E2E_TOL and tail < E2E_TOL, (name, tag, n, whole, tail)
        assert float(y[b, 0, n:].abs().max()) == 0.0 if n < 2047 else True           # the padding is zero
    with pytest.raises(RuntimeError, match="no_grad"):
        net.forward_ragged(torch.zeros(1, 100, device=cuda), [100])


def test_int16_clips_and_no_normalisation(cuda):
    """int16 PCM in equals the float clips in; without normalize_input the ragged result is the first len samples of the
    lone forward's padded output."""
    net, _, _ = _net("442k", cuda)
    g = torch.Generator().manual_seed(1)
    pcm = [(3000 * torch.randn(n, generator=g)).clamp(-32768, 32767).to(torch.int16) for n in (1, 300, 767, 1500)]
    flt = [p.float() / 32768.0 for p in pcm]
    net.normalize_input = False
    try:
        with torch.no_grad():
            a = net.denoise_batch(pcm, max_waste=1.0)
            b = net.denoise_batch([f.to(cuda) for f in flt], max_waste=1.0)
            for n, x, ya, yb in zip((1, 300, 767, 1500), flt, a, b):
                lone = net(x.to(cuda).view(1, 1, -1))
                assert lone.shape[-1] == net.valid_length(n) and ya.shape == (n,)
                assert torch.equal(ya, yb)
                assert rel_l2(ya, lone[0, 0, :n]) < E2E_TOL
    finally:
        net.normalize_input = True


# ------------------------------------------------------------------------------------------------ fused decoder routes
SMALL = dict(channels_input=1, channels_output=1, channels_H=64, max_H=128, encoder_n_layers=3, kernel_size=4, stride=2,
             tsfm_n_layers=1, tsfm_n_head=8, tsfm_d_model=64, tsfm_d_inner=128)
SMALL_LENGTHS = [37, 100, 263, 515, 1000, 64, 777]


def test_fused_decoder_routes_under_f16_autocast(cuda):
    """channels_H = 64: the last two decoder layers dispatch to cum_dec7_fwd_ragged / cum_dech_fwd_ragged, the first to
    the GEMM + cum_rows_zero_tail.  Ragged and lone round the same arithmetic; only tile-dependent order differs, so
    against the f64 oracle the ragged error may exceed the lone error by at most a quarter -- whole clip and tail window.
    Measured (MI355X, f16): see DESIGN.md 7f."""
    from cleanumamba_amd.network import CleanUMamba
    net = CleanUMamba(**SMALL)
    sd = synth.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=3)
    net.load_state_dict(sd, strict=True)
    net = net.to(cuda).eval()
    sd64 = {k: v.double() for k, v in sd.items()}
    E, hop = 3, net.total_stride
    clips = _clips(SMALL_LENGTHS, seed=9)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        outs = net.denoise_batch([c.to(cuda) for c in clips], max_waste=1.0)
        assert net.ragged_dispatch == ["gemm+zero_tail", "dech_ragged", "dec7_ragged"], net.ragged_dispatch
        lone = [net(c.to(cuda).view(1, 1, -1))[0, 0] for c in clips]
    worst = 0.0
    for n, c, got, alone in zip(SMALL_LENGTHS, clips, outs, lone):
        with torch.no_grad():
            ref = R.forward_ref(sd64, c.double().view(1, 1, -1))[0, 0]
        t0 = _tail(hop, E, n)
        for tag, sl in (("whole", slice(0, n)), ("tail", slice(t0, n))):
            er, el = rel_l2(got[sl], ref[sl]), rel_l2(alone[sl], ref[sl])
            record(f"ragged_f16_{tag}[{n}]", er)
            record(f"lone_f16_{tag}[{n}]", el)
            print(n, tag, "ragged", er, "lone", el)
            worst = max(worst, er / el)
            assert er <= 1.25 * el, (n, tag, er, el)
    record("ragged_f16_worst_ratio", worst)
