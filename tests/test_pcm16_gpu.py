"""The PCM16 quantising kernels (csrc/ragged.hip: cum_unframe_rows_ragged_pcm16, cum_pcm16_from_f32_ragged) against the
numpy statement of the two rules (tests/pcm16_ref.py), bit for bit, and ``denoise_batch_pcm16`` against the same rules
applied by torch to ``denoise_batch``'s f32 output: the same plan and the same forwards, only the last kernel differs."""
import ctypes

import numpy as np
import pytest
import torch

import pcm16_ref as P
from conftest import load_ckpt

pytestmark = pytest.mark.gpu
LENS = [1, 7, 8, 9, 4099]
LMAX, T = 4099, 4104
FILL = 0x5A5A
SCALES = [1.0, 0.37, 1.5, 2.0, 0.9993]


def _layouts():
    """(name, offsets, total): packed back to back (clips start at samples 1, 8, 16, 25: odd and whole positions), and with
    3 guard samples in front of, between and behind the clips (3, 7, 17, 28, 40: none on a 16-byte boundary)."""
    packed = np.cumsum(LENS) - LENS
    guarded = packed + 3 * (1 + np.arange(len(LENS)))
    return [("packed", packed.astype(np.int64), int(sum(LENS))), ("guarded", guarded.astype(np.int64), int(sum(LENS)) + 18)]


def _values(rng, n, b):
    """n f32 samples of clip b: the case table at the start, in the middle and at the end (cut where the clip is
    shorter), uniform values a little past full scale elsewhere."""
    table = np.roll(P.case_table(), -7 * b)
    v = rng.uniform(-1.1, 1.1, n).astype(np.float32)
    for at in (0, max(0, n // 2 - table.size // 2), max(0, n - table.size)):
        m = min(table.size, n - at)
        v[at:at + m] = table[:m]
    return v


def _check_flat(flat, offsets, total, want, tag):
    got = flat.cpu().numpy()
    keep = np.ones(total, bool)
    for b, (o, w) in enumerate(zip(offsets, want)):
        assert np.array_equal(got[o:o + w.size], w), (tag, b, np.flatnonzero(got[o:o + w.size] != w)[:5])
        keep[o:o + w.size] = False
    assert np.all(got[keep] == FILL), (tag, "a sample outside the clips was written")


@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.bfloat16])
def test_unframe_pcm16_is_the_rule_bit_for_bit(cuda, dt):
    from cleanumamba_amd.network import convstack as cs
    from cleanumamba_amd.network import ragged as rg
    rng = np.random.default_rng(5)
    geo = cs.Geo(len(LENS), T, 1)
    buf = torch.from_numpy(rng.uniform(-1.1, 1.1, (geo.R, 8)).astype(np.float32))     # junk everywhere else
    rows = geo.rows(buf)
    for b, n in enumerate(LENS):
        rows[b, :n, 0] = torch.from_numpy(_values(rng, n, b))
    buf = buf.to(dt).to(cuda)
    elem = [geo.rows(buf)[b, :n, 0].float().cpu().numpy() for b, n in enumerate(LENS)]   # the element converted to f32
    lens = torch.tensor(LENS, dtype=torch.int32, device=cuda)
    scale = torch.tensor(SCALES, dtype=torch.float32, device=cuda)
    for name, offsets, total in _layouts():
        offs = torch.from_numpy(offsets).to(cuda)
        for mode in (0, 1):
            for sc in (None, scale):
                want = [P.quantise(e * np.float32(SCALES[b]) if sc is not None else e, mode) for b, e in enumerate(elem)]
                flat = torch.full((total,), FILL, dtype=torch.int16, device=cuda)
                rg.unframe_ragged_pcm16(buf, geo, lens, sc, LMAX, flat, offs, mode)
                _check_flat(flat, offsets, total, want, (name, mode, sc is not None))
                again = torch.full((total,), FILL, dtype=torch.int16, device=cuda)
                rg.unframe_ragged_pcm16(buf, geo, lens, sc, LMAX, again, offs, mode)
                assert torch.equal(flat, again)
    # a length past lmax is clamped: lmax samples are written and no more; a negative one writes nothing
    name, offsets, total = _layouts()[1]
    offs = torch.from_numpy(offsets).to(cuda)
    bad = torch.tensor([-5, 7, 8, 9, 100000], dtype=torch.int32, device=cuda)
    flat = torch.full((total,), FILL, dtype=torch.int16, device=cuda)
    rg.unframe_ragged_pcm16(buf, geo, bad, None, LMAX, flat, offs, 0)
    want = [P.quantise(e, 0) for e in elem]
    want[0] = want[0][:0]
    _check_flat(flat, offsets, total, want, "clamped")


def test_pcm16_from_f32_is_the_rule_bit_for_bit(cuda):
    from cleanumamba_amd.network import ragged as rg
    rng = np.random.default_rng(6)
    for stride in (LMAX, 4104):                                # rows off and on the 16-byte boundary
        x = rng.uniform(-1.1, 1.1, (len(LENS), stride)).astype(np.float32)
        for b, n in enumerate(LENS):
            x[b, :n] = _values(rng, n, b)
        xd = torch.from_numpy(x).to(cuda)
        lens = torch.tensor(LENS, dtype=torch.int32, device=cuda)
        for name, offsets, total in _layouts():
            offs = torch.from_numpy(offsets).to(cuda)
            for mode in (0, 1):
                want = [P.quantise(x[b, :n], mode) for b, n in enumerate(LENS)]
                flat = torch.full((total,), FILL, dtype=torch.int16, device=cuda)
                rg.pcm16_from_f32_ragged(xd, lens, flat, offs, mode)
                _check_flat(flat, offsets, total, want, (stride, name, mode))
                again = torch.full((total,), FILL, dtype=torch.int16, device=cuda)
                rg.pcm16_from_f32_ragged(xd, lens, again, offs, mode)
                assert torch.equal(flat, again)
    bad = torch.tensor([1, 7, 8, 9, 1 << 30], dtype=torch.int32, device=cuda)
    name, offsets, total = _layouts()[1]
    flat = torch.full((total,), FILL, dtype=torch.int16, device=cuda)
    rg.pcm16_from_f32_ragged(xd[:, :LMAX], bad, flat, torch.from_numpy(offsets).to(cuda), 1)     # lmax 4099, stride 4104
    _check_flat(flat, offsets, total, [P.quantise(x[b, :n], 1) for b, n in enumerate(LENS)], "clamped")


def test_bad_arguments_are_refused_with_real_buffers(cuda):
    from cleanumamba_amd import hip
    from cleanumamba_amd.network import convstack as cs
    lib = hip.lib()
    geo = cs.Geo(2, 64, 1)
    buf = geo.new(torch.float32, cuda, zero=True)
    lens = torch.tensor([60, 64], dtype=torch.int32, device=cuda)
    offs = torch.tensor([0, 60], dtype=torch.int64, device=cuda)
    flat = torch.full((124,), FILL, dtype=torch.int16, device=cuda)
    x = torch.zeros(2, 64, device=cuda)
    st = hip.stream_ptr()
    p = hip.ptr
    assert lib.cum_unframe_rows_ragged_pcm16(0, p(buf), 2, 64, 64, p(lens), None, 2, p(flat), p(offs), st) == -1
    assert lib.cum_unframe_rows_ragged_pcm16(0, p(buf), 0, 64, 64, p(lens), None, 0, p(flat), p(offs), st) == -1
    assert lib.cum_unframe_rows_ragged_pcm16(0, None, 2, 64, 64, p(lens), None, 0, p(flat), p(offs), st) == -1
    assert lib.cum_unframe_rows_ragged_pcm16(0, p(buf), 2, 64, 64, None, None, 0, p(flat), p(offs), st) == -1
    assert lib.cum_unframe_rows_ragged_pcm16(0, p(buf), 2, 64, 64, p(lens), None, 0, None, p(offs), st) == -1
    assert lib.cum_unframe_rows_ragged_pcm16(0, p(buf), 2, 64, 64, p(lens), None, 0, p(flat), None, st) == -1
    assert lib.cum_pcm16_from_f32_ragged(p(x), 2, 64, 64, p(lens), 2, p(flat), p(offs), st) == -1
    assert lib.cum_pcm16_from_f32_ragged(p(x), 0, 64, 64, p(lens), 0, p(flat), p(offs), st) == -1
    assert lib.cum_pcm16_from_f32_ragged(None, 2, 64, 64, p(lens), 0, p(flat), p(offs), st) == -1
    assert lib.cum_pcm16_from_f32_ragged(p(x), 2, 64, 64, p(lens), 0, p(flat), ctypes.c_void_p(offs.data_ptr() + 4), st) == -1
    torch.cuda.synchronize()
    assert bool((flat == FILL).all())
    assert lib.cum_unframe_rows_ragged_pcm16(0, p(buf), 2, 64, 64, p(lens), None, 0, p(flat), p(offs), st) == 0
    torch.cuda.synchronize()
    assert bool((flat == 0).all())                             # a fresh row buffer is zeros


# ------------------------------------------------------------------------------------------------ whole model, f32
def _torch_rule(y, mode):
    if mode == 0:
        return (y * 32767).clamp(-32768, 32767).to(torch.int16)
    return (y * 32768).round().clamp(-32768, 32767).to(torch.int16)


@pytest.fixture(scope="module")
def net(cuda):
    from cleanumamba_amd.network import CleanUMamba
    sd, cfg = load_ckpt("442k")
    model = CleanUMamba(**cfg)
    model.load_state_dict(sd, strict=True)
    return model.to(cuda).float().eval()


def test_denoise_batch_pcm16_is_the_quantised_denoise_batch(cuda, net, monkeypatch):
    from cleanumamba_amd.network import blockdenoise
    hop, F = net.total_stride, net.valid_length(1)
    lengths = [hop * k + F + d for k in (1, 3) for d in (-1, 0, 1)] + [480, 8000]
    g = torch.Generator().manual_seed(7)
    clips = [0.1 * torch.randn(n, generator=g) + 0.02 for n in lengths]
    long_calls = []
    real = blockdenoise.denoise_long
    monkeypatch.setattr(blockdenoise, "denoise_long", lambda m, x, **kw: (long_calls.append(int(x.shape[-1])), real(m, x, **kw))[1])
    with torch.no_grad():
        for budget in (32 * 160000, 4000):                     # 4000: the 8000-sample clip alone goes through denoise_long
            want = net.denoise_batch(clips, budget_samples=budget)
            for mode in (0, 1):
                flat, offsets, lens = net.denoise_batch_pcm16(clips, mode=mode, budget_samples=budget)
                assert flat.dtype == torch.int16 and flat.is_cuda and flat.shape == (sum(lengths),)
                assert lens.tolist() == lengths and offsets.tolist() == (np.cumsum(lengths) - lengths).tolist()
                for i, (o, n) in enumerate(zip(offsets.tolist(), lengths)):
                    assert torch.equal(flat[o:o + n], _torch_rule(want[i], mode)), (budget, mode, i, n)
                assert int(flat.abs().max()) > 1000            # the clips are not silence
    assert long_calls == [8000] * 3                            # once per denoise_batch / denoise_batch_pcm16 call at 4000
    # int16 clips in: the same samples
    pcm = [(c * 32768).round().clamp(-32768, 32767).to(torch.int16) for c in clips]
    with torch.no_grad():
        a = net.denoise_batch_pcm16(pcm, mode=0)[0]
        b = net.denoise_batch_pcm16([p.float() / 32768.0 for p in pcm], mode=0)[0]
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="mode"):
        net.denoise_batch_pcm16(clips, mode=2)
