"""The resampler on the GPU (csrc/resample.hip, util/resample.py) and the three places it is used: ``denoise_batch``
with ``rates``, ``denoise_long`` with ``rate`` and the folder CLI with ``resample=True``.

The kernel is held to the f64 definition (tests/resample_ref.py) element by element: an output is one K-term f32 fma chain
over f32 taps and f32 samples, so |y[m] - ref[m]| <= (K + 4) 2^-24 A[m] with A[m] = sum |x[n]| |h[..]| -- K roundings of
the chain, and the roundings of taps (and products' operands) to f32.  Derived, not measured; the measured worst ratio
is recorded.  Everything about batches and streams is bit equality, which the fixed order of that chain gives."""
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import wavtree
from conftest import load_ckpt, record
from resample_ref import resample_ref

pytestmark = pytest.mark.gpu
PAIRS = [(48000, 16000), (44100, 16000), (16000, 48000), (16000, 44100), (22050, 16000), (8000, 16000), (32000, 16000)]
_cache = {}


def _lengths(p, T):
    """1, 2, 3, K - 1, K, K + 1, the shortest inputs with at least T - 1, T and T + 1 outputs, 4099."""
    from cleanumamba_amd.util.resample import out_length
    edge = []
    for n in (T - 1, T, T + 1):
        L = n * p.down // p.up
        while out_length(L, p.up, p.down) < n:
            L += 1
        edge.append(L)
    return [1, 2, 3, p.K - 1, p.K, p.K + 1] + edge + [4099]


def _batch(p, T, kind, seed):
    """-> (clips as 1-D host tensors, the same samples as f64 arrays)."""
    rng = np.random.default_rng(seed)
    clips, exact = [], []
    for n in _lengths(p, T):
        if kind == "int16":
            x = wavtree.pcm(n, int(rng.integers(1 << 30)))
            clips.append(torch.from_numpy(x))
            exact.append(x.astype(np.float64) / 32768.0)
        else:
            x = rng.standard_normal(n).astype(np.float32)
            clips.append(torch.from_numpy(x))
            exact.append(x.astype(np.float64))
    return clips, exact


def _stack(clips, device, pitch=None, fill=0):
    Lmax = max(len(c) for c in clips)
    x = torch.full((len(clips), pitch or Lmax), fill, dtype=clips[0].dtype)
    for b, c in enumerate(clips):
        x[b, :len(c)] = c
    return x.to(device)


@pytest.mark.parametrize("kind", ["int16", "f32"])
@pytest.mark.parametrize("pair", PAIRS)
def test_kernel_against_the_f64_definition(cuda, pair, kind):
    from cleanumamba_amd import hip
    from cleanumamba_amd.util.resample import out_length, plan, resample_ragged
    p = plan(*pair)
    T = hip.lib().cum_resample_tile()
    clips, exact = _batch(p, T, kind, sum(pair))
    lens = [len(c) for c in clips]
    y, out_lens = resample_ragged(_stack(clips, cuda), lens, *pair)
    assert y.dtype == torch.float32 and y.shape[0] == len(clips) and y.shape[1] >= max(out_lens)
    assert out_lens == [out_length(n, p.up, p.down) for n in lens]
    assert {T - 1, T, T + 1} <= set(out_lens) or p.up > p.down          # (an upsampler skips some counts)
    got = y.cpu().double().numpy()
    worst = 0.0
    for b, x in enumerate(exact):
        ref, A = resample_ref(x, p.taps, p.up, p.down)
        err = np.abs(got[b, :out_lens[b]] - ref)
        bound = (p.K + 4) * 2.0 ** -24 * A
        worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
        assert np.all(err <= bound), (pair, kind, lens[b], float(np.max(err / np.maximum(bound, 1e-300))))
    print(pair, kind, "worst error / bound", worst)
    record(f"resample_{pair[0]}_{pair[1]}_{kind}_err_over_bound", worst)


@pytest.mark.parametrize("kind", ["int16", "f32"])
@pytest.mark.parametrize("pair", [(48000, 16000), (16000, 44100), (44100, 16000)])
def test_pads_batch_mates_and_reruns_do_not_matter(cuda, pair, kind):
    """Poisoned input pads (NaN / 32767) are never read, the sentinel behind every output row survives, rows that are
    not 16-byte aligned (odd pitch: the narrow loads) give the same bits, and so do a clip alone, a device length table
    and a second run."""
    from cleanumamba_amd import hip
    from cleanumamba_amd.util.resample import plan, resample_ragged
    p = plan(*pair)
    T = hip.lib().cum_resample_tile()
    clips, _ = _batch(p, T, kind, 5)
    lens = [len(c) for c in clips]
    Lmax = max(lens)
    base, out_lens = resample_ragged(_stack(clips, cuda), lens, *pair)
    poison = float("nan") if kind == "f32" else 32767
    for pitch in (Lmax + 8, Lmax + 13):
        x = _stack(clips, cuda, pitch=pitch, fill=poison)
        out = torch.full((len(clips), base.shape[1] + 24), -7.5, device=cuda)
        y, n = resample_ragged(x, lens, *pair, out=out)
        assert y is out and n == out_lens
        for b in range(len(clips)):
            assert torch.equal(out[b, :n[b]], base[b, :n[b]]), (pitch, b)
            assert bool((out[b, n[b]:] == -7.5).all()), (pitch, b)
    again, _ = resample_ragged(_stack(clips, cuda), lens, *pair)
    table, n_dev = resample_ragged(_stack(clips, cuda), torch.tensor(lens, dtype=torch.int32, device=cuda), *pair)
    assert n_dev.dtype == torch.int32 and n_dev.tolist() == out_lens
    for b, c in enumerate(clips):
        alone, n = resample_ragged(c.to(cuda).view(1, -1), [lens[b]], *pair)
        assert n == [out_lens[b]]
        assert torch.equal(alone[0, :n[0]], base[b, :n[0]]), b
        assert torch.equal(again[b, :n[0]], base[b, :n[0]]) and torch.equal(table[b, :n[0]], base[b, :n[0]])


def test_equal_rates_return_the_input(cuda):
    from cleanumamba_amd.util.resample import resample_ragged
    x = torch.from_numpy(np.stack([wavtree.pcm(100, 1), wavtree.pcm(100, 2)])).to(cuda)
    y, n = resample_ragged(x, [100, 7], 16000, 16000)
    assert n == [100, 7] and torch.equal(y, x.float() / 32768.0)
    f = torch.randn(2, 50, device=cuda)
    assert resample_ragged(f, [50, 50], 44100, 44100)[0] is f


@pytest.mark.parametrize("kind", ["int16", "f32"])
@pytest.mark.parametrize("pair", [(48000, 16000), (16000, 48000), (44100, 16000), (16000, 44100)])
def test_stream_resampler_is_the_whole_signal_however_it_is_cut(cuda, pair, kind):
    from cleanumamba_amd.util.resample import StreamResampler, final_outputs, out_length, plan, resample_ragged
    p = plan(*pair)
    L = 20000
    if kind == "int16":
        x = torch.from_numpy(np.stack([wavtree.pcm(L, 11), wavtree.pcm(L, 12)]))
    else:
        x = torch.randn(2, L, generator=torch.Generator().manual_seed(3))
    whole, n = resample_ragged(x.to(cuda), [L, L], *pair)
    whole = whole[:, :n[0]]
    assert n == [out_length(L, p.up, p.down)] * 2
    for cuts in ([1, 0, 7, 1000, 3, None], [None]):
        s = StreamResampler(2, *pair, cuda)
        pos, emitted, parts = 0, 0, []
        for c in cuts:
            c = L - pos if c is None else c
            piece = x[:, pos:pos + c]
            y = s.push(piece if len(parts) % 2 else piece.to(cuda))          # host and device pieces alike
            assert y.device == (piece.device if len(parts) % 2 else cuda) and y.dtype == torch.float32
            pos += c
            want = final_outputs(pos, p.up, p.down, p.H)
            assert y.shape == (2, want - emitted), (cuts, pos)
            emitted = want
            parts.append(y.to(cuda))
        assert pos == L and emitted < n[0]
        parts.append(s.finish())
        assert torch.equal(torch.cat(parts, 1), whole), cuts
        with pytest.raises(RuntimeError, match="finish"):
            s.push(x[:, :1])
        with pytest.raises(RuntimeError, match="finish"):
            s.finish()
    assert s.hist is None
    same = StreamResampler(2, 16000, 16000, cuda)
    assert torch.equal(same.push(x[:, :9].to(cuda)), (x[:, :9].float() * (2.0 ** -15 if kind == "int16" else 1)).to(cuda))
    assert same.finish().shape == (2, 0)


# ------------------------------------------------------------------------------------------------ filter quality
def _db(a, ref):
    return 10 * float(torch.log10(a.double().square().mean() / ref.double().square().mean()))


def _tones(rate, freqs):
    t = torch.arange(rate, dtype=torch.float64) / rate                       # 1 s
    return sum(torch.sin(2 * np.pi * f * t + 0.3 * k) for k, f in enumerate(freqs)).float() * 0.4


@pytest.mark.parametrize("rate", [48000, 44100, 32000, 22050])
def test_a_tone_above_the_new_nyquist_rate_is_rejected(cuda, rate):
    """10 kHz cannot exist at 16 kHz: what is left of it is at most -70 dB of the input (the taps give -72.6 ... -74.9 dB
    on the f64 definition; the f32 kernel adds about -140 dB)."""
    from cleanumamba_amd.util.resample import resample_ragged
    x = _tones(rate, [10000]).to(cuda)
    y, n = resample_ragged(x.view(1, -1), [rate], rate, 16000)
    assert n == [16000]
    left = _db(y[0, 2000:n[0] - 2000], x)
    print(rate, "10 kHz tone after conversion:", left, "dB")
    record(f"resample_alias_db_{rate}", left)
    assert left <= -70.0


@pytest.mark.parametrize("rate,freqs", [(48000, (1000, 6500)), (44100, (1000, 6500)), (32000, (1000, 6500)),
                                        (22050, (1000, 6500)), (8000, (1000, 3000))])
def test_a_round_trip_gives_the_signal_back(cuda, rate, freqs):
    """In-band tones to 16 kHz and back differ from the original by at most -70 dB (-72.9 ... -78.2 dB on the f64
    definition), away from the 2000 samples at each end."""
    from cleanumamba_amd.util.resample import resample_ragged
    x = _tones(rate, freqs).to(cuda)
    mid, n = resample_ragged(x.view(1, -1), [rate], rate, 16000)
    back, m = resample_ragged(mid[:, :n[0]], n, 16000, rate)
    assert m[0] >= rate
    diff = _db(back[0, 2000:rate - 2000] - x[2000:rate - 2000], x)
    print(rate, freqs, "round trip:", diff, "dB")
    record(f"resample_round_trip_db_{rate}", diff)
    assert diff <= -70.0


# ------------------------------------------------------------------------------------------------ the model
def _net(cuda):
    from cleanumamba_amd.network import CleanUMamba
    if "net" not in _cache:
        sd, cfg = load_ckpt("442k")
        net = CleanUMamba(**cfg)
        net.load_state_dict(sd, strict=True)
        _cache["net"] = net.to(cuda).float().eval()
    return _cache["net"]


def _speechlike(n, seed, int16):
    g = torch.Generator().manual_seed(seed)
    x = 0.1 * torch.randn(n, generator=g) + 0.02
    return (x * 32768).round().clamp(-32768, 32767).to(torch.int16) if int16 else x


def test_denoise_batch_with_rates_is_the_hand_made_chain(cuda):
    from cleanumamba_amd.util.resample import resample_ragged
    net = _net(cuda)
    rates = [16000, 48000, 8000, 44100]
    clips = [_speechlike(9000, 1, False), _speechlike(30001, 2, True), _speechlike(5000, 3, True),
             _speechlike(20000, 4, False)]                                   # all under 1.5 s
    with torch.no_grad():
        got = net.denoise_batch(clips, rates=rates)
        at16 = []
        for c, r in zip(clips, rates):
            if r == 16000:
                at16.append(c)
            else:
                y, n = resample_ragged(c.to(cuda).view(1, -1), [len(c)], r, 16000)
                at16.append(y[0, :n[0]])
        plain = net.denoise_batch(at16)
        assert torch.equal(got[0], plain[0])                                 # the 16 kHz clip: the call without rates
        for k in (1, 2, 3):
            y, n = resample_ragged(plain[k].view(1, -1), [len(plain[k])], 16000, rates[k])
            assert n[0] >= len(clips[k])
            assert torch.equal(got[k], y[0, :len(clips[k])]), rates[k]
        for c, y in zip(clips, got):
            assert y.shape == c.shape and y.dtype == torch.float32 and y.is_cuda and bool(torch.isfinite(y).all())
        # one rate for all, and rates that all equal the model's: today's path
        one = net.denoise_batch(clips[1:2], rates=48000)
        assert one[0].shape == clips[1].shape
        same = net.denoise_batch(at16, rates=[16000] * 4)
        assert all(torch.equal(a, b) for a, b in zip(same, plain))
        with pytest.raises(ValueError, match="rates"):
            net.denoise_batch(clips, rates=[16000])
        with pytest.raises(ValueError, match="at least 2"):                  # the converted length is what is checked
            net.denoise_batch([torch.zeros(3)], rates=48000)


def test_denoise_long_with_a_rate_is_the_hand_made_chain(cuda):
    """3 s at 48 kHz on the host: the streamed chain equals resample -> denoise_long -> resample -> crop on the whole
    signal (both take the std from f64 sums over the converted signal), host in gives host out, and a device signal
    gives the same samples on the device."""
    from cleanumamba_amd.util.resample import resample_ragged
    net = _net(cuda)
    L = 144000
    x48 = _speechlike(L, 9, False).view(1, L)
    with torch.no_grad():
        got = net.denoise_long(x48, rate=48000, block_hops=4)
        assert got.shape == (1, 1, L) and not got.is_cuda and got.dtype == torch.float32
        mid, n = resample_ragged(x48.to(cuda), [L], 48000, 16000)
        den = net.denoise_long(mid[:, :n[0]].cpu(), block_hops=4)
        back, m = resample_ragged(den[:, 0].to(cuda), [den.shape[-1]], 16000, 48000)
        assert m[0] >= L
        assert torch.equal(got[0, 0], back[0, :L].cpu())
        dev = net.denoise_long(x48.to(cuda).view(1, 1, L), rate=48000, block_hops=4)
        assert dev.is_cuda and torch.equal(dev.cpu(), got)
        assert torch.equal(net.denoise_long(x48[:, :5000], rate=16000, block_hops=4), net.denoise_long(x48[:, :5000], block_hops=4))


# ------------------------------------------------------------------------------------------------ the folder
FILES = {"a_16k.wav": (16000, 6000), "b_8k.wav": (8000, 1000), "c_44k.wav": (44100, 4410), "d_48k.wav": (48000, 4800)}


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    root = tmp_path_factory.mktemp("resample_folder")
    sd, cfg = load_ckpt("442k")
    ckpt = str(root / "model.pkl")
    torch.save({"network_config": cfg, "model_state_dict": sd}, ckpt)
    for sub in ("mixed", "only16"):
        (root / sub).mkdir()
    rng = np.random.default_rng(0)
    files = {}
    for name, (rate, n) in FILES.items():
        x = np.clip(np.round(3000 * rng.standard_normal(n) + 500), -32768, 32767).astype(np.int16)
        wavfile.write(str(root / "mixed" / name), rate, x)
        files[name] = x
    wavfile.write(str(root / "only16" / "a_16k.wav"), 16000, files["a_16k.wav"])
    return ckpt, root, files


def test_a_folder_of_mixed_rates(cuda, folder):
    """Four files at four rates come back at their own rates and lengths.  The 16 kHz file (much the longest at the
    model's rate, so alone in its batch under the planner's waste bound: the same launches) is the file a folder holding
    it alone gives without ``resample``."""
    from cleanumamba_amd.examples.denoise import denoise
    ckpt, root, files = folder
    out = str(root / "enhanced")
    noisy, cleaned = denoise(ckpt, str(root / "mixed"), out, resample=True)
    names = sorted(FILES)
    assert sorted(os.listdir(out)) == ["enhanced_" + n for n in names]
    for k, name in enumerate(names):
        rate, y = wavfile.read(os.path.join(out, "enhanced_" + name))
        assert (rate, y.shape) == (FILES[name][0], (FILES[name][1],)) and y.dtype == np.float32
        assert np.array_equal(y, cleaned[k]) and np.all(np.isfinite(y)) and float(np.abs(y).max()) > 0
        assert np.array_equal(noisy[k], files[name].astype(np.float32) / np.float32(32768.0))
    alone_noisy, alone = denoise(ckpt, str(root / "only16"), str(root / "enhanced16"))
    assert np.array_equal(alone[0], cleaned[0])
    assert np.array_equal(wavfile.read(str(root / "enhanced16" / "enhanced_a_16k.wav"))[1], cleaned[0])
    with pytest.raises(ValueError, match="b_8k.wav"):
        denoise(ckpt, str(root / "mixed"), str(root / "never"))
    assert not (root / "never").exists()
    # a file over the sample budget takes the streamed route at its own rate
    long_noisy, long_clean = denoise(ckpt, str(root / "mixed"), None, resample=True, budget_samples=1900)
    for k, name in enumerate(names):
        assert long_clean[k].shape == (FILES[name][1],) and np.all(np.isfinite(long_clean[k]))
