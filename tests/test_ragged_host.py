"""Host side of the ragged inference batches (network/ragged.py, util/dataset.py NosyOnlyDataset, examples/denoise.py) and
the argument checks of their C entries, which run before any launch and therefore without a GPU.

The mask rule is pinned here in f64 on the oracle (oracle/cleanumamba_ref.py): a zero-padded batch equals the lone
forwards once every decoder layer's GLU output is cleared past ``level_rows`` -- and does not without."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from scipy.io import wavfile

import wavtree
from conftest import load_ckpt, rel_l2
from oracle import cleanumamba_ref as R

LENGTHS = [300, 766, 767, 1500, 2047, 1022, 1023]       # 442k: E = 8, hop 256, frame 766
_cache = {}


def _sd64():
    if "sd" not in _cache:
        sd, cfg = load_ckpt("442k")
        _cache["sd"] = ({k: v.double() for k, v in sd.items()}, cfg)
    return _cache["sd"]


def _clips():
    g = torch.Generator().manual_seed(7)
    return [0.1 * torch.randn(n, generator=g, dtype=torch.float64) + 0.02 for n in LENGTHS]


@pytest.mark.parametrize("L", [1, 300, 766, 767, 1022, 1023, 2047])
def test_level_rows_are_the_shapes_of_the_reference_forward(L):
    from cleanumamba_amd.network.ragged import level_rows
    sd, cfg = _sd64()
    E = cfg["encoder_n_layers"]
    x = torch.randn(1, 1, L, dtype=torch.float64, generator=torch.Generator().manual_seed(L))
    with torch.no_grad():
        y, skips, _ = R.forward_ref(sd, x, normalize_input=False, return_intermediates=True)
    rows = level_rows(L, E, cfg["kernel_size"], cfg["stride"])
    assert len(rows) == E + 1
    assert rows[0] == y.shape[-1] == R.valid_length(L, E)
    for j in range(E):                                   # skips: deepest first = level E - j
        assert rows[E - j] == skips[j].shape[-1], (L, j)


def _padded_batch_forward(sd, clips, masks):
    """The oracle's forward on the zero-padded batch, every clip divided by its own std and cropped to its own length;
    masks: clear the GLU output of decoder layer j past level_rows(L_b)[E - j] (what forward_ragged does)."""
    from cleanumamba_amd.network.ragged import level_rows
    E = R.count_layers(sd, "encoder.")
    Lmax = max(len(c) for c in clips)
    std = [c.std() + 1e-3 for c in clips]
    x = torch.zeros(len(clips), 1, R.valid_length(Lmax, E), dtype=torch.float64)
    for b, c in enumerate(clips):
        x[b, 0, :len(c)] = c / std[b]
    levels = [level_rows(len(c), E) for c in clips]
    skips = []
    for i in range(E):
        x = R.encoder_layer(sd, i, x)
        skips.append(x)
    skips = skips[::-1]
    x, _ = R.bottleneck(sd, x)
    for j in range(E):
        x = x + skips[j][:, :, :x.shape[-1]]
        p = f"decoder.{j}."
        g = R.glu(F.conv1d(x, sd[p + "0.weight"], sd[p + "0.bias"]))
        if masks:
            for b in range(len(clips)):
                g[b, :, levels[b][E - j]:] = 0
        x = F.conv_transpose1d(g, sd[p + "2.weight"], sd[p + "2.bias"], stride=2)
        x = x if j == E - 1 else F.relu(x)
    return [x[b, 0, :len(c)] * std[b] for b, c in enumerate(clips)]


def test_mask_rule_on_the_f64_oracle():
    sd, _ = _sd64()
    clips = _clips()
    with torch.no_grad():
        alone = [R.forward_ref(sd, c.view(1, 1, -1))[0, 0] for c in clips]
        masked = _padded_batch_forward(sd, clips, masks=True)
        naive = _padded_batch_forward(sd, clips, masks=False)
    Lmax = max(LENGTHS)
    for n, a, m, v in zip(LENGTHS, alone, masked, naive):
        print(n, "masked", rel_l2(m, a), "naive", rel_l2(v, a))
        assert rel_l2(m, a) < 1e-12, n
        if n < Lmax:                                     # the guard against this test going blind
            assert rel_l2(v, a) > 1e-2, n


def _check_plan(lengths, valid_length, **kw):
    from cleanumamba_amd.network.ragged import plan_batches
    max_batch = kw.get("max_batch", 32)
    budget = kw.get("budget_samples", 32 * 160000)
    max_waste = kw.get("max_waste", 0.25)
    plan = plan_batches(lengths, valid_length, **kw)
    seen = sorted(i for b in plan for i in b.indices)
    assert seen == list(range(len(lengths)))
    for b in plan:
        vl = [valid_length(lengths[i]) for i in b.indices]
        if b.long:
            assert len(b.indices) == 1 and vl[0] > budget
            continue
        assert all(v <= budget for v in vl)
        assert 1 <= len(b.indices) <= max_batch
        assert len(b.indices) * max(vl) <= budget
        assert 1 - sum(vl) / (len(b.indices) * max(vl)) <= max_waste
        assert vl[0] == max(vl)                          # longest first
    return plan


def test_plan_batches_bounds_and_coverage():
    vl = lambda n: R.valid_length(n, 8)
    rng = random.Random(3)
    sets = {
        "random": [rng.randint(1, 200000) for _ in range(300)],
        "vctk": [rng.randint(20000, 240000) for _ in range(824)],
        "equal": [48000] * 70,
        "giant": [6000000] + [rng.randint(1000, 4000) for _ in range(40)] + [5200000],
        "geometric": [int(100 * 1.5 ** k) for k in range(28)],
        "one": [5],
        "empty": [],
    }
    for name, lengths in sets.items():
        for kw in ({}, {"max_batch": 4}, {"max_waste": 0.0}, {"budget_samples": 500000}, {"max_batch": 1}):
            _check_plan(lengths, vl, **kw)
    plan = _check_plan(sets["equal"], vl)
    assert [len(b.indices) for b in plan] == [32, 32, 6]
    plan = _check_plan(sets["giant"], vl)
    assert sorted(b.indices[0] for b in plan if b.long) == [0, 41]
    # no padding allowed: only clips of one padded length share a batch
    for b in _check_plan(sets["geometric"], vl, max_waste=0.0):
        assert len({vl(sets["geometric"][i]) for i in b.indices}) == 1
    # a budget below every clip: every clip is long, none is dropped
    assert all(b.long for b in _check_plan([3000, 4000], vl, budget_samples=1000))


def _folder(tmp_path):
    folder = tmp_path / "noisy"
    folder.mkdir()
    mono = wavtree.pcm(1234, 1)
    wavfile.write(str(folder / "b_mono.wav"), 16000, mono)
    stereo = np.stack([wavtree.pcm(777, 2), wavtree.pcm(777, 3)], 1)
    wavfile.write(str(folder / "a_stereo.wav"), 16000, stereo)
    flt = (wavtree.pcm(500, 4).astype(np.float32) / 32768.0)
    wavfile.write(str(folder / "c_float.wav"), 16000, flt)
    wavtree.write_raw(str(folder / "d_ext.wav"), wavtree.pcm(9, 5), extensible=True, chunks=[(b"LIST", b"abc")])
    return str(folder), {"b_mono.wav": mono, "a_stereo.wav": stereo[:, 0], "c_float.wav": flt, "d_ext.wav": wavtree.pcm(9, 5)}


def test_noisy_only_dataset_reads_channel_zero(tmp_path):
    from cleanumamba_amd.util.dataset import NosyOnlyDataset, load_NoisyDataset
    folder, want = _folder(tmp_path)
    ds = NosyOnlyDataset(folder=folder)
    assert ds.noisy_files == sorted(want) and len(ds) == 4 and ds.crop_length_sec == 0
    for n, name in enumerate(ds.noisy_files):
        a, b, rng, fileid = ds[n]
        w = want[name]
        wf = w if w.dtype == np.float32 else w.astype(np.float32) / np.float32(32768.0)
        assert fileid == name and rng == (-1, 1) and a is b
        assert a.dtype == torch.float32 and a.dim() == 1 and np.array_equal(a.numpy(), wf)
        if w.dtype == np.int16:
            assert np.array_equal(ds.read_pcm(n), w)
            out = np.full(len(w) + 3, 99, dtype=np.int16)
            got = ds.read_pcm(n, out=out)
            assert np.array_equal(got, w) and np.array_equal(out[len(w):], [99] * 3)
        else:
            with pytest.raises(ValueError, match="16-bit PCM"):
                ds.read_pcm(n)
    loader = load_NoisyDataset(folder=folder, batch_size=1, sample_rate=16000, num_gpus=1)
    names = []
    for a, b, rng, fileid in loader:                     # the reference's loop: for noisy1, noisy, _, filename in loader
        assert a.shape == b.shape and a.dim() == 2 and a.shape[0] == 1
        names.append(fileid[0])
    assert sorted(names) == sorted(want)


def test_a_rate_mismatch_raises_before_any_gpu_call(tmp_path, monkeypatch):
    from cleanumamba_amd.examples import denoise as D
    folder, _ = _folder(tmp_path)
    wavfile.write(os.path.join(folder, "e_8k.wav"), 8000, wavtree.pcm(100, 6))
    wavfile.write(os.path.join(folder, "f_48k.wav"), 48000, wavtree.pcm(100, 7))

    def no_gpu(*a, **k):
        raise AssertionError("the checkpoint was loaded before the rates were checked")
    monkeypatch.setattr(D, "load_pretrained_CleanUMamba", no_gpu)
    monkeypatch.setattr(torch.Tensor, "cuda", no_gpu)
    with pytest.raises(ValueError) as err:
        D.denoise("no_such_checkpoint.pkl", folder, str(tmp_path / "out"))
    assert "e_8k.wav" in str(err.value) and "f_48k.wav" in str(err.value) and "b_mono.wav" not in str(err.value)
    assert not (tmp_path / "out").exists()


def test_lengths_are_checked_before_any_gpu_work():
    """A length below 1, or below 2 with normalize_input, is a ValueError raised on the host (the model here lives on the
    CPU: anything that reached a kernel would raise RuntimeError instead)."""
    from cleanumamba_amd.network import CleanUMamba
    _, cfg = load_ckpt("442k")
    net = CleanUMamba(**cfg).eval()
    with pytest.raises(ValueError, match="at least 2"):
        net.denoise_batch([torch.zeros(100), torch.zeros(1)])
    with pytest.raises(ValueError, match="at least 2"):
        net.denoise_batch([torch.zeros(0, dtype=torch.int16)])
    net.normalize_input = False
    with pytest.raises(ValueError, match="at least 1"):
        net.denoise_batch([torch.zeros(100), torch.zeros(0)])
    with pytest.raises(ValueError, match="1-D"):
        net.denoise_batch([torch.zeros(2, 100)])
    with pytest.raises(RuntimeError, match="no_grad"):
        net.forward_ragged(torch.zeros(1, 100), [100])


def test_new_symbols_and_their_argument_errors_need_no_gpu():
    from cleanumamba_amd import hip
    lib = hip.lib()
    P = ctypes.c_void_p
    names = ["cum_clip_std_ragged", "cum_frame_rows_ragged", "cum_rows_zero_tail", "cum_unframe_rows_ragged",
             "cum_dech_fwd_ragged", "cum_dec7_fwd_ragged"]
    for name in names:
        assert hasattr(lib, name) and name in hip.SIGNATURES
    assert lib.cum_abi_version() == 16

    def sweep(fn, order, ok, bad):
        for name, value, text in bad:
            args = dict(ok, **{name: value})
            rc = fn(*[args[k] for k in order], None)
            assert rc == -1, (fn.__name__, name, value)
            assert text in lib.cum_last_error(), (fn.__name__, name, value, lib.cum_last_error())

    sweep(lib.cum_clip_std_ragged, ["src", "x", "B", "lmax", "stride", "len", "eps", "out"],
          dict(src=1, x=P(0x1000), B=3, lmax=100, stride=104, len=P(0x2000), eps=1e-3, out=P(0x3000)),
          [("B", 0, b"batch"), ("B", -1, b"batch"), ("lmax", 0, b"lmax"), ("stride", 99, b"stride"), ("x", None, b"null"),
           ("len", None, b"null"), ("out", None, b"null"), ("x", P(0x1001), b"misaligned"), ("len", P(0x2002), b"misaligned"),
           ("src", 2, b"src_i16")])
    sweep(lib.cum_frame_rows_ragged, ["dt", "src", "x", "B", "lmax", "stride", "len", "T", "R", "scale", "out"],
          dict(dt=2, src=1, x=P(0x1000), B=3, lmax=100, stride=104, len=P(0x2000), T=766, R=1 + 3 * 768 + 18,
               scale=P(0x3000), out=P(0x4000)),
          [("B", 0, b"batch"), ("lmax", 0, b"lmax"), ("T", 99, b"T and stride"), ("R", 3 * 768, b"too small"),
           ("x", None, b"null"), ("len", None, b"null"), ("out", None, b"null"), ("out", P(0x4008), b"16-byte"),
           ("scale", P(0x3002), b"misaligned"), ("dt", 7, b"dtype")])
    sweep(lib.cum_rows_zero_tail, ["dt", "rows", "B", "T", "cp", "valid"],
          dict(dt=0, rows=P(0x1000), B=3, T=382, cp=40, valid=P(0x2000)),
          [("B", 0, b"batch"), ("T", 0, b"T must"), ("cp", 35, b"multiple of 8"), ("cp", 0, b"multiple of 8"),
           ("rows", None, b"null"), ("valid", None, b"null"), ("rows", P(0x1008), b"16-byte"), ("valid", P(0x2001), b"aligned")])
    sweep(lib.cum_unframe_rows_ragged, ["dt", "rows", "B", "lmax", "T", "len", "scale", "y"],
          dict(dt=1, rows=P(0x1000), B=3, lmax=100, T=766, len=P(0x2000), scale=None, y=P(0x3000)),
          [("B", 0, b"batch"), ("lmax", 0, b"lmax"), ("T", 50, b"T must"), ("rows", None, b"null"), ("len", None, b"null"),
           ("y", None, b"null"), ("rows", P(0x1004), b"16-byte"), ("y", P(0x3002), b"misaligned")])
    ok = dict(dt=2, M=3 * 40, pitch=40, valid=38, vr=P(0x9000), B=3, u=P(0x1000), u_rows=200, w1p=P(0x2000), b1p=P(0x3000),
              wtp=P(0x4000), btp=P(0x5000), skip=P(0x6000), out=P(0x7000), out_tail=0)
    sweep(lib.cum_dech_fwd_ragged, ["dt", "M", "pitch", "valid", "vr", "B", "u", "u_rows", "w1p", "b1p", "wtp", "btp", "skip",
                                    "out", "out_tail"], ok,
          [("B", 0, b"bad sizes"), ("M", 3 * 40 + 1, b"batch x pitch"), ("vr", None, b"null"), ("u", None, b"null"),
           ("out", None, b"null"), ("vr", P(0x9002), b"aligned"), ("u", P(0x1008), b"aligned"), ("dt", 0, b"16-bit")])
    ok = dict(dt=2, M=3 * 40, pitch=40, valid=38, vr=P(0x9000), B=3, u=P(0x1000), w1p=P(0x2000), b1p=P(0x3000),
              wt=P(0x4000), bt=P(0x5000), out=P(0x7000), tail=0)
    sweep(lib.cum_dec7_fwd_ragged, ["dt", "M", "pitch", "valid", "vr", "B", "u", "w1p", "b1p", "wt", "bt", "out", "tail"], ok,
          [("B", 0, b"bad geometry"), ("M", 3 * 40 - 1, b"batch x pitch"), ("pitch", 16, b"bad geometry"),
           ("vr", None, b"null"), ("u", None, b"null"), ("out", None, b"null"), ("vr", P(0x9001), b"aligned"),
           ("out", P(0x7008), b"aligned"), ("dt", 0, b"16-bit")])
