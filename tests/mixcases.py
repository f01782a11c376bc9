"""Shared by test_mix_host.py and test_mix_gpu.py: a tiny tree of separate speech and noise files, the rows a feeder's
plan describes rebuilt from the arrays behind the files, and the rejected argument sets of cum_mix_pairs."""
import ctypes
import os

import numpy as np
from scipy.io import wavfile

import wavtree

# speech: below and above the crop of the tests (1000 + shift), in folders whose names sort differently as strings and
# as listings;  noise: one file shorter than the gap
SPEECH = [("spk10/b.wav", 3000), ("spk2/a.wav", 700), ("spk2/c/d.wav", 1037), ("z.wav", 5000), ("a.wav", 999),
          ("spk10/a.wav", 2500), ("m/x.wav", 1000), ("m/y.wav", 4100)]
NOISE = [("street/n1.wav", 2600), ("cafe.wav", 431), ("street/n0.wav", 37), ("hum/long.wav", 9000)]


def mix_tree(root, seed=0, speech_scale=None):
    """``root/speech`` and ``root/noise`` with the files above; returns (speech_root, noise_root, {path: int16} in the
    sorted order of each root as two lists)."""
    out = []
    for sub, files in (("speech", SPEECH), ("noise", NOISE)):
        made = {}
        for i, (name, n) in enumerate(files):
            path = os.path.join(root, sub, *name.split("/"))
            os.makedirs(os.path.dirname(path), exist_ok=True)
            x = wavtree.pcm(n, seed + 17 * i + (1000 if sub == "noise" else 0))
            if sub == "speech" and i % 2:                 # some quiet speech: the level and the guard have work to do
                x = (x // 64).astype(np.int16)
            wavfile.write(path, 16000, x)
            made[name] = x
        out.append([made[name] for name in sorted(made, key=lambda s: s.split("/"))])
    return os.path.join(root, "speech"), os.path.join(root, "noise"), out[0], out[1]


def sorted_names(files):
    return sorted((name for name, _ in files), key=lambda s: s.split("/"))


def planned_rows(entries, noise_plan, speech, noise, length):
    """(speech rows (B, length) int16 -- the read samples, zeros behind them --, n_speech, noise rows (B, length)) of one
    batch, from the feeder's plan and the arrays behind the files."""
    nb = len(entries)
    S, N = np.zeros((nb, length), np.int16), np.zeros((nb, length), np.int16)
    n_speech = []
    for r, (index, start, count) in enumerate(entries):
        S[r, :count] = speech[index][start:start + count]
        n_speech.append(count)
        for j, at_file, n, at in noise_plan[r]:
            N[r, at:at + n] = noise[j][at_file:at_file + n]
    return S, n_speech, N


def argument_errors():
    """Every rejected argument set of cum_mix_pairs returns CUM_EINVAL with a text, before any launch."""
    from cleanumamba_amd import hip
    lib = hip.lib()
    P = ctypes.c_void_p
    ok = dict(pcm=P(0x1000), pitch=16, recs=P(0x3000), batch=2, len=9, workspace=P(0x6000), clean=P(0x7000), clean_sb=9,
              noisy=P(0x8000), noisy_sb=12, stats=P(0x9000))
    bad = [("batch", 0, b"batch"), ("batch", 32768, b"batch"), ("len", 0, b"len"), ("pitch", 8, b"pitch"),
           ("pitch", 20, b"multiple of 8"), ("clean_sb", 8, b"clean_sb"), ("noisy_sb", 8, b"noisy_sb"),
           ("pcm", None, b"null"), ("recs", None, b"null"), ("workspace", None, b"null"), ("clean", None, b"null"),
           ("noisy", None, b"null"), ("pcm", P(0x1008), b"16-byte"), ("clean", P(0x7004), b"16-byte"),
           ("noisy", P(0x8008), b"16-byte"), ("workspace", P(0x6004), b"8-byte"), ("recs", P(0x3004), b"8-byte"),
           ("stats", P(0x9002), b"4-byte")]
    for name, value, text in bad:
        args = dict(ok, **{name: value})
        rc = lib.cum_mix_pairs(*args.values(), None)
        assert rc == -1 and text in lib.cum_last_error(), (name, value, rc, lib.cum_last_error())
    assert lib.cum_mix_workspace_elems(0, 10) == 0 and lib.cum_mix_workspace_elems(2, 0) == 0
    n = lib.cum_mix_workspace_elems(5, 40003)
    assert n > 0 and n % 2 == 0
    return len(bad)
