"""Wav files and dataset trees written at test time (helpers of test_dataset_host.py, test_feeder_host.py,
test_feeder_gpu.py): plain files through scipy, the odd headers by hand."""
import os
import struct

import numpy as np
from scipy.io import wavfile

KS_PCM_GUID = struct.pack("<H", 1) + bytes.fromhex("000000001000800000aa00389b71")


def pcm(n, seed):
    """n int16 samples over the whole range, including both extremes."""
    x = np.random.default_rng(seed).integers(-32768, 32768, size=n, dtype=np.int64).astype(np.int16)
    if n >= 2:
        x[0], x[-1] = -32768, 32767
    return x


def write_raw(path, samples, rate=16000, extensible=False, chunks=(), data_size=None):
    """A 16-bit mono RIFF file built by hand.  chunks: (id, payload) pairs placed between ``fmt `` and ``data`` (an odd
    payload gets its pad byte); data_size: the size field of ``data`` if it should lie (0, 0xFFFFFFFF)."""
    body = samples.astype("<i2").tobytes()
    if extensible:
        fmt = struct.pack("<HHIIHH", 0xFFFE, 1, rate, 2 * rate, 2, 16) + struct.pack("<HHI", 22, 16, 4) + KS_PCM_GUID
    else:
        fmt = struct.pack("<HHIIHH", 1, 1, rate, 2 * rate, 2, 16)
    out = b"fmt " + struct.pack("<I", len(fmt)) + fmt
    for cid, payload in chunks:
        out += cid + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")
    out += b"data" + struct.pack("<I", len(body) if data_size is None else data_size) + body
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + len(out)) + b"WAVE" + out)


def training_tree(root, lengths, seed=0, rate=16000):
    """``root/training_set/{clean,noisy}/fileid_{i}.wav`` with the given lengths; returns [(clean, noisy)] int16."""
    pairs = []
    for sub in ("clean", "noisy"):
        os.makedirs(os.path.join(root, "training_set", sub), exist_ok=True)
    for i, n in enumerate(lengths):
        pair = (pcm(n, seed + 2 * i), pcm(n, seed + 2 * i + 1))
        for sub, x in zip(("clean", "noisy"), pair):
            wavfile.write(os.path.join(root, "training_set", sub, f"fileid_{i}.wav"), rate, x)
        pairs.append(pair)
    return pairs
