"""Clean / noisy recording pairs from a dataset directory, with the interface of the reference's
src/util/dataset.py:30-184 (``CleanNoisyPairDataset``, ``load_CleanNoisyPairDataset``: same names, keywords, defaults,
file layout rules and crop semantics) and without its dependencies: no torchaudio, no torchvision.

Differences on the host side:
  * 16-bit mono PCM -- what DNS and VCTK-DEMAND ship -- is read by a small RIFF reader that touches only the samples of
    the crop and keeps them int16 until the last moment; the reference decodes the whole of both files to float to keep
    a third of them.  Every other encoding (float32, 24-bit, several channels: channel 0 is taken, as the reference's
    noisy-only dataset does) goes through ``scipy.io.wavfile`` and is scaled as util/denoise_eval._read_float scales.
  * ``pair_length(n)``, ``pair_rate(n)`` and ``read_pcm(n, start, count)`` expose the header and a raw int16 range of a
    pair: the fast route of training/feeder.py, which leaves scaling, tiling and -- with ``sample_rate`` -- the conversion
    to the model's rate to the device (csrc/pcm.hip, csrc/resample.hip).
  * the file-count assertions look at the directories the chosen layout reads (the reference always counts
    ``training_set``, also for ``subset="testing"``).
  * ``SpeechNoiseDataset`` has no counterpart in the reference: two unpaired corpora, a tree of speech and a tree of
    noise as the DNS challenge distributes them, for the feeder that mixes on the device (training/mix.py).
The reference's import-time ``random.seed(0) / torch.manual_seed(0) / np.random.seed(0)`` is not repeated: importing a
module here does not reseed the process.  Seed numpy's global generator to reproduce the reference's crops.
"""
import os
import struct

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset
from torch.utils.data.distributed import DistributedSampler

WAVE_FORMAT_PCM, WAVE_FORMAT_IEEE_FLOAT, WAVE_FORMAT_EXTENSIBLE = 0x0001, 0x0003, 0xFFFE
# bytes 2..15 of every KSDATAFORMAT_SUBTYPE_* GUID that wraps a plain format tag (bytes 0..1)
_KS_GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")
PCM_SCALE = 1.0 / 32768.0


class WavInfo:
    """What the header of one RIFF/WAVE file says: format, where the samples start and how many frames there are."""
    __slots__ = ("path", "tag", "channels", "rate", "bits", "block_align", "data_offset", "frames")

    @property
    def is_pcm16_mono(self):
        return self.tag == WAVE_FORMAT_PCM and self.bits == 16 and self.channels == 1 and self.block_align == 2

    def describe(self):
        kind = {WAVE_FORMAT_PCM: "PCM", WAVE_FORMAT_IEEE_FLOAT: "IEEE float"}.get(self.tag, "format tag 0x%04x" % self.tag)
        return f"{kind}, {self.bits}-bit, {self.channels} channel(s)"


def read_wav_info(path):
    """Parse the chunks of ``path`` up to ``data``.  Unknown chunks are skipped with the pad byte an odd size carries; a
    ``data`` size of 0 or 0xFFFFFFFF (a streamed writer that never went back), or one that runs past the end of the file,
    means "to the end of the file"."""
    info = WavInfo()
    info.path = path
    info.tag = None
    file_size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise ValueError(f"{path}: not a RIFF/WAVE file")
        while True:
            ck = f.read(8)
            if len(ck) < 8:
                raise ValueError(f"{path}: no 'data' chunk" if info.tag is not None else f"{path}: no 'fmt ' chunk")
            cid, size = ck[:4], struct.unpack("<I", ck[4:])[0]
            if cid == b"fmt ":
                body = f.read(size)
                if size < 16 or len(body) < size:
                    raise ValueError(f"{path}: truncated 'fmt ' chunk")
                info.tag, info.channels, info.rate, _, info.block_align, info.bits = struct.unpack("<HHIIHH", body[:16])
                if info.tag == WAVE_FORMAT_EXTENSIBLE and size >= 40 and body[26:40] == _KS_GUID_TAIL:
                    info.tag = struct.unpack("<H", body[24:26])[0]
                if size & 1:
                    f.seek(1, os.SEEK_CUR)
            elif cid == b"data":
                if info.tag is None:
                    raise ValueError(f"{path}: 'data' chunk before 'fmt '")
                info.data_offset = f.tell()
                rest = file_size - info.data_offset
                if size == 0 or size == 0xFFFFFFFF or size > rest:
                    size = rest
                if info.block_align < 1:
                    raise ValueError(f"{path}: block align of {info.block_align}")
                info.frames = size // info.block_align
                return info
            else:
                f.seek(size + (size & 1), os.SEEK_CUR)


def _read_range_int16(info, start, count, out=None):
    """Frames [start, start + count) of a 16-bit mono PCM file as int16, read straight into ``out`` if given."""
    if out is None:
        out = np.empty(count, dtype=np.int16)
    dst = out[:count]
    if count == 0:
        return dst
    with open(info.path, "rb", buffering=0) as f:
        f.seek(info.data_offset + 2 * start)
        view, got = memoryview(dst).cast("B"), 0
        while got < len(view):
            k = f.readinto(view[got:])
            if not k:
                raise ValueError(f"{info.path}: file ends {len(view) - got} bytes before sample {start + count}")
            got += k
    if dst.dtype.byteorder == ">":        # (never on the machines this runs on; the file is little-endian)
        dst.byteswap(inplace=True)
    return dst


def _read_whole_float(path):
    """Any encoding scipy reads, as a 1-D float32 array (channel 0), scaled as util/denoise_eval._read_float scales."""
    from scipy.io import wavfile
    rate, x = wavfile.read(path)
    if x.ndim == 2:
        x = x[:, 0]
    if x.dtype == np.int16:
        x = x.astype(np.float32) * np.float32(PCM_SCALE)
    elif x.dtype == np.int32:
        x = x.astype(np.float32) / 2147483648.0
    elif x.dtype == np.uint8:
        x = (x.astype(np.float32) - 128.0) / 128.0
    else:
        x = x.astype(np.float32)
    return rate, np.ascontiguousarray(x, dtype=np.float32)


def _identity(x, bits):
    return x


class CleanNoisyPairDataset(Dataset):
    """Element n: ``(clean (1, L) float32, noisy (1, L) float32, (min, max) of the value range = (-1, 1),
    (clean path, noisy path))``."""

    def __init__(self, root="./", subset="training", crop_length_sec=0, dataset="dns", quantization=None, bits=16):
        super().__init__()
        assert subset is None or subset in ["training", "testing"]
        self.crop_length_sec = crop_length_sec
        self.subset = subset
        self.bits = bits
        self.create_quantizer(quantization)

        train_clean, train_noisy = os.path.join(root, "training_set/clean"), os.path.join(root, "training_set/noisy")
        if dataset == "VCTK-DEMAND":
            names = self._counted(train_clean, train_noisy)[0]
            self.files = [(os.path.join(train_clean, name), os.path.join(train_noisy, name)) for name in names]
        elif subset == "training":
            count = len(self._counted(train_clean, train_noisy)[0])
            self.files = [(os.path.join(train_clean, f"fileid_{i}.wav"), os.path.join(train_noisy, f"fileid_{i}.wav"))
                          for i in range(count)]
        elif subset == "testing":
            # the DNS test names end in "..._snr{S}_fileid_{i}.wav" / "clean_fileid_{i}.wav": the pair shares the last two
            # underscore-separated fields
            def sortkey(name):
                return "_".join(name.split("_")[-2:])
            base = os.path.join(root, "datasets/test_set/synthetic/no_reverb")
            clean_names, noisy_names = self._counted(os.path.join(base, "clean"), os.path.join(base, "noisy"))
            clean_names.sort(key=sortkey)
            noisy_names.sort(key=sortkey)
            self.files = []
            for c, n in zip(clean_names, noisy_names):
                assert sortkey(c) == sortkey(n), f"unpaired test files {c} / {n}"
                self.files.append((os.path.join(base, "clean", c), os.path.join(base, "noisy", n)))
            self.crop_length_sec = 0
        else:
            raise NotImplementedError
        self._info = {}

    @staticmethod
    def _counted(clean_dir, noisy_dir):
        clean_names, noisy_names = os.listdir(clean_dir), os.listdir(noisy_dir)
        assert len(clean_names) == len(noisy_names), \
            f"{len(clean_names)} files in {clean_dir}, {len(noisy_names)} in {noisy_dir}"
        assert len(clean_names) > 0, f"Number of dataset files: {len(clean_names)}"
        return clean_names, noisy_names

    # ---- quantization: the reference keeps the hooks and implements none of the modes (src/util/dataset.py:78-106)
    def enable_quantization(self, quantization, bits):
        self.create_quantizer("linear")
        self.bits = bits

    def disable_quantization(self):
        self.create_quantizer(None)
        self.bits = 16

    def dequantize(self, x):
        return self.dequantizer(x, self.bits)

    def create_quantizer(self, quantization):
        if quantization in ("linear", "mu-law"):
            raise NotImplementedError(f"quantization {quantization!r}")
        if quantization is not None:
            raise ValueError("Invalid quantization type")
        self.quantizer = self.dequantizer = _identity
        self.qtype = torch.float

    # ---- headers
    def pair_info(self, n):
        """(WavInfo of the clean file, WavInfo of the noisy file), parsed once.  A pair of unequal lengths is an
        AssertionError naming both files, as in ``__getitem__`` of the reference."""
        pair = self._info.get(n)
        if pair is None:
            clean_path, noisy_path = self.files[n]
            pair = (read_wav_info(clean_path), read_wav_info(noisy_path))
            assert pair[0].frames == pair[1].frames, \
                f"Length mismatch in {self.files[n]}, {pair[0].frames} vs {pair[1].frames}"
            self._info[n] = pair
        return pair

    def pair_length(self, n):
        """Samples per channel of pair n, from the headers."""
        return self.pair_info(n)[0].frames

    def pair_rate(self, n):
        """Sample rate of pair n, from the headers.  A pair whose files disagree is an AssertionError naming both."""
        clean, noisy = self.pair_info(n)
        assert clean.rate == noisy.rate, f"Sample rate mismatch in {self.files[n]}, {clean.rate} vs {noisy.rate}"
        return clean.rate

    def read_pcm(self, n, start, count, out=None):
        """Samples [start, start + count) of both files of pair n as two int16 arrays, reading nothing else.  ``out``: a
        pair of writable int16 arrays of at least ``count`` elements to read into (pinned staging rows)."""
        infos = self.pair_info(n)
        for info in infos:
            if not info.is_pcm16_mono:
                raise ValueError(f"{info.path}: read_pcm takes 16-bit mono PCM, this file is {info.describe()}")
        start, count = int(start), int(count)
        if start < 0 or count < 0 or start + count > infos[0].frames:
            raise ValueError(f"{infos[0].path}: samples [{start}, {start + count}) are outside the clip's "
                             f"{infos[0].frames}")
        outs = out if out is not None else (None, None)
        return tuple(_read_range_int16(info, start, count, o) for info, o in zip(infos, outs))

    # ---- the reference's element
    def __getitem__(self, n):
        fileid = self.files[n]
        infos = self.pair_info(n)
        length, rate = infos[0].frames, infos[0].rate
        whole = None
        if not all(info.is_pcm16_mono for info in infos):
            whole = [_read_whole_float(path)[1] for path in fileid]
            assert len(whole[0]) == len(whole[1]), f"Length mismatch in {fileid}, {len(whole[0])} vs {len(whole[1])}"
            length = len(whole[0])

        # src/util/dataset.py:115-134: a clip shorter than the crop is repeated to fill it; a training clip gives one
        # random window (one draw from numpy's global generator, also when the window is the whole clip); else everything
        crop_length = int(self.crop_length_sec * rate)
        start, count, tile = 0, length, False
        if crop_length > length:
            tile = True
        elif self.subset != "testing" and crop_length > 0:
            start, count = int(np.random.randint(low=0, high=length - crop_length + 1)), crop_length

        if whole is None:
            pair = [x.astype(np.float32) * np.float32(PCM_SCALE) for x in self.read_pcm(n, start, count)]
        else:
            pair = [x[start:start + count] for x in whole]
        if tile:
            reps, rest = divmod(crop_length, length)
            pair = [np.concatenate([x] * reps + [x[:rest]]) for x in pair]
        clean_audio, noisy_audio = (torch.from_numpy(np.ascontiguousarray(x)).unsqueeze(0) for x in pair)
        noisy_audio = self.quantizer(noisy_audio, self.bits)
        return clean_audio, noisy_audio, (-1, 1), fileid

    def __len__(self):
        return len(self.files)


class SpeechNoiseDataset:
    """Two unpaired corpora, as the DNS challenge distributes them: every ``*.wav`` below ``speech_root`` and every one
    below ``noise_root``, each list sorted by relative path (so the order does not depend on the file system).  Only
    16-bit mono PCM at ``sample_rate`` is taken: any other encoding or rate, an empty file or an empty root is a
    ValueError here, naming the file and what it is.  There is no element access: training/feeder.py pairs speech with
    fresh noise every epoch and training/mix.py (csrc/mix.hip) mixes them on the device.

    ``len(ds)``: speech files;  ``n_noise``;  ``speech_files`` / ``noise_files``: the paths;  ``speech_length(i)``,
    ``noise_length(j)``: samples, from the headers;  ``read_speech(i, start, count, out=None)``,
    ``read_noise(j, start, count, out=None)``: that range as int16, reading nothing else (``out``: a writable int16
    array of at least ``count`` elements to read into, e.g. a pinned staging row)."""

    def __init__(self, speech_root, noise_root, crop_length_sec=10, sample_rate=16000):
        self.crop_length_sec, self.sample_rate = crop_length_sec, int(sample_rate)
        self._speech = self._scan(os.fspath(speech_root), "speech_root")
        self._noise = self._scan(os.fspath(noise_root), "noise_root")
        self.speech_files = [info.path for info in self._speech]
        self.noise_files = [info.path for info in self._noise]

    def _scan(self, root, what):
        names = sorted((os.path.relpath(os.path.join(d, f), root) for d, _, files in os.walk(root) for f in files
                        if f.lower().endswith(".wav")), key=lambda name: name.split(os.sep))
        if not names:
            raise ValueError(f"SpeechNoiseDataset: no *.wav file below {what} {root}")
        infos = []
        for name in names:
            info = read_wav_info(os.path.join(root, name))
            if not info.is_pcm16_mono:
                raise ValueError(f"SpeechNoiseDataset: {info.path} is {info.describe()}; only 16-bit mono PCM is taken")
            if info.rate != self.sample_rate:
                raise ValueError(f"SpeechNoiseDataset: {info.path} is at {info.rate} Hz, not {self.sample_rate} "
                                 "(other rates are not converted here)")
            if info.frames < 1:
                raise ValueError(f"SpeechNoiseDataset: {info.path} is empty")
            infos.append(info)
        return infos

    def __len__(self):
        return len(self._speech)

    @property
    def n_noise(self):
        return len(self._noise)

    def speech_length(self, i):
        return self._speech[i].frames

    def noise_length(self, j):
        return self._noise[j].frames

    @staticmethod
    def _read(info, start, count, out):
        start, count = int(start), int(count)
        if start < 0 or count < 0 or start + count > info.frames:
            raise ValueError(f"{info.path}: samples [{start}, {start + count}) are outside the file's {info.frames}")
        return _read_range_int16(info, start, count, out)

    def read_speech(self, i, start, count, out=None):
        return self._read(self._speech[i], start, count, out)

    def read_noise(self, j, start, count, out=None):
        return self._read(self._noise[j], start, count, out)


def load_CleanNoisyPairDataset(root="./", subset="training", dataset="dns", crop_length_sec=10, batch_size=1,
                               quantization=None, bits=32, sample_rate=16000, shuffle=True, num_gpus=1, num_workers=0):
    """The reference's DataLoader over the dataset (src/util/dataset.py:156-184): a DistributedSampler for several
    GPUs, shuffling otherwise, nothing pinned, the last partial batch kept.  This is the drop-in route; the train step's
    fast one is training/feeder.py."""
    pairs = CleanNoisyPairDataset(root=root, subset=subset, crop_length_sec=crop_length_sec, dataset=dataset,
                                  quantization=quantization, bits=bits)
    kwargs = {"batch_size": batch_size, "num_workers": num_workers, "pin_memory": False, "drop_last": False}
    if num_gpus > 1:
        return DataLoader(pairs, sampler=DistributedSampler(pairs), **kwargs)
    return DataLoader(pairs, sampler=None, shuffle=shuffle, **kwargs)


class NosyOnlyDataset(Dataset):
    """Noisy recordings of one folder, with the interface of the reference's class of the same (misspelt) name
    (src/util/dataset.py:187-208).  Element n: ``(noisy (L,) float32, the same tensor, (-1, 1), file name)``: channel 0 of
    the file, scaled to [-1, 1) as torchaudio.load scales it.  The files are read by this module's RIFF reader (16-bit mono
    PCM) or scipy (everything else), not torchaudio; their order is the sorted directory listing, where the reference
    keeps the order ``os.listdir`` happens to return.  ``info(n)`` and ``read_pcm(n, out)`` expose the header and the raw
    int16 samples: the route of examples/denoise.py, which leaves scaling to the device (csrc/ragged.hip)."""

    def __init__(self, folder='./'):
        super().__init__()
        self.folder = folder
        self.noisy_files = sorted(os.listdir(folder))
        self.crop_length_sec = 0
        self._info = {}

    def info(self, n):
        """WavInfo of file n, parsed once."""
        info = self._info.get(n)
        if info is None:
            info = self._info[n] = read_wav_info(os.path.join(self.folder, self.noisy_files[n]))
        return info

    def read_pcm(self, n, out=None):
        """Channel 0 of file n as int16: straight from the file for 16-bit mono PCM (into ``out`` if given, e.g. a row of a
        pinned staging tensor); other 16-bit PCM layouts through scipy.  Other encodings raise ValueError."""
        info = self.info(n)
        if info.is_pcm16_mono:
            return _read_range_int16(info, 0, info.frames, out)
        if info.tag != WAVE_FORMAT_PCM or info.bits != 16:
            raise ValueError(f"{info.path}: read_pcm takes 16-bit PCM, this file is {info.describe()}")
        from scipy.io import wavfile
        x = wavfile.read(info.path)[1]
        x = np.ascontiguousarray(x[:, 0] if x.ndim == 2 else x)
        if out is None:
            return x
        out[:len(x)] = x
        return out[:len(x)]

    def __getitem__(self, n):
        fileid = self.noisy_files[n]
        info = self.info(n)
        if info.is_pcm16_mono:
            x = _read_range_int16(info, 0, info.frames).astype(np.float32) * np.float32(PCM_SCALE)
        else:
            x = _read_whole_float(info.path)[1]
        noisy_audio = torch.from_numpy(np.ascontiguousarray(x))
        return noisy_audio, noisy_audio, (-1, 1), fileid

    def __len__(self):
        return len(self.noisy_files)


def load_NoisyDataset(folder, batch_size, sample_rate, num_gpus=1):
    """The reference's DataLoader over a folder of noisy files (src/util/dataset.py:211-224): a DistributedSampler for
    several GPUs, shuffling otherwise.  ``sample_rate`` is accepted and not used, as in the reference."""
    dataset = NosyOnlyDataset(folder=folder)
    kwargs = {"batch_size": batch_size, "num_workers": 0, "pin_memory": False, "drop_last": False}
    if num_gpus > 1:
        return DataLoader(dataset, sampler=DistributedSampler(dataset), **kwargs)
    return DataLoader(dataset, sampler=None, shuffle=True, **kwargs)
