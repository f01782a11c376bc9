"""util/dataset.py on the host: the reference's pairing, crop and tiling rules, and the RIFF reader's ranges.

The reference's src/util/dataset.py cannot be imported where these tests run (it imports torchaudio and torchvision), so
its semantics are restated here from its lines: the file lists of :51-76, the quantizer modes of :89-106, and the crop of
:115-134 --

    crop_length = int(crop_length_sec * sample_rate)
    crop_length > length            -> the clip crop_length // length times, then its first crop_length % length samples
    training and crop_length > 0    -> start = np.random.randint(low=0, high=length - crop_length + 1); [start, start + crop)
    otherwise                       -> the whole clip

with int16 scaled by 1 / 32768 (what torchaudio.load returns for 16-bit PCM)."""
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import wavtree
from cleanumamba_amd.util.dataset import CleanNoisyPairDataset, load_CleanNoisyPairDataset, read_wav_info

RATE = 16000


def _f32(x):
    return torch.from_numpy(x.astype(np.float32) / np.float32(32768.0))


def test_training_layout_pairs_by_index(tmp_path):
    pairs = wavtree.training_tree(str(tmp_path), [900] * 11)
    ds = CleanNoisyPairDataset(root=str(tmp_path), subset="training", crop_length_sec=0)
    assert len(ds) == 11
    # by number, not by directory order: fileid_10 comes after fileid_9
    assert [os.path.basename(c) for c, _ in ds.files] == [f"fileid_{i}.wav" for i in range(11)]
    for i, (c, n) in enumerate(ds.files):
        assert c == os.path.join(str(tmp_path), "training_set/clean", f"fileid_{i}.wav")
        assert n == os.path.join(str(tmp_path), "training_set/noisy", f"fileid_{i}.wav")
    clean, noisy, rng, fileid = ds[10]
    assert clean.dtype == noisy.dtype == torch.float32 and clean.shape == noisy.shape == (1, 900)
    assert torch.equal(clean[0], _f32(pairs[10][0])) and torch.equal(noisy[0], _f32(pairs[10][1]))
    assert rng == (-1, 1) and tuple(fileid) == tuple(ds.files[10])


def test_vctk_layout_pairs_by_name(tmp_path):
    names = ["p232_001.wav", "p257_413.wav", "p232_010.wav"]
    for sub in ("clean", "noisy"):
        os.makedirs(tmp_path / "training_set" / sub)
    for k, name in enumerate(names):
        wavfile.write(tmp_path / "training_set/clean" / name, RATE, wavtree.pcm(300 + k, k))
        wavfile.write(tmp_path / "training_set/noisy" / name, RATE, wavtree.pcm(300 + k, 50 + k))
    ds = CleanNoisyPairDataset(root=str(tmp_path), subset="training", dataset="VCTK-DEMAND")
    assert sorted(os.path.basename(c) for c, _ in ds.files) == sorted(names)
    for c, n in ds.files:
        assert os.path.basename(c) == os.path.basename(n)
        assert c.startswith(os.path.join(str(tmp_path), "training_set/clean"))
        assert n.startswith(os.path.join(str(tmp_path), "training_set/noisy"))


def test_testing_layout_sort_key_and_no_crop(tmp_path):
    base = tmp_path / "datasets/test_set/synthetic/no_reverb"
    for sub in ("clean", "noisy"):
        os.makedirs(base / sub)
    ids = [10, 2, 33, 1]
    data = {}
    for k, i in enumerate(ids):
        # the noisy names carry more fields in front; the pair shares "fileid_{i}.wav"
        data[i] = (wavtree.pcm(500 + 7 * k, i), wavtree.pcm(500 + 7 * k, 100 + i))
        wavfile.write(base / "clean" / f"clean_fileid_{i}.wav", RATE, data[i][0])
        wavfile.write(base / "noisy" / f"book_{k}_door_snr{k}_fileid_{i}.wav", RATE, data[i][1])
    np.random.seed(0)
    before = np.random.get_state()[1].copy()
    ds = CleanNoisyPairDataset(root=str(tmp_path), subset="testing", crop_length_sec=0.01)
    assert ds.crop_length_sec == 0                      # forced
    order = sorted(ids, key=lambda i: f"fileid_{i}.wav")            # a string sort: 1, 10, 2, 33
    assert order == [1, 10, 2, 33]
    assert [os.path.basename(c) for c, _ in ds.files] == [f"clean_fileid_{i}.wav" for i in order]
    for (c, n), i in zip(ds.files, order):
        assert n.endswith(f"_fileid_{i}.wav")
    for k, i in enumerate(order):
        clean, noisy, _, _ = ds[k]
        assert torch.equal(clean[0], _f32(data[i][0])) and torch.equal(noisy[0], _f32(data[i][1]))     # uncropped
    assert np.array_equal(np.random.get_state()[1], before)          # and no draw


def test_file_count_assertions(tmp_path):
    for sub in ("clean", "noisy"):
        os.makedirs(tmp_path / "training_set" / sub)
    with pytest.raises(AssertionError):
        CleanNoisyPairDataset(root=str(tmp_path), subset="training")            # empty
    wavfile.write(tmp_path / "training_set/clean/fileid_0.wav", RATE, wavtree.pcm(10, 0))
    with pytest.raises(AssertionError):
        CleanNoisyPairDataset(root=str(tmp_path), subset="training")            # 1 clean, 0 noisy


@pytest.mark.parametrize("seed", [0, 1, 7])
def test_random_crop_is_the_references_single_draw(tmp_path, seed):
    pairs = wavtree.training_tree(str(tmp_path), [5000, 1600, 2311])
    ds = CleanNoisyPairDataset(root=str(tmp_path), subset="training", crop_length_sec=0.1)
    crop = int(0.1 * RATE)
    assert crop == 1600
    for n, (c, z) in enumerate(pairs):
        np.random.seed(seed)
        start = np.random.randint(low=0, high=len(c) - crop + 1)        # the restated rule (also for crop == length)
        after_one = np.random.randint(0, 1 << 30)
        np.random.seed(seed)
        clean, noisy, _, _ = ds[n]
        assert np.random.randint(0, 1 << 30) == after_one               # exactly one draw was consumed
        assert clean.shape == (1, crop)
        assert torch.equal(clean[0], _f32(c[start:start + crop])) and torch.equal(noisy[0], _f32(z[start:start + crop]))


def test_short_clip_is_tiled_without_a_draw(tmp_path):
    (c, z), = wavtree.training_tree(str(tmp_path), [700])
    ds = CleanNoisyPairDataset(root=str(tmp_path), subset="training", crop_length_sec=0.1)
    np.random.seed(3)
    after_none = np.random.randint(0, 1 << 30)
    np.random.seed(3)
    clean, noisy, _, _ = ds[0]
    assert np.random.randint(0, 1 << 30) == after_none
    assert clean.shape == noisy.shape == (1, 1600)
    for got, src in ((clean, c), (noisy, z)):
        assert torch.equal(got[0], _f32(np.concatenate([src, src, src[:200]])))     # 1600 // 700 = 2, 1600 % 700 = 200


HEADERS = {
    "plain": {},
    "list_before_data": dict(chunks=[(b"LIST", b"INFOISFT\x04\0\0\0abc\0")]),
    "odd_sized_chunk": dict(chunks=[(b"junk", b"12345")]),
    "extensible": dict(extensible=True),
    "data_size_0": dict(data_size=0),
    "data_size_ffffffff": dict(data_size=0xFFFFFFFF),
}


@pytest.mark.parametrize("case", list(HEADERS))
def test_read_pcm_ranges(tmp_path, case):
    """read_pcm(n, start, count) == scipy.io.wavfile.read(...)[start:start + count] == the samples that were written.
    (scipy itself reads a file whose ``data`` size is 0 as empty -- measured with scipy 1.15 -- so that case is held
    to the written samples alone, which is what scipy returns for every other header here.)"""
    for sub in ("clean", "noisy"):
        os.makedirs(tmp_path / "training_set" / sub)
    written = (wavtree.pcm(1001, 1), wavtree.pcm(1001, 2))
    paths = [str(tmp_path / "training_set" / sub / "fileid_0.wav") for sub in ("clean", "noisy")]
    for p, x in zip(paths, written):
        wavtree.write_raw(p, x, **HEADERS[case])
    if case != "data_size_0":
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                 # scipy warns about chunks it skips
            for p, x in zip(paths, written):
                rate, y = wavfile.read(p)
                assert rate == RATE and np.array_equal(y, x)
    ds = CleanNoisyPairDataset(root=str(tmp_path), subset="training")
    assert ds.pair_length(0) == 1001
    assert read_wav_info(paths[0]).rate == RATE
    for start, count in [(0, 1001), (0, 1), (1000, 1), (313, 500), (17, 0)]:
        got = ds.read_pcm(0, start, count)
        assert len(got) == 2
        for g, x in zip(got, written):
            assert g.dtype == np.int16 and np.array_equal(g, x[start:start + count])
    out = (np.full(640, 7, np.int16), np.full(640, 7, np.int16))
    ds.read_pcm(0, 400, 600, out=out)                       # into caller's rows: only [0, count) is written
    for o, x in zip(out, written):
        assert np.array_equal(o[:600], x[400:1000]) and (o[600:] == 7).all()
    for start, count in [(-1, 2), (1000, 2), (0, 1002)]:
        with pytest.raises(ValueError):
            ds.read_pcm(0, start, count)
    clean, noisy, _, _ = ds[0]                              # and the element reads through the same header
    assert torch.equal(clean[0], _f32(written[0])) and torch.equal(noisy[0], _f32(written[1]))


def test_float32_file_works_in_getitem_and_is_refused_by_read_pcm(tmp_path):
    for sub in ("clean", "noisy"):
        os.makedirs(tmp_path / "training_set" / sub)
    rng = np.random.default_rng(0)
    c, z = (rng.uniform(-1, 1, 2000).astype(np.float32) for _ in range(2))
    wavfile.write(tmp_path / "training_set/clean/fileid_0.wav", RATE, c)
    wavfile.write(tmp_path / "training_set/noisy/fileid_0.wav", RATE, z)
    ds = CleanNoisyPairDataset(root=str(tmp_path), subset="training", crop_length_sec=0.05)
    assert ds.pair_length(0) == 2000
    np.random.seed(5)
    start = np.random.randint(low=0, high=2000 - 800 + 1)
    np.random.seed(5)
    clean, noisy, _, _ = ds[0]
    assert torch.equal(clean[0], torch.from_numpy(c[start:start + 800]))
    assert torch.equal(noisy[0], torch.from_numpy(z[start:start + 800]))
    with pytest.raises(ValueError) as e:
        ds.read_pcm(0, 0, 10)
    assert "fileid_0.wav" in str(e.value) and "float" in str(e.value) and "32" in str(e.value)


def test_unequal_pair_raises_naming_the_files(tmp_path):
    for sub in ("clean", "noisy"):
        os.makedirs(tmp_path / "training_set" / sub)
    wavfile.write(tmp_path / "training_set/clean/fileid_0.wav", RATE, wavtree.pcm(1000, 0))
    wavfile.write(tmp_path / "training_set/noisy/fileid_0.wav", RATE, wavtree.pcm(999, 1))
    ds = CleanNoisyPairDataset(root=str(tmp_path), subset="training")
    with pytest.raises(AssertionError) as e:
        ds[0]
    assert "training_set/clean/fileid_0.wav" in str(e.value) and "training_set/noisy/fileid_0.wav" in str(e.value)
    assert "1000" in str(e.value) and "999" in str(e.value)
    with pytest.raises(AssertionError):
        ds.pair_length(0)


def test_quantization_modes(tmp_path):
    wavtree.training_tree(str(tmp_path), [100])
    for mode in ("linear", "mu-law"):
        with pytest.raises(NotImplementedError):
            CleanNoisyPairDataset(root=str(tmp_path), quantization=mode)
    with pytest.raises(ValueError):
        CleanNoisyPairDataset(root=str(tmp_path), quantization="a-law")
    ds = CleanNoisyPairDataset(root=str(tmp_path), quantization=None)
    assert ds.qtype is torch.float and ds.bits == 16
    x = torch.ones(3)
    assert ds.dequantize(x) is x
    with pytest.raises(NotImplementedError):
        ds.enable_quantization("linear", 8)


def test_loader_is_the_references_dataloader(tmp_path):
    pairs = wavtree.training_tree(str(tmp_path), [2000] * 5)
    loader = load_CleanNoisyPairDataset(root=str(tmp_path), subset="training", crop_length_sec=0.05, batch_size=2,
                                        shuffle=False, num_gpus=1, num_workers=0)
    assert isinstance(loader, torch.utils.data.DataLoader) and not loader.drop_last and not loader.pin_memory
    assert isinstance(loader.sampler, torch.utils.data.SequentialSampler)
    shapes, seen = [], []
    np.random.seed(11)
    for clean, noisy, _, fileid in loader:                  # the reference's loop unpacks four
        shapes.append(tuple(clean.shape))
        seen += list(fileid[0])
        assert clean.dtype == torch.float32 and noisy.shape == clean.shape
    assert shapes == [(2, 1, 800), (2, 1, 800), (1, 1, 800)]             # the last partial batch is kept
    assert [os.path.basename(p) for p in seen] == [f"fileid_{i}.wav" for i in range(5)]
    np.random.seed(11)
    starts = [np.random.randint(low=0, high=2000 - 800 + 1) for _ in range(5)]
    np.random.seed(11)
    first = next(iter(loader))[0]
    assert torch.equal(first[1, 0], _f32(pairs[1][0][starts[1]:starts[1] + 800]))
    shuffled = load_CleanNoisyPairDataset(root=str(tmp_path), batch_size=2)
    assert isinstance(shuffled.sampler, torch.utils.data.RandomSampler)
    assert shuffled.dataset.crop_length_sec == 10
