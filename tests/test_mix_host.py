"""Training from separate speech and noise corpora, on the host: ``SpeechNoiseDataset`` (listing order, refusals), the
feeder's plan (a pure function of seed, epoch, rank and the files), the layout of a noise row, ``Mix`` / ``MixDraws``
validation, CPU ``mix.apply`` against mix_ref.py bit for bit, the CPU feeder end to end, and the argument checks of
cum_mix_pairs, which run before any launch and therefore without a GPU."""
import os
import struct

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import mix_ref as R
import mixcases
import wavtree
from cleanumamba_amd.training import augment as A
from cleanumamba_amd.training import mix as M
from cleanumamba_amd.training.feeder import BatchFeeder
from cleanumamba_amd.util.dataset import CleanNoisyPairDataset, SpeechNoiseDataset

CROP = 1000
MIX = dict(snr_db=(-5.0, 20.0), level_db=(-35.0, -15.0), frame=160, gap=50, max_pieces=3)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return mixcases.mix_tree(str(tmp_path_factory.mktemp("unpaired")), seed=300)


def _dataset(tree):
    return SpeechNoiseDataset(tree[0], tree[1], crop_length_sec=CROP / 16000)


# ---------------------------------------------------------------------------------------------------------------- dataset
def test_listing_is_sorted_by_relative_path_and_reads_ranges(tree):
    speech_root, noise_root, speech, noise = tree
    ds = _dataset(tree)
    assert len(ds) == len(mixcases.SPEECH) and ds.n_noise == len(mixcases.NOISE)
    assert [os.path.relpath(p, speech_root).replace(os.sep, "/") for p in ds.speech_files] \
        == mixcases.sorted_names(mixcases.SPEECH)
    assert [os.path.relpath(p, noise_root).replace(os.sep, "/") for p in ds.noise_files] \
        == mixcases.sorted_names(mixcases.NOISE)
    for i, x in enumerate(speech):
        assert ds.speech_length(i) == len(x)
        got = ds.read_speech(i, 5, len(x) - 9)
        assert got.dtype == np.int16 and np.array_equal(got, x[5:len(x) - 4])
    out = np.full(50, 77, np.int16)
    for j, x in enumerate(noise):
        assert ds.noise_length(j) == len(x)
        got = ds.read_noise(j, len(x) - 30, 30, out=out)
        assert np.array_equal(got, x[-30:]) and np.array_equal(out[:30], x[-30:]) and (out[30:] == 77).all()
    with pytest.raises(ValueError, match="outside"):
        ds.read_speech(0, 0, ds.speech_length(0) + 1)
    with pytest.raises(ValueError, match="outside"):
        ds.read_noise(1, -1, 5)


def _one_file_roots(tmp_path, write):
    """A good speech root and a noise root whose one file comes from ``write(path)``."""
    speech, noise = tmp_path / "speech", tmp_path / "noise" / "sub"
    speech.mkdir()
    noise.mkdir(parents=True)
    wavfile.write(str(speech / "ok.wav"), 16000, wavtree.pcm(100, 1))
    path = str(noise / "odd.wav")
    write(path)
    return str(speech), str(tmp_path / "noise"), path


@pytest.mark.parametrize("case,text", [("48k", "48000 Hz"), ("stereo", "2 channel"), ("float", "IEEE float"),
                                       ("empty", "is empty")])
def test_refused_files_are_named(tmp_path, case, text):
    writers = {
        "48k": lambda p: wavfile.write(p, 48000, wavtree.pcm(100, 2)),
        "stereo": lambda p: wavfile.write(p, 16000, np.stack([wavtree.pcm(100, 2), wavtree.pcm(100, 3)], axis=1)),
        "float": lambda p: wavfile.write(p, 16000, np.linspace(-1, 1, 100).astype(np.float32)),
        "empty": lambda p: wavtree.write_raw(p, np.zeros(0, np.int16)),
    }
    speech, noise, path = _one_file_roots(tmp_path, writers[case])
    with pytest.raises(ValueError) as err:
        SpeechNoiseDataset(speech, noise)
    assert path in str(err.value) and text in str(err.value)
    with pytest.raises(ValueError) as err:                   # the same file among the speech
        SpeechNoiseDataset(noise, speech)
    assert path in str(err.value)


def test_an_empty_root_is_refused(tmp_path):
    speech, noise, _ = _one_file_roots(tmp_path, lambda p: wavfile.write(p, 16000, wavtree.pcm(100, 2)))
    empty = tmp_path / "nothing" / "here"
    empty.mkdir(parents=True)
    (empty / "notes.txt").write_text("no audio")
    for roots in ((speech, str(tmp_path / "nothing")), (str(tmp_path / "nothing"), noise)):
        with pytest.raises(ValueError) as err:
            SpeechNoiseDataset(*roots)
        assert str(tmp_path / "nothing") in str(err.value)


# ---------------------------------------------------------------------------------------------------------------- config
def test_mix_and_draws_validation():
    assert M.Mix(snr_db=5, level_db=-20).snr_db == (5.0, 5.0)
    assert M.Mix(level_db=None).level_db is None
    for bad in (dict(snr_db=(3, 1)), dict(level_db=(-10, -20)), dict(snr_db=(0, float("inf"))), dict(snr_db=float("nan")),
                dict(snr_db=None), dict(activity_db=float("nan")), dict(frame=0), dict(clip=0.0), dict(clip=1.01),
                dict(clip=float("nan")), dict(gap=-1), dict(max_pieces=0)):
        with pytest.raises(ValueError):
            M.Mix(**bad)
    M.Mix(clip=1.0, gap=0, max_pieces=1, frame=1)
    for bad in (dict(snr_db=[1.0], level_db=[1.0, 2.0]), dict(snr_db=[], level_db=[]),
                dict(snr_db=[float("nan")], level_db=[0.0]), dict(snr_db=[0.0], level_db=[float("inf")]),
                dict(snr_db=[0.0], level_db=[0.0], frame=0), dict(snr_db=[0.0], level_db=[0.0], clip=2.0)):
        with pytest.raises(ValueError):
            M.MixDraws(**bad)
    d = M.MixDraws([3.0, -20.0], [float("nan"), -1.0], activity_db=-50.0, frame=37, clip=0.5)
    with pytest.raises(ValueError):
        d.pack([5])
    with pytest.raises(ValueError):
        d.pack([5, 0])
    recs = d.pack([5, 900]).reshape(2, M.REC_INTS)
    assert recs.dtype == np.int32 and recs[:, 0].tolist() == [5, 900] and recs[:, 1].tolist() == [37, 37]
    assert (recs[:, 9:] == 0).all()
    for b in range(2):
        thr, q, l = struct.unpack("<qdd", recs[b, 2:8].tobytes())
        want_q, want_l, want_thr = R.scalars(d.snr_db[b], d.level_db[b], -50.0)
        assert thr == want_thr == 10737 and q == want_q and (l == want_l or (np.isnan(l) and np.isnan(want_l)))
        assert struct.unpack("<f", recs[b, 8:9].tobytes())[0] == 0.5


def test_draw_is_a_pure_function_of_its_generator():
    mix = M.Mix(**MIX)
    a, b, c = (mix.draw(np.random.default_rng(s), 6) for s in (5, 5, 6))
    assert np.array_equal(a.snr_db, b.snr_db) and np.array_equal(a.level_db, b.level_db)
    assert not np.array_equal(a.snr_db, c.snr_db)
    assert a.batch == 6 and a.frame == 160 and a.clip == 0.99 and a.activity_db == -50.0
    assert (a.snr_db >= -5).all() and (a.snr_db <= 20).all() and (a.level_db >= -35).all() and (a.level_db <= -15).all()
    assert np.isnan(M.Mix(level_db=None).draw(np.random.default_rng(1), 3).level_db).all()


# ---------------------------------------------------------------------------------------------------------------- apply
def _rows(seed, nb, L):
    rng = np.random.default_rng(seed)
    speech = rng.integers(-3000, 3000, (nb, L)).astype(np.int16)
    noise = rng.integers(-32768, 32768, (nb, L)).astype(np.int16)
    speech[:, L // 2:] //= 50                                   # a quiet second half (about -59 dBFS): inactive frames
    return speech, noise


@pytest.mark.parametrize("L,frame", [(1, 1600), (7, 37), (1599, 1600), (1601, 1600), (3205, 37)])
def test_cpu_apply_equals_the_reference_bit_for_bit(L, frame):
    nb = 4
    speech, noise = _rows(L, nb, L)
    noise[1] = 0                                                # all-zero noise: a = 1
    speech[2] = 0                                               # all-zero speech
    n_speech = [L, max(1, L // 3), L, max(1, L - 1)]
    draws = M.MixDraws([5.0, 0.0, 10.0, -20.0], [-25.0, -20.0, float("nan"), -1.0], frame=frame)
    clean, noisy, stats = M.apply(torch.from_numpy(speech), n_speech, torch.from_numpy(noise), draws)
    want = R.mix_batch(speech, n_speech, noise, draws.snr_db, draws.level_db, frame=frame)
    assert clean.dtype == noisy.dtype == stats.dtype == torch.float32
    assert clean.shape == noisy.shape == (nb, L) and stats.shape == (nb, 8)
    for got, ref in zip((clean, noisy, stats), want[:3]):
        assert np.array_equal(got.numpy().view(np.int32), ref.view(np.int32))
    if L > 7:
        assert want[3][3]["guard"] and not want[3][0]["guard"]          # both sides of the guard were taken
        assert stats[3, 7] == 1 and stats[0, 7] == 0
        assert np.abs(noisy[3].numpy()).max() <= np.float32(0.99) * (1 + 2.0 ** -22)


def test_cpu_apply_writes_into_given_tensors_and_checks_them():
    nb, L = 3, 50
    speech, noise = (torch.from_numpy(x) for x in _rows(1, nb, L))
    draws = M.MixDraws([5.0] * nb, [-25.0] * nb, frame=16)
    want = M.apply(speech, [L] * nb, noise, draws)
    clean, noisy, stats = torch.full((nb, L + 3), 7.0), torch.full((nb, 1, L), 7.0), torch.zeros(nb, 8)
    got = M.apply(speech, [L] * nb, noise, draws, clean[:, :L], noisy, stats)
    assert got[0].data_ptr() == clean.data_ptr() and got[1] is noisy and got[2] is stats
    assert torch.equal(clean[:, :L], want[0]) and torch.equal(noisy[:, 0], want[1]) and torch.equal(stats, want[2])
    assert (clean[:, L:] == 7).all()
    both = torch.zeros(nb, 2 * L)
    for bad in (dict(clean_out=both[:, :L], noisy_out=both[:, L - 1:2 * L - 1]),       # overlapping
                dict(clean_out=torch.zeros(nb, L + 1)), dict(noisy_out=torch.zeros(nb - 1, L)),
                dict(clean_out=torch.zeros(nb, L, dtype=torch.float64)), dict(stats_out=torch.zeros(nb, 4))):
        with pytest.raises(ValueError):
            M.apply(speech, [L] * nb, noise, draws, **bad)
    with pytest.raises(ValueError):
        M.apply(speech.float(), [L] * nb, noise, draws)
    with pytest.raises(ValueError):
        M.apply(speech, [L] * nb, noise, M.MixDraws([1.0], [1.0]))


def test_argument_errors_of_the_c_abi():
    assert mixcases.argument_errors() == 18


# ---------------------------------------------------------------------------------------------------------------- feeder
def test_feeder_wants_mix_with_unpaired_data_and_only_then(tree, tmp_path):
    ds = _dataset(tree)
    with pytest.raises(ValueError, match="mix="):
        BatchFeeder(ds, 2, "cpu")
    wavtree.training_tree(str(tmp_path), [2000, 2100])
    pairs = CleanNoisyPairDataset(root=str(tmp_path), subset="training", crop_length_sec=CROP / 16000)
    with pytest.raises(ValueError, match="mix="):
        BatchFeeder(pairs, 2, "cpu", mix=M.Mix())
    with pytest.raises(ValueError, match="mix"):
        BatchFeeder(ds, 2, "cpu", mix="yes")
    with pytest.raises(ValueError, match="sample_rate"):
        BatchFeeder(ds, 2, "cpu", mix=M.Mix(), sample_rate=16000)


def test_plan_is_a_function_of_seed_epoch_and_rank_alone(tree):
    ds = _dataset(tree)
    mix = M.Mix(**MIX)
    seen = {}
    for workers in (0, 1, 4):
        with BatchFeeder(ds, 4, "cpu", seed=8, workers=workers, mix=mix) as feeder:
            seen[workers] = [(feeder.plan(e), [feeder.noise_plan(e, k) for k in range(len(feeder))]) for e in range(2)]
            handed = [(b.epoch, b.entries, b.noise, b.mix.snr_db.tolist()) for _ in range(2) for b in feeder]
            assert [h[1] for h in handed] == [b for e in range(2) for b in seen[workers][e][0]]
            assert [h[2] for h in handed] == [n for e in range(2) for n in seen[workers][e][1]]
            assert handed[0][3] == feeder.mix_draws(0, 0).snr_db.tolist() != handed[1][3]
    assert seen[0] == seen[1] == seen[4]
    epoch0, epoch1 = seen[1]
    assert epoch0[0] != epoch1[0] and epoch0[1] != epoch1[1]                     # fresh order, fresh noise every epoch
    with BatchFeeder(ds, 4, "cpu", seed=8, mix=mix) as again:                    # resumed at epoch 1
        assert again.plan(1) == epoch1[0] and again.noise_plan(1, 1) == epoch1[1][1]
    with BatchFeeder(ds, 2, "cpu", seed=8, rank=0, world=2, mix=mix) as r0, \
            BatchFeeder(ds, 2, "cpu", seed=8, rank=1, world=2, mix=mix) as r1:
        files = [{index for b in r.plan(0) for index, _, _ in b} for r in (r0, r1)]
        assert len(files[0]) == len(files[1]) == 4 and not files[0] & files[1]
        assert r0.noise_plan(0, 0) != r1.noise_plan(0, 0)
    # a speech file no longer than the crop is read whole; a longer one gives a window of the crop
    for index, start, count in (e for b in epoch0[0] for e in b):
        n = ds.speech_length(index)
        assert (start, count) == (0, n) if n <= CROP else (count == CROP and 0 <= start <= n - CROP)


def test_noise_row_layout(tree):
    ds = _dataset(tree)
    lengths = [ds.noise_length(j) for j in range(ds.n_noise)]
    assert min(lengths) < 50                                    # a noise file shorter than the gap
    short, exhausted, cut = 0, 0, 0
    with BatchFeeder(ds, 4, "cpu", seed=3, mix=M.Mix(**MIX)) as feeder:
        for e in range(6):
            for k in range(len(feeder)):
                for r, pieces in enumerate(feeder.noise_plan(e, k)):
                    rng = np.random.Generator(np.random.PCG64([3, e, 0, k, r, 0x4E6F69]))
                    assert 1 <= len(pieces) <= 3
                    pos = 0
                    for j, start, count, at in pieces:
                        assert j == int(rng.integers(0, ds.n_noise)) and start == int(rng.integers(0, lengths[j]))
                        assert at == pos < CROP and count == min(lengths[j] - start, CROP - at) >= 1
                        short += lengths[j] < 50
                        cut += start + count < lengths[j]
                        pos = at + count + 50                   # the gap behind every piece
                    full = pieces[-1][3] + pieces[-1][2] + 50 >= CROP
                    assert full or len(pieces) == 3
                    exhausted += not full
    assert short and exhausted and cut                          # every case of the layout was seen


@pytest.mark.parametrize("workers", [0, 1, 4])
def test_cpu_feeder_batches_equal_the_reference_on_the_planned_reads(tree, workers):
    _, _, speech, noise = tree
    ds = _dataset(tree)
    mix = M.Mix(**MIX)
    with BatchFeeder(ds, 4, "cpu", seed=9, workers=workers, mix=mix) as feeder:
        n = 0
        for epoch in range(2):
            for k, batch in enumerate(feeder):
                assert batch.epoch == epoch and batch.shape == (4, 1, CROP)
                assert batch.entries == feeder.plan(epoch)[k] and batch.noise == feeder.noise_plan(epoch, k)
                assert batch.fileids == [ds.speech_files[i] for i, _, _ in batch.entries]
                S, n_speech, N = mixcases.planned_rows(batch.entries, batch.noise, speech, noise, CROP)
                draws = mix.draw(np.random.Generator(np.random.PCG64([9, epoch, 0, k, 0x4D6978])), 4)
                assert np.array_equal(batch.mix.snr_db, draws.snr_db) and np.array_equal(batch.mix.level_db, draws.level_db)
                want = R.mix_batch(S, n_speech, N, draws.snr_db, draws.level_db, frame=160)
                clean, noisy = batch.tensors()
                assert np.array_equal(clean[:, 0].numpy().view(np.int32), want[0].view(np.int32))
                assert np.array_equal(noisy[:, 0].numpy().view(np.int32), want[1].view(np.int32))
                assert np.array_equal(batch.mix_stats().numpy().view(np.int32), want[2].view(np.int32))
                again = torch.full((4, CROP + 3), 7.0), torch.full((4, 1, CROP), 7.0)
                batch.into(again[0][:, :CROP], again[1])
                assert torch.equal(again[0][:, :CROP], clean[:, 0]) and torch.equal(again[1], noisy)
                assert (again[0][:, CROP:] == 7).all()
                n += 1
        assert n == 4


def test_cpu_feeder_with_augment_behind_the_mix(tree):
    _, _, speech, noise = tree
    ds = _dataset(tree)
    mix, shift = M.Mix(**MIX), 37
    aug = A.Augment(shift=shift, gain_db=(-6, 3))
    with BatchFeeder(ds, 4, "cpu", seed=9, mix=mix, augment=aug) as feeder:
        for k, batch in enumerate(feeder):
            assert batch.shape == (4, 1, CROP) and batch.draws.shift == shift
            assert all(count == min(ds.speech_length(i), CROP + shift) for i, _, count in batch.entries)
            S, n_speech, N = mixcases.planned_rows(batch.entries, batch.noise, speech, noise, CROP + shift)
            mixed = M.apply(torch.from_numpy(S), n_speech, torch.from_numpy(N), batch.mix)
            want = A.apply(mixed[0], mixed[1], batch.draws)
            clean, noisy = batch.tensors()
            assert torch.equal(clean[:, 0], want[0]) and torch.equal(noisy[:, 0], want[1])
            assert torch.equal(batch.mix_stats(), mixed[2])
        assert k == 1
