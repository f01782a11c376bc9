"""training/feeder.py on the host: the plan (one scheduler, one generator per epoch), the rank sharding, the CPU mode's
batches against the planned slices, how errors and a stuck dataset surface, and the argument checks of
cum_pcm_batch_f32, which run before any launch and therefore without a GPU."""
import ctypes
import os
import threading
import time

import numpy as np
import pytest
import torch

import wavtree
from cleanumamba_amd.training.feeder import BatchFeeder
from cleanumamba_amd.util.dataset import CleanNoisyPairDataset

LENGTHS = [3000, 9000, 4099, 4100, 5000, 3500, 8000, 4098, 6001, 7000, 3333, 8999]      # some shorter than the crop
CROP = 4099


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("pairs"))
    pairs = wavtree.training_tree(root, LENGTHS, seed=100)
    return root, pairs


def _dataset(root):
    return CleanNoisyPairDataset(root=root, subset="training", crop_length_sec=CROP / 16000)


def expected_batch(pairs, entries, crop):
    """The formula of include/cleanumamba_hip.h for one planned batch: sample t of a clip is sample (t mod count) of its
    planned slice, times 2^-15."""
    out = []
    for k in range(2):
        rows = []
        for index, start, count in entries:
            sl = pairs[index][k][start:start + count]
            rows.append(sl[np.arange(crop) % count].astype(np.float32) * np.float32(2.0 ** -15))
        out.append(torch.from_numpy(np.stack(rows))[:, None, :])
    return out


def test_plan_is_the_schedulers_alone(tree):
    root, _ = tree
    ds = _dataset(root)
    assert BatchFeeder(ds, 4, "cpu").crop_length == CROP            # default: int(crop_length_sec * 16000)
    with BatchFeeder(ds, 4, "cpu", seed=3, workers=1) as one, BatchFeeder(ds, 4, "cpu", seed=3, workers=4) as four, \
            BatchFeeder(ds, 4, "cpu", seed=4) as other:
        for e in range(3):
            assert one.plan(e) == four.plan(e) == one.plan(e)
        assert one.plan(0) != one.plan(1)
        assert one.plan(0) != other.plan(0)
        plan = one.plan(0)
        assert len(plan) == len(one) == 3 and all(len(b) == 4 for b in plan)
        assert sorted(i for b in plan for i, _, _ in b) == list(range(12))
        for b in plan:
            for index, start, count in b:
                n = LENGTHS[index]
                if n <= CROP:
                    assert (start, count) == (0, n)
                else:
                    assert count == CROP and 0 <= start <= n - CROP
        # the crop starts move: not every long clip starts at 0, and they differ between epochs
        starts = [[s for b in one.plan(e) for i, s, _ in sorted(b) if LENGTHS[i] > CROP] for e in range(2)]
        assert any(starts[0]) and starts[0] != starts[1]
    with BatchFeeder(ds, 4, "cpu", shuffle=False) as plain:
        assert [i for b in plain.plan(5) for i, _, _ in b] == list(range(12))


def test_ranks_get_disjoint_equal_shares_and_drop_last(tree):
    root, _ = tree
    ds = _dataset(root)
    with BatchFeeder(ds, 2, "cpu", seed=1, rank=0, world=2) as r0, BatchFeeder(ds, 2, "cpu", seed=1, rank=1, world=2) as r1:
        for e in range(2):
            a = [i for b in r0.plan(e) for i, _, _ in b]
            c = [i for b in r1.plan(e) for i, _, _ in b]
            assert len(a) == len(c) == 6 and not set(a) & set(c) and sorted(a + c) == list(range(12))
    # 12 pairs over 5 ranks: 2 each (the common count), two pairs idle
    shares = []
    for rank in range(5):
        with BatchFeeder(ds, 1, "cpu", seed=1, rank=rank, world=5) as f:
            shares.append([i for b in f.plan(0) for i, _, _ in b])
    assert all(len(s) == 2 for s in shares) and len({i for s in shares for i in s}) == 10
    with BatchFeeder(ds, 5, "cpu", drop_last=True) as f:
        assert len(f) == 2 and [len(b) for b in f.plan(0)] == [5, 5]
    with BatchFeeder(ds, 5, "cpu", drop_last=False) as f:
        assert len(f) == 3 and [len(b) for b in f.plan(0)] == [5, 5, 2]
        sizes = [tuple(batch.tensors()[0].shape) for batch in f]
        assert sizes == [(5, 1, CROP), (5, 1, CROP), (2, 1, CROP)]
    with pytest.raises(ValueError):
        BatchFeeder(ds, 13, "cpu")                      # no whole batch


@pytest.mark.parametrize("workers", [1, 4])
def test_cpu_batches_equal_the_planned_slices(tree, workers):
    root, pairs = tree
    ds = _dataset(root)
    with BatchFeeder(ds, 4, "cpu", crop_length=CROP, seed=9, workers=workers) as feeder:
        for epoch in range(2):
            plan = feeder.plan(epoch)
            assert any(count < CROP for b in plan for _, _, count in b)          # some clips are tiled
            got = 0
            for batch, entries in zip(feeder, plan):
                assert batch.epoch == epoch and batch.entries == entries
                assert batch.fileids == [tuple(ds.files[i]) for i, _, _ in entries]
                clean, noisy = batch.tensors()
                want_clean, want_noisy = expected_batch(pairs, entries, CROP)
                assert clean.dtype == torch.float32 and clean.shape == (4, 1, CROP)
                assert torch.equal(clean, want_clean) and torch.equal(noisy, want_noisy)
                got += 1
            assert got == 3
        assert feeder.epoch == 2


def test_into_writes_views_and_stale_batch_raises(tree):
    root, pairs = tree
    ds = _dataset(root)
    with BatchFeeder(ds, 3, "cpu", crop_length=1000, seed=2, depth=2) as feeder:
        first = feeder.next()
        big = torch.full((3, 2, 1500), 7.0)
        clean, noisy = big[:, 0:1, :1000], big[:, 1:2, 500:]
        first.into(clean, noisy)
        want = expected_batch(pairs, first.entries, 1000)
        assert torch.equal(clean, want[0]) and torch.equal(noisy, want[1])
        assert (big[:, 0, 1000:] == 7).all() and (big[:, 1, :500] == 7).all()
        feeder.next()
        assert torch.equal(first.tensors()[0], want[0])         # one further next(): still its own data
        feeder.next()
        with pytest.raises(RuntimeError):
            first.tensors()
        with pytest.raises(ValueError):
            feeder.next().into(torch.zeros(3, 1, 999), torch.zeros(3, 1, 999))


def test_corrupt_file_surfaces_with_its_name(tmp_path):
    root = str(tmp_path)
    wavtree.training_tree(root, [2000] * 4)
    bad = os.path.join(root, "training_set/noisy/fileid_2.wav")
    ds = CleanNoisyPairDataset(root=root, subset="training")
    for n in range(4):
        ds.pair_length(n)                               # headers parsed while the file was whole
    with open(bad, "r+b") as f:
        f.truncate(44 + 2 * 700)                        # the samples end early
    with BatchFeeder(ds, 2, "cpu", crop_length=1500, shuffle=False, timeout_s=20) as feeder:
        feeder.next()
        with pytest.raises(RuntimeError) as e:
            feeder.next()
        assert "fileid_2.wav" in str(e.value)
    # a file that is no wav at all fails in the plan, also with its name
    with open(bad, "wb") as f:
        f.write(b"not a wav file at all")
    with BatchFeeder(CleanNoisyPairDataset(root=root, subset="training"), 2, "cpu", crop_length=1500, timeout_s=20) as feeder:
        with pytest.raises(RuntimeError) as e:
            feeder.next()
        assert "fileid_2.wav" in str(e.value)


class _Stuck:
    """A dataset whose reads never return until the test lets them."""
    files = [(f"c{i}", f"n{i}") for i in range(4)]

    def __init__(self):
        self.gate = threading.Event()

    def __len__(self):
        return 4

    def pair_length(self, n):
        return 100

    def read_pcm(self, n, start, count):
        self.gate.wait(30)
        return np.zeros(count, np.int16), np.zeros(count, np.int16)


def test_next_times_out_and_close_leaves_no_thread():
    ds = _Stuck()
    before = {t for t in threading.enumerate()}
    feeder = BatchFeeder(ds, 2, "cpu", crop_length=64, timeout_s=1)
    assert any(t.name.startswith("BatchFeeder") for t in threading.enumerate())
    t0 = time.monotonic()
    with pytest.raises(TimeoutError):
        feeder.next()
    assert 0.9 < time.monotonic() - t0 < 3.0
    ds.gate.set()                                       # the readers come back
    batch = feeder.next()
    assert batch.tensors()[0].shape == (2, 1, 64)
    feeder.close()
    assert not [t for t in threading.enumerate() if t not in before and t.is_alive()]
    with pytest.raises(RuntimeError):
        feeder.next()


def test_workers_are_capped_and_not_sized_from_the_machine(tree):
    root, _ = tree
    ds = _dataset(root)
    before = threading.active_count()
    with BatchFeeder(ds, 4, "cpu") as f:
        assert threading.active_count() - before == 4           # the default
    with BatchFeeder(ds, 1, "cpu", depth=2, workers=64) as f:
        assert threading.active_count() - before == 2           # never more than the rows in flight
    assert threading.active_count() == before


def test_pcm_batch_argument_errors_need_no_gpu():
    """Every rejected argument set of cum_pcm_batch_f32 returns CUM_EINVAL with a text, before any launch."""
    from cleanumamba_amd import hip
    lib = hip.lib()
    P = ctypes.c_void_p
    ok = dict(pcm=P(0x1000), pitch=16, src_len=P(0x2000), batch=2, len=9, clean=P(0x3000), clean_sb=9, noisy=P(0x4000),
              noisy_sb=12)
    order = ["pcm", "pitch", "src_len", "batch", "len", "clean", "clean_sb", "noisy", "noisy_sb"]
    bad = [("batch", 0, b"batch"), ("batch", -3, b"batch"), ("len", 0, b"len"), ("pitch", 8, b"pitch"),
           ("pitch", 20, b"multiple of 8"), ("clean_sb", 8, b"clean_sb"), ("noisy_sb", 8, b"noisy_sb"),
           ("pcm", None, b"null"), ("src_len", None, b"null"), ("clean", None, b"null"), ("noisy", None, b"null"),
           ("pcm", P(0x1002), b"aligned"), ("clean", P(0x3004), b"aligned"), ("noisy", P(0x4008), b"aligned")]
    for name, value, text in bad:
        args = dict(ok, **{name: value})
        rc = lib.cum_pcm_batch_f32(*[args[k] for k in order], None)
        assert rc == -1, (name, value)
        assert text in lib.cum_last_error(), (name, value, lib.cum_last_error())
