"""A feeder for pairs at any sample rate, on the host (training/feeder.py with ``sample_rate``, util/resample.py,
csrc/resample.hip: cum_pcm_batch_resample_f32): the source window of a crop against the f64 definition, the plan rule,
the C entry's argument checks (they run before any launch, so without a GPU) and the CPU mode."""
import ctypes
import os

import numpy as np
import pytest
import torch

import wavtree
from resample_ref import resample_ref

MODEL = 16000
RATES = [8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000]
COUNTS = [1, 2, 767, 768, 769, 1537]


@pytest.mark.parametrize("rate", RATES)
def test_crop_window_holds_all_a_crop_reads_and_window_bound_is_tight(rate):
    """The f64 direct sum over the window alone (everything else zero) is the sum over the whole file, bit for bit; no
    window is longer than ``window_bound`` and, per count, some window is that long."""
    from cleanumamba_amd.util.resample import crop_window, out_length, plan, window_bound
    up, down, H, K, h = plan(rate, MODEL)
    rng = np.random.default_rng(rate)
    reached = {c: False for c in COUNTS}
    for N in (1, 2, 3, K - 1, K, K + 1, 5 * K + 7, 20000):
        x = rng.standard_normal(N)
        M = out_length(N, up, down)
        whole = resample_ref(x, h, up, down)[0]
        for count in COUNTS:
            if count > M:
                continue
            for m0 in sorted({0, min(1, M - count), (M - count) // 2, M - count}):
                n_lo, n_cnt = crop_window(N, up, down, H, K, m0, count)
                assert 0 <= n_lo and n_cnt >= 1 and n_lo + n_cnt <= N
                assert n_cnt <= window_bound(count, up, down, K), (rate, N, count, m0)
                alone = np.zeros(N)
                alone[n_lo:n_lo + n_cnt] = x[n_lo:n_lo + n_cnt]
                got = resample_ref(alone, h, up, down, m0, m0 + count)[0]
                assert np.array_equal(got, whole[m0:m0 + count]), (rate, N, count, m0)
            if N == 20000:           # every phase of the crop start: the bound is met and never passed
                for m0 in range(0, min(M - count, 2000) + 1):
                    n_cnt = crop_window(N, up, down, H, K, m0, count)[1]
                    assert n_cnt <= window_bound(count, up, down, K)
                    reached[count] |= n_cnt == window_bound(count, up, down, K)
    assert all(reached.values()), (rate, reached)


# ---- the plan rule ---------------------------------------------------------------------------------------------------
MIXED = [(8000, 9000), (16000, 9000), (22050, 14000), (44100, 30000), (48000, 30000), (48000, 9000), (16000, 3000),
         (32000, 20000)]           # (rate, frames): 48 k / 9000 and 16 k / 3000 give fewer than the crop's 4000 outputs
CROP = 4000


def mixed_tree(root, spec, seed=0):
    """``root/training_set/{clean,noisy}/fileid_{i}.wav``, pair i at spec[i] = (rate, frames); returns the int16 pairs."""
    pairs = []
    for sub in ("clean", "noisy"):
        os.makedirs(os.path.join(root, "training_set", sub), exist_ok=True)
    for i, (rate, n) in enumerate(spec):
        pair = (wavtree.pcm(n, seed + 2 * i), wavtree.pcm(n, seed + 2 * i + 1))
        for sub, x in zip(("clean", "noisy"), pair):
            wavtree.write_raw(os.path.join(root, "training_set", sub, f"fileid_{i}.wav"), x, rate=rate)
        pairs.append(pair)
    return pairs


class _Rated:
    """The headers of a mixed tree without the files' rates mattering to the device: what ``plan`` needs."""

    def __init__(self, ds):
        self.ds, self.files = ds, ds.files

    def __len__(self):
        return len(self.ds)

    def pair_length(self, n):
        return self.ds.pair_length(n)

    def pair_rate(self, n):
        return MODEL                 # (so that a CPU feeder can be built; the plan under test is set from RATES below)

    def read_pcm(self, n, start, count):
        return self.ds.read_pcm(n, start, count)


def _dataset(root):
    from cleanumamba_amd.util.dataset import CleanNoisyPairDataset
    return CleanNoisyPairDataset(root=root, subset="training", crop_length_sec=CROP / MODEL)


def test_rated_plan_on_a_16k_tree_is_the_unrated_plan(tmp_path):
    from cleanumamba_amd.training.feeder import BatchFeeder
    root = str(tmp_path)
    lengths = [3000, 9000, 4000, 4001, 5000, 3999, 8000, 6001]
    wavtree.training_tree(root, lengths, seed=3)
    ds = _dataset(root)
    with BatchFeeder(ds, 4, "cpu", crop_length=CROP, seed=5) as plain, \
            BatchFeeder(ds, 4, "cpu", crop_length=CROP, seed=5, sample_rate=MODEL) as rated:
        assert rated.pitch == plain.pitch and rated.crop_length == plain.crop_length == CROP
        for e in range(3):
            assert rated.plan(e) == plain.plan(e)
        assert any(start > 0 for b in rated.plan(0) for _, start, _ in b)
        for entries, windows in zip(*rated._plan_full(0)):
            for (index, start, count), (m0, M, rate) in zip(entries, windows):
                assert (m0, M, rate) == (start, lengths[index], MODEL) and count == min(CROP, M)
    with BatchFeeder(ds, 4, "cpu") as f:
        assert f.crop_length == CROP                     # the default stays int(crop_length_sec * 16000)


def _plan_only_feeder(ds, rates, **kw):
    """A rated CPU feeder over the headers of a mixed tree whose plan sees the files' true rates (no batch is made)."""
    from cleanumamba_amd.training.feeder import BatchFeeder
    from cleanumamba_amd.util import resample as rs
    f = BatchFeeder(_Rated(ds), 2, "cpu", crop_length=CROP, sample_rate=MODEL, **kw)
    f.close()                        # the readers would stage model-rate windows: only plan() is used
    f._rates = list(rates)
    for r in sorted(set(rates) - {MODEL}):
        f._rs_ids[r] = f._rs.add(rs.plan(r, MODEL))
    return f


def test_rated_plan_is_the_schedulers_alone_and_ranks_partition_an_epoch(tmp_path):
    from cleanumamba_amd.util.resample import crop_window, out_length, plan
    root = str(tmp_path)
    mixed_tree(root, MIXED)
    ds = _dataset(root)
    rates = [r for r, _ in MIXED]
    assert [ds.pair_rate(i) for i in range(len(ds))] == rates
    one, four = _plan_only_feeder(ds, rates, seed=3, workers=1), _plan_only_feeder(ds, rates, seed=3, workers=4)
    for e in range(3):
        assert one.plan(e) == four.plan(e) == one.plan(e)
        assert one._plan_full(e)[1] == four._plan_full(e)[1]
    assert one.plan(0) != one.plan(1)
    entries, windows = one._plan_full(0)
    assert sorted(i for b in entries for i, _, _ in b) == list(range(len(MIXED)))
    tiled = 0
    for b, w in zip(entries, windows):
        for (index, start, count), (m0, M, rate) in zip(b, w):
            N = MIXED[index][1]
            up, down, H, K, _ = plan(rate, MODEL) if rate != MODEL else (1, 1, 0, 1, None)
            assert rate == rates[index] and M == out_length(N, up, down)
            if M <= CROP:
                assert m0 == 0 and (start, count) == crop_window(N, up, down, H, K, 0, M)
                tiled += 1
            else:
                assert 0 <= m0 <= M - CROP and (start, count) == crop_window(N, up, down, H, K, m0, CROP)
            assert start >= 0 and start + count <= N
    assert tiled == 2
    # sharded ranks partition the epoch and keep the draws of the single-rank plan
    for e in range(2):
        r0 = _plan_only_feeder(ds, rates, seed=3, rank=0, world=2).plan(e)
        r1 = _plan_only_feeder(ds, rates, seed=3, rank=1, world=2).plan(e)
        a, c = [x for b in r0 for x in b], [x for b in r1 for x in b]
        assert len(a) == len(c) == 4 and not {i for i, _, _ in a} & {i for i, _, _ in c}
        assert sorted(a + c) == sorted(x for b in one.plan(e) for x in b)


# ---- the C entry -------------------------------------------------------------------------------------------------------
def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _case(**kw):
    """A good argument set of cum_pcm_batch_resample_f32: pair 0 a 48 k crop (outputs [100, 109) of 1000), pair 1 a 16 k
    file of 5 samples repeated.  Host tables are real (the entry reads them), device pointers are never followed."""
    P = ctypes.c_void_p
    plans = _i32([[1, 3, 219, 219, 220, 0, 0, 0]])
    recs = np.zeros((2, 16), dtype=np.int32)
    recs[0, :4] = (0, 243, 1000, 3000)                   # first sample read: (100 * 3 + 109) - 218 = 191, last 433
    recs[1, :4] = (-1, 5, 5, 5)
    pos = recs.view(np.int64)
    pos[0, 6], pos[0, 7] = 191, 100
    a = dict(pcm=P(0x10000), pitch=248, recs_host=recs, recs=P(0x20000), batch=2, plans_host=plans, plans=P(0x30000),
             n_plans=1, tables=P(0x40000), table_floats=220, len=9, clean=P(0x50000), clean_sb=9, noisy=P(0x60000),
             noisy_sb=12)
    a.update(kw)
    return a


ORDER = ["pcm", "pitch", "recs_host", "recs", "batch", "plans_host", "plans", "n_plans", "tables", "table_floats", "len",
         "clean", "clean_sb", "noisy", "noisy_sb"]


def _call(lib, a):
    args = []
    for k in ORDER:
        v = a[k]
        args.append(ctypes.c_void_p(v.ctypes.data) if isinstance(v, np.ndarray) else v)
    return lib.cum_pcm_batch_resample_f32(*args, None)


def _rec(row, **kw):
    """The good records with fields of record ``row`` replaced (plan, n_src, M, N, in0, out0)."""
    recs = _case()["recs_host"].copy()
    pos = recs.view(np.int64)
    for k, v in kw.items():
        if k in ("in0", "out0"):
            pos[row, 6 + ("in0", "out0").index(k)] = v
        else:
            recs[row, ("plan", "n_src", "M", "N").index(k)] = v
    return recs


def _plan(**kw):
    plans = _case()["plans_host"].copy()
    for k, v in kw.items():
        plans[0, ("up", "down", "taps", "K", "kp", "off").index(k)] = v
    return plans


def test_new_symbol_and_its_argument_errors_need_no_gpu():
    from cleanumamba_amd import hip
    lib = hip.lib()
    assert hasattr(lib, "cum_pcm_batch_resample_f32") and "cum_pcm_batch_resample_f32" in hip.SIGNATURES
    P = ctypes.c_void_p
    room = np.zeros(2 * 16 + 2, dtype=np.int32)
    k = 1 if room.ctypes.data % 8 == 0 else 2
    off8 = room[k:k + 32]                                # a record table 4 bytes off an 8-byte boundary
    off8[:] = _case()["recs_host"].reshape(-1)
    assert off8.ctypes.data % 8 == 4
    bad = [
        (dict(pcm=None), b"null"), (dict(recs=None), b"null"), (dict(recs_host=None), b"null"),
        (dict(clean=None), b"null"), (dict(noisy=None), b"null"), (dict(plans=None), b"null plan"),
        (dict(plans_host=None), b"null plan"), (dict(tables=None), b"null plan"),
        (dict(pcm=P(0x10008)), b"16-byte"), (dict(clean=P(0x50004)), b"16-byte"), (dict(noisy=P(0x60008)), b"16-byte"),
        (dict(tables=P(0x40004)), b"16-byte"), (dict(recs=P(0x20004)), b"misaligned"), (dict(recs_host=off8), b"misaligned"),
        (dict(plans=P(0x30002)), b"misaligned"),
        (dict(batch=0), b"batch"), (dict(batch=-2), b"batch"), (dict(batch=32768), b"batch"), (dict(len=0), b"len"),
        (dict(pitch=244), b"multiple of 8"), (dict(pitch=240), b"n_src"), (dict(clean_sb=8), b"clean_sb"),
        (dict(noisy_sb=8), b"noisy_sb"), (dict(n_plans=-1), b"negative"),
        (dict(recs_host=_rec(0, plan=1)), b"plan outside"), (dict(recs_host=_rec(1, plan=-2)), b"plan outside"),
        (dict(n_plans=0, plans=None, plans_host=None, tables=None), b"plan outside"),
        (dict(plans_host=_plan(up=0)), b"up and down"), (dict(plans_host=_plan(down=1025)), b"1024"),
        (dict(plans_host=_plan(taps=218)), b"odd"), (dict(plans_host=_plan(K=218)), b"smaller than the tap count"),
        (dict(plans_host=_plan(kp=218)), b"table_pitch"), (dict(plans_host=_plan(off=4)), b"blob"),
        (dict(plans_host=_plan(off=2)), b"blob"), (dict(table_floats=219), b"blob"),
        (dict(plans_host=_plan(down=48, taps=3477, K=3477, kp=3480), table_floats=3480), b"LDS"),
        (dict(recs_host=_rec(0, M=0)), b"M must be"), (dict(recs_host=_rec(1, M=0, N=0)), b"M must be"),
        (dict(recs_host=_rec(0, M=999)), b"M must be"),
        (dict(recs_host=_rec(0, out0=992, in0=2867, n_src=133)), b"out0 + len exceeds M"),
        (dict(recs_host=_rec(1, out0=1)), b"out0 + len exceeds M"),
        (dict(recs_host=_rec(0, in0=192, n_src=242)), b"starts behind"),
        (dict(recs_host=_rec(0, n_src=242)), b"ends before"), (dict(recs_host=_rec(1, n_src=4)), b"ends before"),
        (dict(recs_host=_rec(1, n_src=6)), b"past the end"), (dict(recs_host=_rec(0, in0=-1)), b"negative"),
        (dict(recs_host=_rec(0, out0=-1)), b"negative"), (dict(recs_host=_rec(0, n_src=-1)), b"n_src"),
    ]
    for change, text in bad:
        rc = _call(lib, _case(**change))
        assert rc == -1, change
        assert text in lib.cum_last_error(), (change, lib.cum_last_error())
    # Record 0 of the good set passes every check, and so does a window that stops short of what its outputs would read
    # where the file ends, or starts late where the file starts: the error is then record 1's.  (No set here is all
    # good: that would launch.)
    ends = dict(out0=991, in0=2864, n_src=136)           # the last output's n_hi is 3106: past the file's 3000 samples
    starts = dict(out0=0, in0=0, n_src=136)              # the first output's oldest tap is sample -109
    for change in ({}, ends, starts):
        recs = _rec(0, **change)
        recs[1, 0] = -2
        assert _call(lib, _case(recs_host=recs)) == -1 and b"plan outside" in lib.cum_last_error(), change


# ---- device="cpu" ------------------------------------------------------------------------------------------------------
def test_rated_cpu_feeder_on_a_16k_tree_gives_the_unrated_batches(tmp_path):
    from cleanumamba_amd.training.feeder import BatchFeeder
    root = str(tmp_path)
    wavtree.training_tree(root, [3000, 9000, 4000, 4001, 5000, 3999, 8000, 6001], seed=11)
    ds = _dataset(root)
    with BatchFeeder(ds, 4, "cpu", crop_length=CROP, seed=2) as plain, \
            BatchFeeder(ds, 4, "cpu", crop_length=CROP, seed=2, sample_rate=MODEL) as rated:
        n = 0
        for a, b in zip(plain, rated):
            assert a.entries == b.entries and a.fileids == b.fileids and a.windows is None
            assert b.windows == [(start, ds.pair_length(i), MODEL) for i, start, _ in b.entries]
            (ca, na), (cb, nb) = a.tensors(), b.tensors()
            assert cb.shape == (4, 1, CROP) and torch.equal(ca, cb) and torch.equal(na, nb)
            n += 1
        assert n == 2


def test_cpu_feeder_refuses_a_48k_pair_and_pair_rate_a_mismatched_one(tmp_path):
    from cleanumamba_amd.training.feeder import BatchFeeder
    root = str(tmp_path)
    mixed_tree(root, [(16000, 5000), (48000, 9000), (16000, 5000)])
    ds = _dataset(root)
    with pytest.raises(ValueError, match="fileid_1.wav") as e:
        BatchFeeder(ds, 1, "cpu", crop_length=1000, sample_rate=MODEL)
    assert "48000" in str(e.value)
    with BatchFeeder(ds, 1, "cpu", crop_length=1000) as f:          # unrated: the header rates are never read
        assert f.sample_rate is None and f.next().tensors()[0].shape == (1, 1, 1000)
    wavtree.write_raw(os.path.join(root, "training_set/noisy/fileid_2.wav"), wavtree.pcm(5000, 1), rate=8000)
    ds = _dataset(root)
    assert ds.pair_rate(0) == 16000 and ds.pair_rate(1) == 48000
    with pytest.raises(AssertionError) as e:
        ds.pair_rate(2)
    assert "clean/fileid_2.wav" in str(e.value) and "noisy/fileid_2.wav" in str(e.value)


def test_a_rate_the_resampler_cannot_reduce_is_named(tmp_path):
    """Checked before any GPU work: the device is only named, never touched, when the constructor raises."""
    from cleanumamba_amd.training import feeder as F
    root = str(tmp_path)
    mixed_tree(root, [(16000, 5000), (16001, 5000)])
    f = F.BatchFeeder.__new__(F.BatchFeeder)
    f.dataset, f.sample_rate, f.crop_length, f.device = _dataset(root), MODEL, 1000, torch.device("cuda", 0)
    with pytest.raises(ValueError, match="fileid_1.wav") as e:
        f._read_rates(True)
    assert "16001" in str(e.value)
