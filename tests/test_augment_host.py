"""training/augment.py on the host: the draws (pure functions of their generator), the worst-case tap count, the
all-off config, ``apply`` on CPU tensors against the f64 oracle of augment_ref.py, the CPU BatchFeeder with ``augment``
and the argument checks of cum_augment_pairs, which run before any launch and therefore without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import augment_ref as R
import wavtree
from cleanumamba_amd.training import augment as A
from cleanumamba_amd.training.feeder import BatchFeeder
from cleanumamba_amd.util.dataset import CleanNoisyPairDataset

LENGTHS = [3000, 9000, 4099, 4100, 5000, 3500, 8000, 4098, 6001, 7000, 3333, 8999]      # as test_feeder_host.py
CROP, SHIFT = 1000, 37
FULL = dict(remix=True, shift=SHIFT, snr_db=(-5, 15), gain_db=(-6, 3))


def _echo():
    return A.Echo(rt60=(0.05, 0.1))              # short rooms: a few dozen taps at the test's lengths


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("pairs_aug"))
    return root, wavtree.training_tree(root, LENGTHS, seed=100)


def _dataset(root):
    return CleanNoisyPairDataset(root=root, subset="training", crop_length_sec=CROP / 16000)


def _same(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True)
               for k in ("perm", "off_clean", "off_noise", "snr_db", "gain", "kappa", "n_taps", "delay", "tap_gain"))


def test_draw_is_a_pure_function_of_its_generator():
    aug = A.Augment(echo=A.Echo(), **FULL)
    L, nb = 16000, 6
    a = aug.draw(np.random.default_rng(5), nb, L)
    b = aug.draw(np.random.default_rng(5), nb, L)
    c = aug.draw(np.random.default_rng(6), nb, L)
    assert _same(a, b) and not _same(a, c)
    assert a.length == L and a.shift == SHIFT and a.batch == nb
    assert sorted(a.perm.tolist()) == list(range(nb))
    for off in (a.off_clean, a.off_noise):
        assert off.dtype == np.int32 and off.min() >= 0 and off.max() <= SHIFT
    assert not np.array_equal(a.off_clean, a.off_noise)
    assert a.snr_db.dtype == np.float32 and (a.snr_db >= -5).all() and (a.snr_db <= 15).all()
    assert a.gain.dtype == np.float32 and (a.gain >= 10 ** (-6 / 20) * (1 - 1e-6)).all() and (a.gain <= 10 ** (3 / 20) * (1 + 1e-6)).all()
    assert (a.kappa == np.float32(0.1)).all()
    assert a.delay.shape == a.tap_gain.shape == (nb, A.K_MAX) and a.delay.dtype == np.int32
    assert a.tap_gain.dtype == np.float32
    for r in range(nb):
        n = int(a.n_taps[r])
        assert 0 < n <= A.K_MAX
        d = a.delay[r, :n]
        assert d.min() >= 1 and d.max() < L
        starts = [0] + [i for i in range(1, n) if d[i] <= d[i - 1]]             # a new repeat starts over
        assert len(starts) <= 3
        for s, e in zip(starts, starts[1:] + [n]):
            assert (np.diff(d[s:e]) > 0).all()                                   # ascending within a repeat
            assert (np.diff(a.tap_gain[r, s:e]) <= 0).all()                      # and decaying
        assert (a.delay[r, n:] == 0).all() and (a.tap_gain[r, n:] == 0).all()
    # a short clip drops the taps that would fall behind it
    short = aug.draw(np.random.default_rng(5), nb, 300)
    assert (short.n_taps < a.n_taps).all() and short.delay.max() < 300
    # transforms that are off draw nothing and give the neutral values
    plain = A.Augment(gain_db=(-3, 3)).draw(np.random.default_rng(1), 4, 100)
    assert plain.perm.tolist() == [0, 1, 2, 3] and not plain.off_clean.any() and np.isnan(plain.snr_db).all()
    assert not plain.n_taps.any() and not plain.rescales and (plain.kappa == 0).all()
    # proba = 0: never a tap
    assert not A.Augment(echo=A.Echo(proba=0.0)).draw(np.random.default_rng(1), 8, 16000).n_taps.any()


def test_worst_case_tap_count():
    assert A.Echo().max_taps == 3 * 145 == 435
    assert A.Augment(echo=A.Echo()).max_taps == 436 and A.Augment().max_taps == 0
    with pytest.raises(ValueError):
        A.Echo(rt60=(5, 5))
    with pytest.raises(ValueError):
        A.Echo(repeat=4)                                 # 4 x 145
    assert A.Echo(repeat=1, rt60=(3.0, 4.0)).max_taps <= A.K_MAX
    rng = np.random.default_rng(0)
    echo = A.Echo()
    assert max(len(echo.draw(rng, 1 << 30)) for _ in range(300)) <= echo.max_taps
    for bad in (dict(snr_db=(3, 1)), dict(shift=-1), dict(echo="yes"), dict(gain_db=(0, float("inf")))):
        with pytest.raises(ValueError):
            A.Augment(**bad)


def test_pack_layout():
    d = R.make_draws(10, 3, [1, 0], off_clean=[3, 0], off_noise=[1, 2], snr_db=[2.5, np.nan], gain=[0.5, 2.0],
                     taps=[[(1, 0.25), (4, 0.125)], []])
    assert d.columns() == 4 and d.rescales
    t = d.pack()
    assert t.dtype == np.int32 and t.shape == (A.table_ints(2, 4),) == (2 * (8 + 8),)
    recs = t[:16].reshape(2, 8)
    assert recs[:, :4].tolist() == [[1, 3, 1, 2], [0, 0, 2, 0]]
    assert recs[:, 4:7].view(np.float32).tolist()[0] == [2.5, 0.5, np.float32(0.1)]
    assert np.isnan(recs[1, 4:5].view(np.float32)[0]) and not recs[:, 7].any()
    assert t[16:24].tolist() == [1, 4, 0, 0, 0, 0, 0, 0]
    assert t[24:32].view(np.float32).tolist() == [0.25, 0.125, 0, 0, 0, 0, 0, 0]
    assert d.pack(8).shape == (2 * (8 + 16),)
    with pytest.raises(ValueError):
        d.pack(1)
    with pytest.raises(ValueError):
        R.make_draws(10, 3, [0, 0])                      # not a permutation
    with pytest.raises(ValueError):
        R.make_draws(10, 3, [0, 1], off_clean=[4, 0])    # beyond the shift


def _taps(L, n, seed):
    rng = np.random.default_rng(seed)
    return [(int(d), float(g)) for d, g in zip(rng.integers(1, L + 40, n), rng.uniform(-0.3, 0.3, n))]


CASES = {
    "remix": dict(perm=[0, 2, 1]),
    "shift": dict(off_clean=[0, 37, 5], off_noise=[36, 1, 5]),
    "snr": dict(snr_db=[5.0, np.nan, -3.25]),
    "gain": dict(gain=[0.5, 1.0, 1.7]),
    "echo": dict(taps=[_taps(515, 51, 1), [], [(1, 0.3)]], kappa=0.1),
    "all": dict(perm=[0, 2, 1], off_clean=[0, 37, 5], off_noise=[36, 1, 5], snr_db=[5.0, np.nan, -3.25],
                gain=[0.5, 1.0, 1.7], taps=[_taps(515, 51, 1), [(600, 0.5)], [(1, 0.3)]], kappa=0.25),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_apply_on_the_cpu_meets_the_oracle(case):
    L, S = 515, 37
    kw = dict(CASES[case])
    draws = R.make_draws(L, S, kw.pop("perm", [0, 1, 2]), **kw)
    C, Y = R.signals(3, L + S, seed=11)
    ref = R.reference(C, Y, draws)
    clean, noisy = A.apply(torch.from_numpy(C), torch.from_numpy(Y), draws)
    assert clean.shape == noisy.shape == (3, L) and clean.dtype == torch.float32
    R.check(clean.numpy(), noisy.numpy(), ref, case)
    if case in ("snr", "all"):
        assert R.snr_check(clean.numpy(), noisy.numpy(), ref, draws) == 2
    if case == "remix":                                  # nothing but an exchange: exact
        assert torch.equal(clean, torch.from_numpy(C[:, :L]))
        assert torch.equal(noisy, torch.from_numpy(C[:, :L] + (Y - C)[[0, 2, 1], :L]))
    # (B, 1, n) sources, given strided outputs: the same values, nothing written around them
    buf = torch.full((2, 3, 1, L + 5), 7.0)
    c3, n3 = A.apply(torch.from_numpy(C)[:, None], torch.from_numpy(Y)[:, None], draws, buf[0, :, :, :L], buf[1, :, :, :L])
    assert torch.equal(c3[:, 0], clean) and torch.equal(n3[:, 0], noisy) and (buf[..., L:] == 7).all()
    with pytest.raises(ValueError):
        A.apply(torch.from_numpy(C), torch.from_numpy(Y), draws, torch.from_numpy(C)[:, :L], None)       # overlap
    with pytest.raises(ValueError):
        A.apply(torch.from_numpy(C)[:, :L], torch.from_numpy(Y)[:, :L], draws)                           # no room to shift


def test_silent_rows_keep_a_at_one_on_the_cpu():
    L = 64
    # (row 1 has no taps: with an echo the reverberated speech is noise, and a silent noise row would not stay silent)
    draws = R.make_draws(L, 0, [0, 1, 2], snr_db=[3.0, 3.0, 3.0], taps=[[(2, 0.5)], [], [(2, 0.5)]])
    C, Y = R.signals(3, L, seed=3, silent_clean=[0], silent_noise=[1])
    ref = R.reference(C, Y, draws)
    assert ref["a"].tolist()[:2] == [1.0, 1.0] and ref["a"][2] != 1.0
    clean, noisy = A.apply(torch.from_numpy(C), torch.from_numpy(Y), draws)
    R.check(clean.numpy(), noisy.numpy(), ref, "silent")
    assert not clean[0].any()


def test_all_off_config_is_none(tree):
    root, _ = tree
    ds = _dataset(root)
    off = A.Augment(remix=False, shift=0, snr_db=None, gain_db=None, echo=None)
    assert not off.active and A.Augment(remix=True).active and A.Augment(echo=A.Echo()).active
    with BatchFeeder(ds, 4, "cpu", seed=3) as plain, BatchFeeder(ds, 4, "cpu", seed=3, augment=off) as same:
        assert same.augment is None and same.pitch == plain.pitch
        assert same._stage[0].flat.numel() == plain._stage[0].flat.numel()       # no table in the slot
        for a, b in zip(plain, same):
            assert b.draws is None and a.entries == b.entries
            (ca, na), (cb, nb) = a.tensors(), b.tensors()
            assert torch.equal(ca, cb) and torch.equal(na, nb)
    with pytest.raises(ValueError):
        BatchFeeder(ds, 4, "cpu", augment="remix")


def test_plan_with_and_without_shift(tree):
    root, _ = tree
    ds = _dataset(root)
    with BatchFeeder(ds, 4, "cpu", seed=3) as plain, \
            BatchFeeder(ds, 4, "cpu", seed=3, augment=A.Augment(remix=True, snr_db=(0, 10), echo=_echo())) as noshift, \
            BatchFeeder(ds, 4, "cpu", seed=3, augment=A.Augment(shift=SHIFT)) as shifted, \
            BatchFeeder(ds, 4, "cpu", seed=3, crop_length=CROP + SHIFT) as longer:
        for e in range(2):
            assert noshift.plan(e) == plain.plan(e)
            assert shifted.plan(e) == longer.plan(e) != plain.plan(e)
            assert all(count == CROP + SHIFT for b in shifted.plan(e) for _, _, count in b)
        assert shifted.pitch == longer.pitch and shifted.crop_length == CROP
        assert shifted.next().shape == (4, 1, CROP)


def test_feeder_draws_do_not_depend_on_workers_or_restarts(tree):
    root, _ = tree
    ds = _dataset(root)
    aug = A.Augment(echo=_echo(), **FULL)
    seen = {}
    for workers in (1, 4):
        with BatchFeeder(ds, 4, "cpu", seed=8, workers=workers, augment=aug) as feeder:
            got = []
            for epoch in range(2):
                for k, batch in enumerate(feeder):
                    want = aug.draw(np.random.Generator(np.random.PCG64([8, epoch, 0, k, 0x417567])), 4, CROP)
                    assert _same(batch.draws, want) and _same(feeder.draws(epoch, k), want)
                    got.append(batch.draws)
            assert len(got) == 6 and not _same(got[0], got[1]) and not _same(got[0], got[3])
        seen[workers] = got
    assert all(_same(a, b) for a, b in zip(seen[1], seen[4]))
    # a run restarted at epoch 1 draws epoch 1's draws: they hang on (seed, epoch, rank, batch) alone
    with BatchFeeder(ds, 4, "cpu", seed=8, augment=aug) as again:
        assert all(_same(again.draws(1, k), seen[1][3 + k]) for k in range(3))
    with BatchFeeder(ds, 2, "cpu", seed=8, rank=1, world=2, augment=aug) as other:
        assert not _same(other.draws(0, 0, 4), seen[1][0])


@pytest.mark.parametrize("workers", [1, 4])
def test_cpu_feeder_batches_meet_the_oracle_on_the_unaugmented_crops(tree, workers):
    root, _ = tree
    ds = _dataset(root)
    aug = A.Augment(echo=_echo(), **FULL)
    with BatchFeeder(ds, 4, "cpu", seed=9, workers=workers, augment=aug) as feeder, \
            BatchFeeder(ds, 4, "cpu", seed=9, crop_length=CROP + SHIFT) as longer:
        n = 0
        for batch, plain in zip(feeder, longer):
            assert batch.entries == plain.entries and batch.shape == (4, 1, CROP)
            C, Y = plain.tensors()
            ref = R.reference(C[:, 0].numpy(), Y[:, 0].numpy(), batch.draws)
            clean, noisy = batch.tensors()
            assert clean.shape == (4, 1, CROP)
            R.check(clean[:, 0].numpy(), noisy[:, 0].numpy(), ref, f"feeder batch {n}")
            assert R.snr_check(clean[:, 0].numpy(), noisy[:, 0].numpy(), ref, batch.draws) == 4
            again = torch.full((4, CROP + 3), 7.0), torch.full((4, 1, CROP), 7.0)
            batch.into(again[0][:, :CROP], again[1])
            assert torch.equal(again[0][:, :CROP], clean[:, 0]) and torch.equal(again[1], noisy)
            assert (again[0][:, CROP:] == 7).all()
            n += 1
        assert n == 3 and int(batch.draws.n_taps.max()) > 0


def augment_argument_errors():
    """Every rejected argument set of cum_augment_pairs returns CUM_EINVAL with a text, before any launch."""
    from cleanumamba_amd import hip
    lib = hip.lib()
    P = ctypes.c_void_p
    ok = dict(clean_src=P(0x1000), clean_src_sb=24, noisy_src=P(0x2000), noisy_src_sb=20, batch=2, len=9, src_len=20,
              recs=P(0x3000), tap_delay=P(0x4000), tap_gain=P(0x5000), k_max=4, workspace=P(0x6000), clean=P(0x7000),
              clean_sb=9, noisy=P(0x8000), noisy_sb=12)
    bad = [("batch", 0, b"batch"), ("batch", 32768, b"batch"), ("len", 0, b"len"), ("src_len", 8, b"src_len"),
           ("k_max", 513, b"k_max"), ("k_max", -1, b"k_max"), ("clean_src_sb", 19, b"src_sb"),
           ("noisy_src_sb", 19, b"src_sb"), ("clean_sb", 8, b"clean_sb"), ("noisy_sb", 8, b"noisy_sb"),
           ("clean_src", None, b"null"), ("noisy_src", None, b"null"), ("recs", None, b"null"), ("clean", None, b"null"),
           ("noisy", None, b"null"), ("tap_delay", None, b"null"), ("tap_gain", None, b"null"),
           ("clean", P(0x7004), b"16-byte"), ("noisy", P(0x8008), b"16-byte"), ("workspace", P(0x6004), b"8-byte"),
           ("clean_src", P(0x1002), b"4-byte"), ("recs", P(0x3001), b"4-byte"), ("tap_gain", P(0x5002), b"4-byte")]
    for name, value, text in bad:
        args = dict(ok, **{name: value})
        rc = lib.cum_augment_pairs(*args.values(), None)
        assert rc == -1, (name, value)
        assert text in lib.cum_last_error(), (name, value, lib.cum_last_error())
    assert lib.cum_augment_workspace_elems(3, 4099) == 4 * 3 * 3 and lib.cum_augment_workspace_elems(1, 2048) == 4
    assert lib.cum_augment_workspace_elems(0, 10) == 0


def test_augment_argument_errors_need_no_gpu():
    augment_argument_errors()
