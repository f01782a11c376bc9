"""Reverb on the host (training/augment.py): the preparation rule, the refusals, the draw order, the packed
records, the torch restatement of the stage against the f64 oracle of reverb_ref.py, the CPU feeder, and the library's
argument checks."""
import ctypes
import os

import numpy as np
import pytest
import torch

import augment_ref as AR
import reverb_ref as R
import wavtree
from test_feeder_host import expected_batch


def make_draws(L, S, ids, **kw):
    """AugmentDraws of augment_ref.make_draws with per-row response ids."""
    from cleanumamba_amd.training.augment import AugmentDraws
    d = AR.make_draws(L, S, kw.pop("perm", list(range(len(ids)))), **kw)
    return AugmentDraws(L, S, d.perm, d.off_clean, d.off_noise, d.snr_db, d.gain, d.kappa, d.n_taps, d.delay, d.tap_gain,
                        rir=ids)


def direct_c(rows):
    """The constant of a direct f32 convolution, per row: T terms in some fixed order round fewer than T times on partial
    sums no larger than s_b, and each product once."""
    return np.array([(len(h) + 2) if h is not None else 0 for h in rows], dtype=np.float64)


def small_reverb(**kw):
    from cleanumamba_amd.training.augment import Reverb
    kw.setdefault("decay_db", R.DECAY)                   # (every tap stays)
    return Reverb([R.synth_raw(T, 40 + i) for i, T in enumerate((1, 2, 37, 300, 1500))], **kw)


def test_preparation_rule():
    from cleanumamba_amd.training.augment import Reverb, prepare_rir
    raw = R.raw_response()
    want = R.prepare(raw)
    got = Reverb([raw]).taps[0]
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert abs(float((got.astype(np.float64) ** 2).sum()) - 1.0) < 1e-6          # unit energy
    assert np.argmax(np.abs(got)) == 0 and got[0] > 0                              # the direct path first: 37 samples cut
    assert 2000 < got.shape[0] < 3000          # the Schroeder cut falls in the body (60 dB over 3000), not in the 9000 tail
    for db in (20.0, 40.0):
        assert np.array_equal(Reverb([raw], decay_db=db).taps[0], R.prepare(raw, decay_db=db))
    assert Reverb([raw], decay_db=20.0).taps[0].shape[0] < Reverb([raw], decay_db=40.0).taps[0].shape[0] < got.shape[0]
    capped = Reverb([raw], max_taps=100).taps[0]
    assert capped.shape == (100,) and np.array_equal(capped, R.prepare(raw, max_taps=100))
    long = np.random.default_rng(0).standard_normal(40000)                         # no decay at all: the cap is T_MAX
    long[0] = 10.0
    rv = Reverb([long], max_taps=10 ** 6)
    assert rv.t_max == R.T_MAX and rv.taps[0].shape == (R.T_MAX,) and np.array_equal(rv.taps[0], R.prepare(long))
    two = Reverb([np.stack([raw, -raw[::-1]])]).taps[0]                            # channels first: channel 0
    assert np.array_equal(two, want)
    assert np.array_equal(prepare_rir(np.array([0.0, -2.0, 1.0, 2.0])), R.prepare([0.0, -2.0, 1.0, 2.0]))   # the first peak
    assert np.array_equal(Reverb([[3.0]]).taps[0], np.ones(1, np.float32))


def test_a_directory_is_read_sorted_and_a_wrong_rate_is_named(tmp_path):
    from scipy.io import wavfile
    from cleanumamba_amd.training.augment import Reverb
    raw = [R.synth(T, 7 + i) for i, T in enumerate((50, 700))]
    os.makedirs(tmp_path / "b")
    wavfile.write(tmp_path / "b" / "x.wav", 16000, raw[0])                         # float32 files
    wavfile.write(tmp_path / "a.wav", 16000, (raw[1] * 20000).astype(np.int16))    # and 16-bit PCM
    (tmp_path / "notes.txt").write_text("not a response")
    rv = Reverb(str(tmp_path))
    assert len(rv) == 2
    assert np.array_equal(rv.taps[0], R.prepare((raw[1] * 20000).astype(np.int16).astype(np.float32) / 32768.0))
    assert np.array_equal(rv.taps[1], R.prepare(raw[0]))
    wavfile.write(tmp_path / "b" / "y.wav", 48000, raw[0])
    with pytest.raises(ValueError, match="y.wav"):
        Reverb(str(tmp_path))
    os.remove(tmp_path / "b" / "y.wav")
    (tmp_path / "b" / "z.wav").write_bytes(b"RIFFjunk")
    with pytest.raises(ValueError, match="z.wav"):
        Reverb(str(tmp_path))


def test_refusals():
    from cleanumamba_amd.training.augment import Augment, AugmentDraws, Reverb
    h = R.synth(10, 0)
    for bad in ([], [np.zeros(5)], [[1.0, np.nan]], [[1.0, np.inf]], [np.zeros((2, 0))], [np.ones((2, 2, 2))]):
        with pytest.raises(ValueError):
            Reverb(bad)
    for kw in (dict(proba=-0.1), dict(proba=1.5), dict(decay_db=0.0), dict(decay_db=-3.0), dict(max_taps=0)):
        with pytest.raises(ValueError):
            Reverb([h], **kw)
    with pytest.raises(ValueError):
        Augment(reverb="room")
    with pytest.raises(ValueError):
        Augment(reverb=[h])
    assert Augment(reverb=Reverb([h])).active and not Augment(reverb=None).active and not Augment().active
    base = AR.make_draws(60, 4, [0, 1, 2])
    args = (60, 4, base.perm, base.off_clean, base.off_noise, base.snr_db, base.gain, base.kappa, base.n_taps, base.delay,
            base.tap_gain)
    for bad in ([0, 1], [[0, 1, 2]], [0, 1, 2, 3]):
        with pytest.raises(ValueError):
            AugmentDraws(*args, rir=bad)
    d = AugmentDraws(*args)
    assert d.rir.dtype == np.int32 and d.rir.tolist() == [-1, -1, -1] and not d.reverberant
    assert AugmentDraws(*args, rir=[-1, 0, -1]).reverberant


CONFIGS = [dict(), dict(remix=True), dict(shift=37), dict(snr_db=(-5, 15)), dict(gain_db=(-6, 3)), dict(echo=True),
           dict(band_mask=True), dict(remix=True, shift=37, snr_db=(-5, 15), gain_db=(-6, 3), echo=True, band_mask=True)]


@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: "+".join(c) or "none")
def test_existing_draws_are_untouched_and_the_rooms_are_drawn_last(config):
    from cleanumamba_amd.training.augment import Augment, BandMask, Echo
    kw = dict(config)
    if kw.pop("echo", False):
        kw["echo"] = Echo(rt60=(0.05, 0.1))
    if kw.pop("band_mask", False):
        kw["band_mask"] = BandMask()
    names = ("perm", "off_clean", "off_noise", "snr_db", "gain", "kappa", "n_taps", "delay", "tap_gain", "band_half",
             "band_lo", "band_hi")
    rng, twin, third = (np.random.default_rng(8) for _ in range(3))
    rv = small_reverb(proba=0.5)
    plain = Augment(**kw).draw(rng, 6, 3000)
    again = Augment(**kw, reverb=None).draw(twin, 6, 3000)
    room = Augment(**kw, reverb=rv).draw(third, 6, 3000)
    for name in names:
        assert np.array_equal(getattr(plain, name), getattr(again, name), equal_nan=True), name
        assert np.array_equal(getattr(plain, name), getattr(room, name), equal_nan=True), name
    assert rng.bit_generator.state == twin.bit_generator.state        # reverb=None drew nothing more
    assert not plain.reverberant and (plain.rir == -1).all()
    want = []
    for _ in range(6):                                   # the generator after the band's draws gives the rooms, row by row
        want.append(int(rng.integers(0, 5)) if rng.random() < 0.5 else -1)
    assert room.rir.tolist() == want and rng.bit_generator.state == third.bit_generator.state


def test_rooms_are_drawn_at_the_rate_proba():
    rv = small_reverb(proba=0.3)
    rng = np.random.default_rng(1)
    ids = np.array([rv.draw(rng) for _ in range(20000)])
    assert abs((ids == -1).mean() - 0.7) < 0.02          # (six standard deviations of a fair count are 0.019)
    assert set(ids[ids >= 0].tolist()) == set(range(5)) and ids.min() == -1
    assert all(small_reverb(proba=0.0).draw(rng) == -1 for _ in range(50))
    assert all(0 <= small_reverb(proba=1.0).draw(rng) < 5 for _ in range(50))


def test_pack_reverb_layout_and_the_without_forms():
    import bandmask_ref as BR
    from cleanumamba_amd.training.augment import REVERB_INTS, AugmentDraws, reverb_ints
    d = make_draws(60, 4, [3, -1, 0])
    table = d.pack_reverb()
    assert table.dtype == np.int32 and table.shape == (reverb_ints(3),) == (REVERB_INTS * 3,) == (12,)
    assert np.array_equal(table, R.pack([3, -1, 0])) and table.reshape(3, 4)[:, 0].tolist() == [3, -1, 0]
    assert not table.reshape(3, 4)[:, 1:].any()
    bands = [BR.band(0, 23), (0, 0.0, 0.0), BR.band(100, 119)]
    both = AugmentDraws(60, 4, d.perm, d.off_clean, d.off_noise, d.snr_db, d.gain, d.kappa, d.n_taps, d.delay, d.tap_gain,
                        *zip(*bands), rir=[3, -1, 0])
    assert both.banded and both.reverberant
    nb = both.without_band()
    assert not nb.banded and nb.reverberant and nb.rir.tolist() == [3, -1, 0]          # the band goes, the rooms stay
    nr = both.without_reverb()
    assert nr.banded and not nr.reverberant and np.array_equal(nr.pack_band(), both.pack_band())
    assert np.array_equal(nr.pack(), both.pack()) and np.array_equal(nb.pack(), both.pack())


@pytest.mark.parametrize("form", ["flat", "three"])
def test_reverb_on_cpu_tensors_meets_the_oracle(form):
    """Rows shorter and longer than the response; a -1 row and an id past the bank are copies.  The host path is a direct
    f32 convolution: its constant is the tap count."""
    from cleanumamba_amd.training.augment import reverb
    rv = small_reverb()
    bank = rv.bank("cpu")
    assert len(bank) == 5 and bank.table_host[:, 2].tolist() == [1, 2, 37, 300, 1500]
    offs = bank.table_host.view(np.int64)[:, 0]
    assert (offs % 4 == 0).all() and offs.tolist() == [0, 4, 8, 48, 348] and bank.blob.numel() == 1848
    assert rv.bank("cpu") is bank
    ids = [4, 2, -1, 0, 5, 3]
    rows = [rv.taps[r] if 0 <= r < 5 else None for r in ids]
    for n in (7, 500, 2001):
        C, Y = R.case_signals(n, 6, seed=n)
        c_src, y_src = torch.from_numpy(C), torch.from_numpy(Y)
        if form == "three":
            c_src, y_src = c_src[:, None], y_src[:, None]
        clean, noisy = reverb(c_src, y_src, make_draws(n - 3, 3, ids), bank)
        assert clean.shape == c_src.shape
        R.check((clean.reshape(6, n).numpy(), noisy.reshape(6, n).numpy()), C, Y, rows, f"cpu n = {n}", c=direct_c(rows))
        assert torch.equal(c_src.reshape(6, n), torch.from_numpy(C))


def test_apply_on_cpu_tensors_runs_the_reverb_first():
    import bandmask_ref as BR
    from cleanumamba_amd.training.augment import AugmentDraws, apply, band_mask, reverb
    L, S = 900, 30
    rv = small_reverb()
    d = AR.make_draws(L, S, [2, 0, 1], off_clean=[1, 30, 0], off_noise=[29, 2, 4], snr_db=[5.0, np.nan, -3.0],
                      gain=[0.5, 1.0, 1.7], taps=[[(3, 0.4), (40, -0.2)], [], [(1, 0.3)]])
    bands = [BR.band(5, 20), BR.band(100, 119), (0, 0.0, 0.0)]
    draws = AugmentDraws(L, S, d.perm, d.off_clean, d.off_noise, d.snr_db, d.gain, d.kappa, d.n_taps, d.delay, d.tap_gain,
                         *zip(*bands), rir=[3, -1, 4])
    C, Y = (torch.from_numpy(x) for x in R.case_signals(L + S, 3, seed=4))
    got = apply(C, Y, draws, reverb=rv)
    staged = reverb(C, Y, draws, rv.bank("cpu"))
    want = apply(*staged, draws.without_reverb())
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    want = apply(*band_mask(*staged, draws), draws.without_reverb().without_band())
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(got[0], apply(C, Y, draws.without_reverb())[0])
    with pytest.raises(ValueError, match="reverb"):
        apply(C, Y, draws)
    plain = draws.without_reverb()
    a, b = apply(C, Y, plain), apply(C, Y, plain, reverb=rv)                           # nothing to do: reverb= is not read
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_cpu_feeder_with_a_reverb_equals_apply_on_its_unaugmented_crops(tmp_path):
    from cleanumamba_amd.training.augment import Augment, BandMask, apply
    from cleanumamba_amd.training.feeder import BatchFeeder
    from cleanumamba_amd.util.dataset import CleanNoisyPairDataset
    root, crop, shift = str(tmp_path), 1500, 21
    pairs = wavtree.training_tree(root, [1200, 4000, 1521, 2500], seed=60)
    ds = CleanNoisyPairDataset(root=root, subset="training", crop_length_sec=crop / 16000)
    rv = small_reverb(proba=0.7)
    for config, extra in ((dict(reverb=rv), 2 * 4), (dict(remix=True, shift=shift, gain_db=(-6, 3), band_mask=BandMask(),
                                                          reverb=rv), 2 * 4 + 2 * 4)):
        augment = Augment(**config)
        with BatchFeeder(ds, 2, "cpu", crop_length=crop, seed=2, augment=augment) as feeder:
            s = augment.shift
            assert feeder._dev[0].flat.numel() == 2 * 2 * feeder.pitch + 2 * 2 + 2 * (2 * 8 + extra)
            n, rooms = 0, 0
            for batch in feeder:
                clean, noisy = batch.tensors()
                C, Y = expected_batch(pairs, batch.entries, crop + s)
                want = apply(C, Y, batch.draws, reverb=rv)
                assert torch.equal(clean, want[0]) and torch.equal(noisy, want[1])
                if batch.draws.reverberant:
                    rooms += 1
                    assert not torch.equal(clean, apply(C, Y, batch.draws.without_reverb())[0])
                n += 1
            assert n == 2 and rooms >= 1


def reverb_argument_errors():
    """Every rejected argument set of cum_reverb_pairs returns CUM_EINVAL with a text, before any launch.  The host table
    is real (the entry reads it); the device pointers are never followed."""
    from cleanumamba_amd import hip
    lib = hip.lib()
    P = ctypes.c_void_p
    T_MAX = lib.cum_reverb_max_taps()
    assert T_MAX == 16384 and lib.cum_reverb_block() == 4096

    def table(*recs):
        t = np.zeros((len(recs), 4), dtype=np.int32)
        for r, (off, taps) in enumerate(recs):
            t[r].view(np.int64)[0], t[r, 2] = off, taps
        return t
    good = table((0, 10), (12, T_MAX))
    ok = dict(clean_src=P(0x1000), clean_src_sb=24, noisy_src=P(0x2000), noisy_src_sb=20, batch=2, n=20, recs=P(0x3000),
              bank=P(0x4000), bank_floats=12 + T_MAX, rirs_host=good, rirs=P(0x5000), n_rirs=2, workspace=P(0x6000),
              clean=P(0x7000), clean_sb=20, noisy=P(0x8000), noisy_sb=24)
    bad = [("batch", 0, b"batch"), ("batch", 32768, b"batch"), ("n", 0, b"n must"), ("clean_src_sb", 19, b"src_sb"),
           ("noisy_src_sb", 19, b"src_sb"), ("clean_sb", 19, b"clean_sb"), ("noisy_sb", 19, b"noisy_sb"),
           ("clean_src", None, b"null"), ("noisy_src", None, b"null"), ("recs", None, b"null"), ("bank", None, b"null"),
           ("rirs_host", None, b"null"), ("rirs", None, b"null"),
           ("workspace", None, b"null"), ("clean", None, b"null"), ("noisy", None, b"null"),
           ("clean", P(0x7004), b"16-byte"), ("noisy", P(0x8008), b"16-byte"), ("workspace", P(0x6004), b"8-byte"),
           ("clean_src", P(0x1002), b"4-byte"), ("noisy_src", P(0x2001), b"4-byte"), ("recs", P(0x3002), b"4-byte"),
           ("bank", P(0x4002), b"4-byte"), ("rirs", P(0x5001), b"4-byte"),
           ("n_rirs", 0, b"n_rirs"), ("bank_floats", 0, b"bank_floats"),
           ("rirs_host", table((0, 10), (12, 0)), b"taps"), ("rirs_host", table((0, 10), (12, T_MAX + 1)), b"taps"),
           ("rirs_host", table((0, -5), (12, 4)), b"taps"),
           ("rirs_host", table((0, 10), (10, 4)), b"offset"), ("rirs_host", table((-4, 10), (12, 4)), b"offset"),
           ("rirs_host", table((0, 10), (16, T_MAX)), b"span"), ("rirs_host", table((0, 10), (2 ** 40, 4)), b"span"),
           ("bank_floats", 11 + T_MAX, b"span")]
    for name, value, text in bad:
        args = dict(ok, **{name: value})
        keep = [v for v in args.values() if isinstance(v, np.ndarray)]
        call = [P(v.ctypes.data) if isinstance(v, np.ndarray) else v for v in args.values()]
        rc = lib.cum_reverb_pairs(*call, None)
        assert rc == -1, (name, value)
        assert text in lib.cum_last_error(), (name, value, lib.cum_last_error())
        del keep
    N = lib.cum_reverb_block()
    assert lib.cum_reverb_workspace_elems(0, 100) == 0 and lib.cum_reverb_workspace_elems(1, 0) == 0
    head = lib.cum_reverb_workspace_elems(1, 1) - 2 * N * (T_MAX // (N // 2) + 1)
    assert head >= 2 * (N + 1)                           # the twiddle table
    for batch, n in ((1, N // 2), (1, N // 2 + 1), (3, 168000)):
        blocks = -(-n // (N // 2))
        assert lib.cum_reverb_workspace_elems(batch, n) == head + 2 * N * batch * (T_MAX // (N // 2) + blocks)
    assert lib.cum_abi_version() == 16


def test_reverb_argument_errors_need_no_gpu():
    reverb_argument_errors()
    from cleanumamba_amd.training.augment import reverb
    bank = small_reverb().bank("cpu")
    C, Y = (torch.from_numpy(x) for x in R.case_signals(64, 2, seed=1))
    draws = make_draws(60, 4, [0, 1])
    with pytest.raises(ValueError):
        reverb(C, Y, draws, bank, C, None)               # an output over a source
    with pytest.raises(ValueError):
        reverb(C[:, :60], Y, draws, bank)                # not L + S long
    with pytest.raises(ValueError):
        reverb(C.double(), Y, draws, bank)
    with pytest.raises(ValueError):
        reverb(C, Y, draws, small_reverb().taps)         # not a bank
