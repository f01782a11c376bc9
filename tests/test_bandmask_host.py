"""BandMask on the host (training/augment.py): the mel edges, the draw, the packed records, the torch
restatement of the stage against the f64 oracle of bandmask_ref.py, the CPU feeder, and the library's argument checks.

The half-widths at the extreme bands follow the contract's own formula, W = int(2 / c) on the float32 edge widened to
f64: float32(40 / 16000) lies just below 0.0025, so the lowest edge gives 800 (1 601 taps), and the top edge, exactly
0.5, gives 4."""
import ctypes

import numpy as np
import pytest
import torch

import augment_ref as AR
import bandmask_ref as R
import wavtree
from test_feeder_host import expected_batch


def direct_c(bands):
    """The constant of a direct f32 convolution, per row: K = 2 W + 1 taps round K times on partial sums no larger than
    s_b (the standard bound of a fixed-order f32 chain)."""
    return np.array([2 * W + 1 for W, _, _ in bands], dtype=np.float64)


def test_mel_edges():
    from cleanumamba_amd.training.augment import BandMask, mel_edges
    e = mel_edges()
    assert e.dtype == np.float32 and e.shape == (120,)
    assert e[0] == np.float32(40 / 16000) and e[119] == np.float32(0.5)
    assert (np.diff(e.astype(np.float64)) > 0).all()
    assert np.array_equal(e, R.mel_edges()) and np.array_equal(BandMask().edges, e)
    other = mel_edges(64, 100.0, 48000)
    assert np.array_equal(other, R.mel_edges(64, 100.0, 48000)) and other[-1] == np.float32(0.5)


def test_draw_is_a_pure_function_of_its_generator():
    from cleanumamba_amd.training.augment import BandMask
    bm = BandMask()
    assert bm.bandwidth == 24 and bm.max_half == 800
    a = [bm.draw(np.random.default_rng(5)) for _ in range(2)]
    assert a[0] == a[1]
    rng, twin = np.random.default_rng(11), np.random.default_rng(11)
    seen = set()
    for _ in range(400):
        W, c_lo, c_hi = bm.draw(rng)
        assert twin.random() < 1.0                       # proba = 1: one uniform, then the two integers, nothing else
        lo = int(twin.integers(0, 120))
        hi = int(twin.integers(lo, min(120, lo + 24)))
        assert lo <= hi < min(120, lo + 24)
        assert (c_lo, c_hi) == (bm.edges[lo], bm.edges[hi]) and W == int(2.0 / float(bm.edges[lo])) == R.band(lo, hi)[0]
        seen.add(lo)
    assert rng.random() == twin.random() and len(seen) > 100
    assert R.band(0, 0)[0] == 800 and R.band(119, 119)[0] == 4        # the extreme bands (see the module's docstring)
    none = BandMask(proba=0.0)
    rng, twin = np.random.default_rng(3), np.random.default_rng(3)
    assert none.draw(rng) == (0, 0.0, 0.0)
    twin.random()
    assert rng.random() == twin.random()                 # a band that is not drawn consumed one uniform


def test_constructor_refuses_what_the_kernel_cannot_take():
    from cleanumamba_amd.training.augment import W_MAX, Augment, BandMask
    assert W_MAX == 1600
    with pytest.raises(ValueError, match="half-width"):
        BandMask(min_freq=15)
    assert BandMask(min_freq=20).max_half == 1600
    with pytest.raises(ValueError):
        BandMask(maxwidth=0.001)                         # bandwidth = int(0.12) = 0
    with pytest.raises(ValueError):
        Augment(band_mask="yes")
    assert Augment(band_mask=BandMask()).active and not Augment().active


def test_equal_edges_give_the_unit_impulse():
    from cleanumamba_amd.training.augment import band_taps
    for j in (0, 5, 60, 119):
        W, c, _ = R.band(j, j)
        for h in (R.taps(W, c, c), band_taps(W, c, c).astype(np.float64)):
            want = np.zeros(2 * W + 1)
            want[W] = 1.0
            assert np.array_equal(h, want)
    W, lo, hi = R.band(5, 20)
    assert np.array_equal(band_taps(W, lo, hi).astype(np.float64), R.taps(W, lo, hi))
    assert np.array_equal(R.taps(W, lo, hi), R.taps(W, lo, hi)[::-1])


CONFIGS = [dict(), dict(remix=True), dict(shift=37), dict(snr_db=(-5, 15)), dict(gain_db=(-6, 3)), dict(echo=True),
           dict(remix=True, shift=37, snr_db=(-5, 15), gain_db=(-6, 3), echo=True)]


@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: "+".join(c) or "none")
def test_existing_draws_are_untouched_and_the_band_is_drawn_last(config):
    from cleanumamba_amd.training.augment import Augment, BandMask, Echo
    kw = dict(config)
    if kw.pop("echo", False):
        kw["echo"] = Echo(rt60=(0.05, 0.1))
    names = ("perm", "off_clean", "off_noise", "snr_db", "gain", "kappa", "n_taps", "delay", "tap_gain")
    rng, twin, third = (np.random.default_rng(8) for _ in range(3))
    plain = Augment(**kw).draw(rng, 4, 3000)
    again = Augment(**kw, band_mask=None).draw(twin, 4, 3000)
    band = Augment(**kw, band_mask=BandMask()).draw(third, 4, 3000)
    for name in names:
        assert np.array_equal(getattr(plain, name), getattr(again, name), equal_nan=True), name
        assert np.array_equal(getattr(plain, name), getattr(band, name), equal_nan=True), name
    assert rng.bit_generator.state == twin.bit_generator.state       # band_mask=None drew nothing more
    assert not plain.banded and not plain.band_half.any() and plain.band_lo.dtype == np.float32
    W, c_lo, c_hi = BandMask().draw(rng)                 # the generator after the echo's draws gives the batch's band
    assert band.banded and (band.band_half == W).all() and (band.band_lo == c_lo).all() and (band.band_hi == c_hi).all()
    assert rng.bit_generator.state == third.bit_generator.state


def test_pack_band_layout_and_validation():
    from cleanumamba_amd.training.augment import BAND_INTS, AugmentDraws, band_ints
    bands = [R.band(0, 23), (0, 0.0, 0.0), R.band(100, 119)]
    draws = make_draws(60, 4, bands)
    table = draws.pack_band()
    assert table.dtype == np.int32 and table.shape == (band_ints(3),) == (BAND_INTS * 3,) == (12,)
    assert np.array_equal(table, R.pack(bands))
    recs = table.reshape(3, 4)
    assert recs[:, 0].tolist() == [800, 0, bands[2][0]] and bands[2][0] == 6 and not recs[:, 3].any()
    assert recs[0, 1:3].view(np.float32).tolist() == [bands[0][1], bands[0][2]]
    assert np.array_equal(draws.without_band().pack(), draws.pack()) and not draws.without_band().banded
    base = AR.make_draws(60, 4, [0, 1, 2])
    args = (60, 4, base.perm, base.off_clean, base.off_noise, base.snr_db, base.gain, base.kappa, base.n_taps, base.delay,
            base.tap_gain)
    for bad in ([1601, 0, 0], [-1, 0, 0], [3, 3]):
        with pytest.raises(ValueError):
            AugmentDraws(*args, bad, np.zeros(len(bad)), np.zeros(len(bad)))
    for lo, hi in (([0.3] * 3, [0.2] * 3), ([0.1] * 3, [0.6] * 3), ([-0.1] * 3, [0.2] * 3), ([np.nan] * 3, [0.2] * 3),
                   ([0.1] * 3, [np.inf] * 3)):
        with pytest.raises(ValueError):
            AugmentDraws(*args, [5, 5, 5], lo, hi)


def make_draws(L, S, bands, **kw):
    """AugmentDraws of augment_ref.make_draws with per-row bands (W, c_lo, c_hi)."""
    from cleanumamba_amd.training.augment import AugmentDraws
    d = AR.make_draws(L, S, kw.pop("perm", list(range(len(bands)))), **kw)
    return AugmentDraws(L, S, d.perm, d.off_clean, d.off_noise, d.snr_db, d.gain, d.kappa, d.n_taps, d.delay, d.tap_gain,
                        *zip(*bands))


@pytest.mark.parametrize("form", ["flat", "three"])
def test_band_mask_on_cpu_tensors_meets_the_oracle(form):
    """Rows shorter and longer than the filter; the W = 0 row is a copy.  The host path is a direct f32 convolution: its
    constant is the tap count, not the FFT's."""
    from cleanumamba_amd.training.augment import band_mask
    bands = [R.band(0, 23), R.band(60, 80), (0, 0.0, 0.0), R.band(119, 119)]
    for n in (7, 500, 2001):
        C, Y = R.case_signals(n, 4, seed=n)
        ref = R.reference(C, Y, bands)
        c_src, y_src = torch.from_numpy(C), torch.from_numpy(Y)
        if form == "three":
            c_src, y_src = c_src[:, None], y_src[:, None]
        clean, noisy = band_mask(c_src, y_src, make_draws(n - 3, 3, bands))
        assert clean.shape == c_src.shape
        R.check(clean.reshape(4, n).numpy(), ref[0], ref[2], f"cpu clean n = {n}", c=direct_c(bands))
        R.check(noisy.reshape(4, n).numpy(), ref[1], ref[3], f"cpu noisy n = {n}", c=direct_c(bands))
        assert torch.equal(clean.reshape(4, n)[2], torch.from_numpy(C[2]))
        assert torch.equal(noisy.reshape(4, n)[2], torch.from_numpy(Y[2]))


def test_apply_on_cpu_tensors_runs_the_band_first():
    from cleanumamba_amd.training.augment import apply, band_mask
    L, S = 900, 30
    bands = [R.band(5, 20), R.band(100, 119), (0, 0.0, 0.0)]
    draws = make_draws(L, S, bands, perm=[2, 0, 1], off_clean=[1, 30, 0], off_noise=[29, 2, 4], snr_db=[5.0, np.nan, -3.0],
                       gain=[0.5, 1.0, 1.7], taps=[[(3, 0.4), (40, -0.2)], [], [(1, 0.3)]])
    C, Y = (torch.from_numpy(x) for x in R.case_signals(L + S, 3, seed=4))
    got = apply(C, Y, draws)
    want = apply(*band_mask(C, Y, draws), draws.without_band())
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    plain = apply(C, Y, draws.without_band())
    assert not torch.equal(got[0], plain[0])


def test_cpu_feeder_with_a_band_equals_apply_on_its_unaugmented_crops(tmp_path):
    from cleanumamba_amd.training.augment import Augment, BandMask, apply
    from cleanumamba_amd.training.feeder import BatchFeeder
    from cleanumamba_amd.util.dataset import CleanNoisyPairDataset
    root, crop, shift = str(tmp_path), 1500, 21
    pairs = wavtree.training_tree(root, [1200, 4000, 1521, 2500], seed=60)
    ds = CleanNoisyPairDataset(root=root, subset="training", crop_length_sec=crop / 16000)
    for config in (dict(band_mask=BandMask()), dict(remix=True, shift=shift, gain_db=(-6, 3), band_mask=BandMask())):
        augment = Augment(**config)
        with BatchFeeder(ds, 2, "cpu", crop_length=crop, seed=2, augment=augment) as feeder:
            s = augment.shift
            assert feeder._dev[0].flat.numel() == 2 * 2 * feeder.pitch + 2 * 2 + 2 * (2 * 8 + 2 * 4)
            n = 0
            for batch in feeder:
                assert batch.draws.banded and len(set(batch.draws.band_half.tolist())) == 1
                clean, noisy = batch.tensors()
                C, Y = expected_batch(pairs, batch.entries, crop + s)
                want = apply(C, Y, batch.draws)
                assert torch.equal(clean, want[0]) and torch.equal(noisy, want[1])
                assert not torch.equal(clean, apply(C, Y, batch.draws.without_band())[0])
                n += 1
            assert n == 2


def band_argument_errors():
    """Every rejected argument set of cum_band_mask_pairs returns CUM_EINVAL with a text, before any launch."""
    from cleanumamba_amd import hip
    lib = hip.lib()
    P = ctypes.c_void_p
    ok = dict(clean_src=P(0x1000), clean_src_sb=24, noisy_src=P(0x2000), noisy_src_sb=20, batch=2, n=20, recs=P(0x3000),
              workspace=P(0x6000), clean=P(0x7000), clean_sb=20, noisy=P(0x8000), noisy_sb=24)
    bad = [("batch", 0, b"batch"), ("batch", 32768, b"batch"), ("n", 0, b"n must"), ("clean_src_sb", 19, b"src_sb"),
           ("noisy_src_sb", 19, b"src_sb"), ("clean_sb", 19, b"clean_sb"), ("noisy_sb", 19, b"noisy_sb"),
           ("clean_src", None, b"null"), ("noisy_src", None, b"null"), ("recs", None, b"null"),
           ("workspace", None, b"null"), ("clean", None, b"null"), ("noisy", None, b"null"),
           ("clean", P(0x7004), b"16-byte"), ("noisy", P(0x8008), b"16-byte"), ("workspace", P(0x6004), b"8-byte"),
           ("clean_src", P(0x1002), b"4-byte"), ("noisy_src", P(0x2001), b"4-byte"), ("recs", P(0x3002), b"4-byte")]
    for name, value, text in bad:
        args = dict(ok, **{name: value})
        rc = lib.cum_band_mask_pairs(*args.values(), None)
        assert rc == -1, (name, value)
        assert text in lib.cum_last_error(), (name, value, lib.cum_last_error())
    N = lib.cum_band_mask_block()
    assert N in (4096, 8192)
    assert lib.cum_band_mask_workspace_elems(0) == 0
    per_row = lib.cum_band_mask_workspace_elems(2) - lib.cum_band_mask_workspace_elems(1)
    assert per_row == 2 * N and lib.cum_band_mask_workspace_elems(1) >= 2 * N + 2 * (N + 1)
    assert lib.cum_abi_version() == 16


def test_band_argument_errors_need_no_gpu():
    band_argument_errors()
    from cleanumamba_amd.training.augment import band_mask
    C, Y = (torch.from_numpy(x) for x in R.case_signals(64, 2, seed=1))
    draws = make_draws(60, 4, [R.band(100, 119)] * 2)
    with pytest.raises(ValueError):
        band_mask(C, Y, draws, C, None)                  # an output over a source
    with pytest.raises(ValueError):
        band_mask(C[:, :60], Y, draws)                   # not L + S long
    with pytest.raises(ValueError):
        band_mask(C.double(), Y, draws)
