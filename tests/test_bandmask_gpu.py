"""csrc/bandmask.hip (cum_band_mask_pairs) through ``training.augment.band_mask`` / ``apply`` against the f64 oracle of
bandmask_ref.py, and the augmenting BatchFeeder with a band mask on the device.

Every output meets ``|out - ref| <= (c + 1) 2^-24 s_b`` with c = bandmask_ref.C = 20: four times the worst constant,
4.99, that a float32 overlap-save on pocketfft at the same N = 4096 gives over exactly these cases (bandmask_ref.C_CPU,
``python tests/bandmask_ref.py``); the kernel's own worst over them is 3.9.  A seam, halo or alignment mistake is an error of the order of s_b itself.  N is
``cum_band_mask_block()`` and V = N - 2 W per row; the seams are placed with them."""
import numpy as np
import pytest
import torch

import bandmask_ref as R
import wavtree
from test_augment_gpu import CROP, LENGTHS, SHIFT, TINY, _dataset, h2d_copies, leave_global_state_as_found  # noqa: F401
from test_bandmask_host import band_argument_errors, make_draws
from test_feeder_rates_host import MODEL, mixed_tree

pytestmark = pytest.mark.gpu

SENTINEL = 7.0


@pytest.fixture(scope="module")
def block():
    from cleanumamba_amd import hip
    N = hip.lib().cum_band_mask_block()
    assert N == 4096, "bandmask_ref.C_CPU was measured at N = 4096: measure it again at the new block length"
    return N


def _run(cuda, C, Y, bands, form="gaps"):
    """band_mask() into guarded buffers, twice.  form "gaps": (B, n) rows in pitches above n, odd, so that the rows fall
    on every 4-byte phase, the sources' gaps NaN and the outputs' gaps a sentinel; "flat": (B, n) rows n apart; "three":
    (B, 1, n).  Returns (clean, noisy) as (B, n) numpy."""
    from cleanumamba_amd.training.augment import band_mask
    B, n = C.shape
    draws = make_draws(n, 0, bands)
    if form == "gaps":
        src = torch.full((2, B, n + 5 + (n & 1)), float("nan"), device=cuda)
        src[0, :, :n], src[1, :, :n] = torch.from_numpy(C).to(cuda), torch.from_numpy(Y).to(cuda)
        c_src, y_src = src[0, :, :n], src[1, :, :n]
        pitch = n + 7 + (n & 1)                          # odd, like the sources' n + 5 + (n & 1)
        buf = torch.full((2, (B * pitch + 3) // 4 * 4 + 4), SENTINEL, device=cuda)     # (both halves on the 16-byte grid)
        clean, noisy = (buf[i, :B * pitch].view(B, pitch)[:, :n] for i in range(2))
    else:
        c_src, y_src = torch.from_numpy(C).to(cuda), torch.from_numpy(Y).to(cuda)
        buf = torch.full((2, (B * n + 3) // 4 * 4 + 8), SENTINEL, device=cuda)
        clean, noisy = buf[0, :B * n].view(B, n), buf[1, :B * n].view(B, n)
        if form == "three":
            c_src, y_src, clean, noisy = c_src[:, None], y_src[:, None], clean[:, None], noisy[:, None]
    band_mask(c_src, y_src, draws, clean, noisy)
    torch.cuda.synchronize()
    first = buf.clone()
    band_mask(c_src, y_src, draws, clean, noisy)
    torch.cuda.synchronize()
    assert torch.equal(buf, first), "two runs differ"
    mask = torch.ones_like(buf, dtype=torch.bool)
    for i, t in enumerate((clean, noisy)):
        view = torch.as_strided(mask[i], (B, n), (t.stride(0) if B > 1 else n, 1))
        view[:] = False
    assert (buf[mask] == SENTINEL).all(), "a store outside the rows"
    assert torch.equal(c_src.reshape(B, n).cpu(), torch.from_numpy(C)), "the sources were written"
    return clean.reshape(B, n).cpu().numpy(), noisy.reshape(B, n).cpu().numpy()


def _check(got, C, Y, bands, what):
    rc, ry, sc, sy = R.reference(C, Y, bands)
    worst = max(R.check(got[0], rc, sc, f"{what} clean"), R.check(got[1], ry, sy, f"{what} noisy"))
    for b, (W, _, _) in enumerate(bands):
        if W == 0:
            assert np.array_equal(got[0][b], C[b]) and np.array_equal(got[1][b], Y[b]), "the W = 0 row is no copy"
    return worst


@pytest.mark.parametrize("which", range(len(R.BANDS)), ids=[f"band{lo}_{hi}" for lo, hi in R.BANDS])
def test_seam_and_edge_lengths(cuda, block, which):
    """n in {1, 7, W, V - 1, V, V + 1, 2 V + 1, 3 V + 5} of the band, every launch with one row of each band and a W = 0
    row, rows in strides above n with NaN between them."""
    lo, hi = R.BANDS[which]
    cases = [c for c in R.seam_cases(block) if c[0].startswith(f"band ({lo}, {hi}) ")]
    W = R.band(lo, hi)[0]
    assert [c[1] for c in cases] == R.seam_lengths(W, block) and len(cases) == 8
    for name, n, bands, seed in cases:
        assert len({b[0] for b in bands}) == len(R.BANDS) + 1            # every band's own W, and the W = 0 row
        C, Y = R.case_signals(n, len(bands), seed)
        _check(_run(cuda, C, Y, bands), C, Y, bands, name)


@pytest.mark.parametrize("lo,hi", R.IMPULSE_BANDS)
def test_impulses_return_the_taps(cuda, block, lo, hi):
    """A unit impulse at t in {0, V - 1, V, n - 1}: row r is the taps centred on its t, each within the bound of the
    oracle's; the noisy row carries -0.5 of them (an exact scale)."""
    n, bands, pos, C, Y = R.impulse_case(lo, hi, block)
    W = bands[0][0]
    clean, noisy = _run(cuda, C, Y, bands)
    _check((clean, noisy), C, Y, bands, f"impulses ({lo}, {hi})")
    h = R.taps(*bands[0])
    bound = (R.C + 1) * R.U * np.abs(h).sum()
    for r, t in enumerate(pos):
        want = np.zeros(n)
        a, b = max(0, t - W), min(n, t + W + 1)
        want[a:b] = h[a - t + W:b - t + W]
        assert np.abs(clean[r] - want).max() <= bound and np.abs(noisy[r] + 0.5 * want).max() <= 0.5 * bound, (r, t)
        assert abs(clean[r, t] - h[W]) <= bound


def test_both_forms(cuda, block):
    bands = [R.band(5, 20), R.band(60, 80), (0, 0.0, 0.0)]
    n = block - 2 * bands[0][0] + 1
    C, Y = R.case_signals(n, 3, seed=5)
    flat = _run(cuda, C, Y, bands, "flat")
    three = _run(cuda, C, Y, bands, "three")
    _check(flat, C, Y, bands, "flat")
    assert np.array_equal(flat[0], three[0]) and np.array_equal(flat[1], three[1])


def test_largest_filter(cuda, block):
    """W = 1600, which the default edges never draw: V = N - 3200 at n = 2 V + 1."""
    name, n, bands, seed = R.largest_case(block)
    assert bands[0][0] == 1600 and n == 2 * (block - 3200) + 1
    C, Y = R.case_signals(n, len(bands), seed)
    _check(_run(cuda, C, Y, bands), C, Y, bands, name)


def test_a_row_does_not_depend_on_its_batch(cuda, block):
    bands = [R.band(0, 23), R.band(5, 20), R.band(60, 80), (0, 0.0, 0.0), R.band(100, 119)]
    n = 2 * (block - 2 * bands[0][0]) + 1
    C, Y = R.case_signals(n, 5, seed=9)
    together = _run(cuda, C, Y, bands)                   # (_run itself runs twice and compares the bits)
    for b in (0, 2, 4):
        alone = _run(cuda, C[b:b + 1], Y[b:b + 1], bands[b:b + 1], "flat")
        assert np.array_equal(alone[0][0], together[0][b]) and np.array_equal(alone[1][0], together[1][b]), b


def test_bad_records_are_copies(cuda, block):
    """A cutoff that is not finite or out of order makes the row a copy; W is clamped to 1600."""
    from cleanumamba_amd import hip
    from cleanumamba_amd.training.augment import band_workspace_for
    n = 300
    C, Y = R.case_signals(n, 5, seed=12)
    e = R.mel_edges()
    recs = R.pack([(50, np.nan, 0.2), (50, 0.3, 0.2), (50, 0.1, np.inf), (50, -0.1, 0.2), (5000, e[0], e[23])])
    c_src, y_src = torch.from_numpy(C).to(cuda), torch.from_numpy(Y).to(cuda)
    clean, noisy = torch.empty_like(c_src), torch.empty_like(y_src)
    table, workspace = torch.from_numpy(recs).to(cuda), band_workspace_for(5, cuda)
    hip.check(hip.lib().cum_band_mask_pairs(hip.ptr(c_src), n, hip.ptr(y_src), n, 5, n, hip.ptr(table), hip.ptr(workspace),
                                            hip.ptr(clean), n, hip.ptr(noisy), n, hip.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(clean[:4], c_src[:4]) and torch.equal(noisy[:4], y_src[:4])
    bands = [(0, 0.0, 0.0)] * 4 + [(1600, e[0], e[23])]
    _check((clean.cpu().numpy(), noisy.cpu().numpy()), C, Y, bands, "clamped W")


def test_apply_is_the_band_stage_then_the_rest(cuda):
    """apply(C, Y, draws with a band) == apply(*band_mask(C, Y, draws), the draws without it), bit for bit, with remix,
    shift, SNR, gain and echo on; B = 4, L = 3000, S = 500."""
    from cleanumamba_amd.training.augment import Augment, AugmentDraws, BandMask, Echo, apply, band_mask
    L, S = 3000, 500
    config = Augment(remix=True, shift=S, snr_db=(-5, 15), gain_db=(-6, 3), echo=Echo(rt60=(0.05, 0.1)),
                     band_mask=BandMask())
    d = config.draw(np.random.default_rng(3), 4, L)
    assert d.banded and d.rescales and int(d.n_taps.min()) > 0
    rows = [R.band(0, 23), R.band(60, 80), (0, 0.0, 0.0), (int(d.band_half[0]), d.band_lo[0], d.band_hi[0])]
    d = AugmentDraws(L, S, d.perm, d.off_clean, d.off_noise, d.snr_db, d.gain, d.kappa, d.n_taps, d.delay, d.tap_gain,
                     *zip(*rows))
    C, Y = (torch.from_numpy(x).to(cuda) for x in R.case_signals(L + S, 4, seed=31))
    got = apply(C, Y, d)
    fc, fy = band_mask(C, Y, d)
    want = apply(fc, fy, d.without_band())
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(got[0], apply(C, Y, d.without_band())[0])
    _check((fc.cpu().numpy(), fy.cpu().numpy()), C.cpu().numpy(), Y.cpu().numpy(), rows, "composition, the stage")


def test_argument_errors_return_the_error_code_without_a_launch(cuda):
    band_argument_errors()
    from cleanumamba_amd.training.augment import band_mask
    C, Y = (torch.from_numpy(x).to(cuda) for x in R.case_signals(64, 2, seed=1))
    draws = make_draws(60, 4, [R.band(100, 119)] * 2)
    with pytest.raises(ValueError):
        band_mask(C, Y, draws, C, None)                  # an output over a source
    with pytest.raises(RuntimeError):
        band_mask(C, Y, draws, torch.empty(2, 65, device=cuda)[:, 1:], None)     # off the 16-byte grid: the library's -1
    torch.cuda.synchronize()


# ---- the feeder ---------------------------------------------------------------------------------------------------------
def _augment():
    from cleanumamba_amd.training.augment import Augment, BandMask, Echo
    return Augment(remix=True, shift=SHIFT, snr_db=(-5, 15), gain_db=(-6, 3), echo=Echo(rt60=(0.05, 0.1)),
                   band_mask=BandMask())


def test_feeder_batch_equals_apply_on_the_unaugmented_crops(cuda, tmp_path, h2d_copies):  # noqa: F811
    """The augmenting feeder's batch with a band == apply() on the L + S tensors of a plain feeder with the same plan, bit
    for bit, with one host-to-device copy per batch; and the same with nothing but the band on."""
    from cleanumamba_amd.training.augment import Augment, BandMask, apply, band_ints, table_ints
    from cleanumamba_amd.training.feeder import BatchFeeder
    root = str(tmp_path)
    wavtree.training_tree(root, LENGTHS, seed=100)
    ds = _dataset(root)
    for augment in (_augment(), Augment(band_mask=BandMask())):
        shift = augment.shift
        with BatchFeeder(ds, 4, cuda, crop_length=CROP, seed=9, augment=augment) as feeder:
            assert feeder._dev[0].flat.numel() == 2 * 4 * feeder.pitch + 2 * 4 + 2 * (
                table_ints(4, augment.max_taps) + band_ints(4))
            before = len(h2d_copies)
            got = [(b.entries, b.draws, b.tensors()) for b in feeder]
            torch.cuda.synchronize()
            assert len(got) == 2 and len(h2d_copies) - before == feeder._uploaded in (2, 3), h2d_copies[before:]
            assert {n for _, n in h2d_copies[before:]} == {feeder._dev[0].flat.numel()}
        with BatchFeeder(ds, 4, cuda, crop_length=CROP + shift, seed=9) as longer:
            for (entries, draws, (clean, noisy)), plain in zip(got, longer):
                assert entries == plain.entries and clean.shape == (4, 1, CROP) and draws.banded
                C, Y = plain.tensors()
                want = apply(C, Y, draws)
                assert torch.equal(clean, want[0]) and torch.equal(noisy, want[1])
                assert not torch.equal(clean, apply(C, Y, draws.without_band())[0])


def test_rated_feeder_batch_equals_apply_on_the_unaugmented_crops(cuda, tmp_path):
    from cleanumamba_amd.training.augment import apply
    from cleanumamba_amd.training.feeder import BatchFeeder
    root = str(tmp_path)
    mixed_tree(root, [(16000, 9000), (48000, 30000), (16000, 3000), (16000, 5000)], seed=40)
    ds = _dataset(root)
    with BatchFeeder(ds, 2, cuda, crop_length=CROP, seed=6, sample_rate=MODEL, augment=_augment()) as feeder, \
            BatchFeeder(ds, 2, cuda, crop_length=CROP + SHIFT, seed=6, sample_rate=MODEL) as longer:
        n = 0
        for batch, plain in zip(feeder, longer):
            assert batch.entries == plain.entries and batch.windows == plain.windows and batch.draws.banded
            want = apply(*plain.tensors(), batch.draws)
            clean, noisy = batch.tensors()
            assert torch.equal(clean, want[0]) and torch.equal(noisy, want[1])
            n += 1
        assert n == 2


def test_captured_step_replays_on_a_feeder_with_a_band(cuda, tmp_path):
    from cleanumamba_amd.network import CleanUMamba
    from cleanumamba_amd.training.feeder import BatchFeeder
    from cleanumamba_amd.training.train_step import TrainStep
    from cleanumamba_amd.util.dataset import CleanNoisyPairDataset
    root = str(tmp_path)
    wavtree.training_tree(root, [9000, 12000, 8000, 16000, 10000, 5000], seed=7)
    torch.manual_seed(0)
    net = CleanUMamba(**TINY).to(cuda).train()
    step = TrainStep(net, optimization={"n_iters": 200}, use_graph=True)
    ds = CleanNoisyPairDataset(root=root, subset="training", crop_length_sec=0.5)
    losses = []
    with BatchFeeder(ds, 2, cuda, crop_length=8000, seed=1, augment=_augment()) as feeder:
        while len(losses) < 8:
            for batch in feeder:
                loss, _ = step(batch)
                losses.append(float(loss))
                last = batch
                if len(losses) == 8:
                    break
        assert step.graph_status == "captured", step.graph_status
        clean, noisy = last.tensors()                    # the last step was a replay: the graph's input is the batch
        assert torch.equal(step._graph["clean"], clean) and torch.equal(step._graph["noisy"], noisy)
    assert all(np.isfinite(l) for l in losses) and len(set(losses)) == len(losses), losses
