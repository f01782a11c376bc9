"""csrc/reverb.hip (cum_reverb_pairs) through ``training.augment.reverb`` / ``apply`` against the f64 oracle of
reverb_ref.py, and the augmenting BatchFeeder with a reverb on the device.

Every clean output meets ``|out - ref| <= c 2^-24 s_b`` and every noisy one ``(c + 1) 2^-24 s_b + 2^-23 max |Y - C|`` with
c = reverb_ref.C = 15: four times the worst constant, 3.54, that a float32 partitioned overlap-save on pocketfft at the
same N = 4096 gives over exactly these cases (reverb_ref.C_CPU, ``python tests/reverb_ref.py``).  A seam, partition-order
or halo mistake is an error of the order of the signal itself.  N is ``cum_reverb_block()``, P = N / 2; the seams are
placed with them."""
import numpy as np
import pytest
import torch

import reverb_ref as R
import wavtree
from test_augment_gpu import CROP, LENGTHS, SHIFT, TINY, _dataset, h2d_copies, leave_global_state_as_found  # noqa: F401
from test_feeder_rates_host import MODEL, mixed_tree
from test_reverb_host import make_draws, reverb_argument_errors

pytestmark = pytest.mark.gpu

SENTINEL = 7.0


@pytest.fixture(scope="module")
def room():
    """The ``Reverb`` over reverb_ref's bank: one response of every length of R.TAPS, every tap kept."""
    from cleanumamba_amd import hip
    from cleanumamba_amd.training.augment import Reverb
    N = hip.lib().cum_reverb_block()
    assert N == 4096 == R.N, "reverb_ref.C_CPU was measured at N = 4096: measure it again at the new block length"
    assert hip.lib().cum_reverb_max_taps() == R.T_MAX
    rv = Reverb(R.bank_raw(), proba=1.0, decay_db=R.DECAY)
    assert [h.shape[0] for h in rv.taps] == R.TAPS
    assert all(np.array_equal(a, b) for a, b in zip(rv.taps, R.bank()))
    return rv


def _taps(room, ids):
    return [room.taps[r] if 0 <= r < len(room) else None for r in ids]


def _run(cuda, room, C, Y, ids, form="gaps"):
    """reverb() into guarded buffers, twice.  form "gaps": (B, n) rows in pitches above n, odd, so that the rows fall on
    every 4-byte phase, the sources' gaps NaN and the outputs' gaps a sentinel; "flat": (B, n) rows n apart; "three":
    (B, 1, n); "strided": every second row of (2 B, n + 3) buffers.  Returns (clean, noisy) as (B, n) numpy."""
    from cleanumamba_amd.training.augment import reverb
    B, n = C.shape
    draws = make_draws(n, 0, ids)
    bank = room.bank(cuda)
    if form == "gaps":
        src = torch.full((2, B, n + 5 + (n & 1)), float("nan"), device=cuda)
        src[0, :, :n], src[1, :, :n] = torch.from_numpy(C).to(cuda), torch.from_numpy(Y).to(cuda)
        c_src, y_src = src[0, :, :n], src[1, :, :n]
        pitch = n + 7 + (n & 1)                          # odd, like the sources' n + 5 + (n & 1)
        buf = torch.full((2, (B * pitch + 3) // 4 * 4 + 4), SENTINEL, device=cuda)     # (both halves on the 16-byte grid)
        clean, noisy = (buf[i, :B * pitch].view(B, pitch)[:, :n] for i in range(2))
    elif form == "strided":
        src = torch.full((2, 2 * B, n + 3), float("nan"), device=cuda)
        src[0, ::2, :n], src[1, ::2, :n] = torch.from_numpy(C).to(cuda), torch.from_numpy(Y).to(cuda)
        c_src, y_src = src[0, ::2, :n], src[1, ::2, :n]
        pitch = n + 3
        buf = torch.full((2, (2 * B * pitch + 3) // 4 * 4 + 4), SENTINEL, device=cuda)
        clean, noisy = (buf[i, :2 * B * pitch].view(2 * B, pitch)[::2, :n] for i in range(2))
    else:
        c_src, y_src = torch.from_numpy(C).to(cuda), torch.from_numpy(Y).to(cuda)
        buf = torch.full((2, (B * n + 3) // 4 * 4 + 8), SENTINEL, device=cuda)
        clean, noisy = buf[0, :B * n].view(B, n), buf[1, :B * n].view(B, n)
        if form == "three":
            c_src, y_src, clean, noisy = c_src[:, None], y_src[:, None], clean[:, None], noisy[:, None]
    reverb(c_src, y_src, draws, bank, clean, noisy)
    torch.cuda.synchronize()
    first = buf.clone()
    reverb(c_src, y_src, draws, bank, clean, noisy)
    torch.cuda.synchronize()
    assert torch.equal(buf, first), "two runs differ"
    mask = torch.ones_like(buf, dtype=torch.bool)
    for i, t in enumerate((clean, noisy)):
        view = torch.as_strided(mask[i], (B, n), (t.stride(0) if B > 1 else n, 1))
        view[:] = False
    assert (buf[mask] == SENTINEL).all(), "a store outside the rows"
    assert torch.equal(c_src.reshape(B, n).cpu(), torch.from_numpy(C)), "the sources were written"
    assert torch.equal(y_src.reshape(B, n).cpu(), torch.from_numpy(Y)), "the sources were written"
    return clean.reshape(B, n).cpu().numpy(), noisy.reshape(B, n).cpu().numpy()


@pytest.mark.parametrize("which", range(len(R.TAPS)), ids=[f"T{T}" for T in R.TAPS])
def test_seam_and_edge_lengths(cuda, room, which):
    """n in {1, 7, P - 1, P, P + 1, 2 P + 1, 3 P + 5} for the response of T taps, every launch with the rows of three
    different responses and a -1 row, rows in strides above n with NaN between them: T > n, T = 1 (a scaled copy), and a
    partition boundary that falls on a block boundary are all here."""
    T = R.TAPS[which]
    cases = [c for c in R.seam_cases() if c[0].startswith(f"T = {T} ")]
    assert [c[1] for c in cases] == R.LENGTHS and len(cases) == 7
    for name, n, ids, seed in cases:
        assert ids[0] == which and len(set(ids)) == 4 and ids[3] == -1
        C, Y = R.case_signals(n, len(ids), seed)
        R.check(_run(cuda, room, C, Y, ids), C, Y, _taps(room, ids), name)


@pytest.mark.parametrize("r", R.IMPULSE_RIRS)
def test_impulses_return_the_taps(cuda, room, r):
    """A unit impulse at t in {0, P - 1, P, n - 1}: the clean row is the taps from t on, each within the bound; the noisy
    row, built as Y = C + N with a known N, is N + the taps."""
    n, ids, pos, C, Y, noise = R.impulse_case(r)
    clean, noisy = _run(cuda, room, C, Y, ids)
    R.check((clean, noisy), C, Y, _taps(room, ids), f"impulses of response {r}")
    h = room.taps[r].astype(np.float64)
    s = np.abs(h).sum()
    for row, t in enumerate(pos):
        want = np.zeros(n)
        m = min(n - t, h.shape[0])
        want[t:t + m] = h[:m]
        assert np.abs(clean[row] - want).max() <= R.C * R.U * s, (row, t)
        assert np.abs(noisy[row] - (noise[row] + want)).max() <= (R.C + 1) * R.U * s + 2 * R.U * np.abs(noise[row]).max()


def test_a_row_does_not_depend_on_its_batch(cuda, room):
    ids = [7, 3, 5, -1, 0]
    n = 2 * R.P + 1
    C, Y = R.case_signals(n, 5, seed=9)
    together = _run(cuda, room, C, Y, ids)               # (_run itself runs twice and compares the bits)
    for b in (0, 2, 4):
        alone = _run(cuda, room, C[b:b + 1], Y[b:b + 1], ids[b:b + 1], "flat")
        assert np.array_equal(alone[0][0], together[0][b]) and np.array_equal(alone[1][0], together[1][b]), b


def test_the_forms_agree(cuda, room):
    name, n, ids, seed = R.OTHER_CASES["forms"]
    C, Y = R.case_signals(n, 3, seed)
    flat = _run(cuda, room, C, Y, ids, "flat")
    R.check(flat, C, Y, _taps(room, ids), name)
    for form in ("three", "strided", "gaps"):
        other = _run(cuda, room, C, Y, ids, form)
        assert np.array_equal(flat[0], other[0]) and np.array_equal(flat[1], other[1]), form


def test_bad_records_are_copies(cuda, room):
    """Ids R, -1, -7 and 2^30 are copies, beside a row that is not."""
    name, n, good, seed = R.OTHER_CASES["bad ids"]
    ids = [len(room), -1, -7, 2 ** 30, 2]
    C, Y = R.case_signals(n, 5, seed)
    got = _run(cuda, room, C, Y, ids)
    assert np.array_equal(got[0][:4], C[:4]) and np.array_equal(got[1][:4], Y[:4])
    R.check(got, C, Y, _taps(room, good), name)


def test_a_bad_device_table_is_clamped(cuda, room):
    """The device table is not trusted: taps above T_MAX are clamped to it, taps below 1 to 1, an offset outside the bank
    makes the row a copy.  Called through the library with a good host table, so that the check before the launch passes."""
    import ctypes
    from cleanumamba_amd import hip
    from cleanumamba_amd.training.augment import reverb_workspace_for
    bank = room.bank(cuda)
    name, n, good, seed = R.OTHER_CASES["bad device table"]
    ids = [7, 1, 0, 3]
    C, Y = R.case_signals(n, 4, seed)
    table = bank.table_host.copy()
    table[7, 2] = 5 * R.T_MAX                            # response 7 is the bank's last: T_MAX taps are all there are
    table[1].view(np.int64)[0] = bank.blob.numel() + 4   # outside the bank: a copy
    table[0, 2] = -3                                     # one tap
    table[3].view(np.int64)[0] = -8                      # in front of the bank: a copy
    c_src, y_src = torch.from_numpy(C).to(cuda), torch.from_numpy(Y).to(cuda)
    clean, noisy = torch.empty_like(c_src), torch.empty_like(y_src)
    recs, dev_table = torch.from_numpy(R.pack(ids)).to(cuda), torch.from_numpy(table).to(cuda)
    workspace = reverb_workspace_for(4, n, cuda)
    hip.check(hip.lib().cum_reverb_pairs(hip.ptr(c_src), n, hip.ptr(y_src), n, 4, n, hip.ptr(recs), hip.ptr(bank.blob),
                                         bank.blob.numel(), ctypes.c_void_p(bank.table_host.ctypes.data),
                                         hip.ptr(dev_table), len(bank), hip.ptr(workspace),
                                         hip.ptr(clean), n, hip.ptr(noisy), n, hip.stream_ptr()))
    torch.cuda.synchronize()
    R.check((clean.cpu().numpy(), noisy.cpu().numpy()), C, Y, _taps(room, good), name)


def test_apply_is_the_reverb_stage_then_the_band_then_the_rest(cuda, room):
    """apply() with reverb, band, remix, shift, SNR, gain and echo all on == stage -> band_mask -> apply(without both),
    bit for bit; B = 4, L = 3000, S = 500."""
    import bandmask_ref as BR
    from cleanumamba_amd.training.augment import Augment, AugmentDraws, BandMask, Echo, apply, band_mask, reverb
    L, S = 3000, 500
    config = Augment(remix=True, shift=S, snr_db=(-5, 15), gain_db=(-6, 3), echo=Echo(rt60=(0.05, 0.1)),
                     band_mask=BandMask(), reverb=room)
    d = config.draw(np.random.default_rng(3), 4, L)
    assert d.banded and d.rescales and d.reverberant and int(d.n_taps.min()) > 0 and (d.rir >= 0).all()
    rows = [BR.band(0, 23), BR.band(60, 80), (0, 0.0, 0.0), (int(d.band_half[0]), d.band_lo[0], d.band_hi[0])]
    name, n, ids, seed = R.OTHER_CASES["composition"]
    assert n == L + S
    d = AugmentDraws(L, S, d.perm, d.off_clean, d.off_noise, d.snr_db, d.gain, d.kappa, d.n_taps, d.delay, d.tap_gain,
                     *zip(*rows), rir=ids)
    C, Y = (torch.from_numpy(x).to(cuda) for x in R.case_signals(L + S, 4, seed))
    got = apply(C, Y, d, reverb=room)
    rc, ry = reverb(C, Y, d, room.bank(cuda))
    fc, fy = band_mask(rc, ry, d)
    want = apply(fc, fy, d.without_band().without_reverb())
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(got[0], apply(C, Y, d.without_reverb())[0])
    with pytest.raises(ValueError, match="reverb"):
        apply(C, Y, d)
    R.check((rc.cpu().numpy(), ry.cpu().numpy()), C.cpu().numpy(), Y.cpu().numpy(), _taps(room, ids), name)


def test_argument_errors_return_the_error_code_without_a_launch(cuda, room):
    reverb_argument_errors()
    from cleanumamba_amd.training.augment import reverb
    C, Y = (torch.from_numpy(x).to(cuda) for x in R.case_signals(64, 2, seed=1))
    draws = make_draws(60, 4, [0, 1])
    with pytest.raises(ValueError):
        reverb(C, Y, draws, room.bank(cuda), C, None)    # an output over a source
    with pytest.raises(ValueError):
        reverb(C, Y, draws, room.bank("cpu"))            # the bank of another device
    with pytest.raises(RuntimeError):
        reverb(C, Y, draws, room.bank(cuda), torch.empty(2, 65, device=cuda)[:, 1:], None)   # off the 16-byte grid: -1
    torch.cuda.synchronize()


# ---- the feeder ---------------------------------------------------------------------------------------------------------
def _rooms():
    from cleanumamba_amd.training.augment import Reverb
    return Reverb([R.synth_raw(T, 80 + i) for i, T in enumerate((1, 300, 2049, 5000))], proba=0.7, decay_db=R.DECAY)


def _augment(rooms):
    from cleanumamba_amd.training.augment import Augment, BandMask, Echo
    return Augment(remix=True, shift=SHIFT, snr_db=(-5, 15), gain_db=(-6, 3), echo=Echo(rt60=(0.05, 0.1)),
                   band_mask=BandMask(), reverb=rooms)


def test_feeder_batch_equals_apply_on_the_unaugmented_crops(cuda, tmp_path, h2d_copies):  # noqa: F811
    """The augmenting feeder's batch with a reverb == apply(..., reverb=...) on the L + S tensors of a plain feeder with the
    same plan, bit for bit, with one host-to-device copy per batch; and the same with nothing but the reverb on."""
    from cleanumamba_amd.training.augment import Augment, apply, band_ints, reverb_ints, table_ints
    from cleanumamba_amd.training.feeder import BatchFeeder
    root = str(tmp_path)
    wavtree.training_tree(root, LENGTHS, seed=100)
    ds = _dataset(root)
    rooms = _rooms()
    for augment in (_augment(rooms), Augment(reverb=rooms)):
        shift = augment.shift
        with BatchFeeder(ds, 4, cuda, crop_length=CROP, seed=9, augment=augment) as feeder:
            tail = table_ints(4, augment.max_taps) + reverb_ints(4) + (band_ints(4) if augment.band_mask is not None else 0)
            assert feeder._dev[0].flat.numel() == 2 * 4 * feeder.pitch + 2 * 4 + 2 * tail
            before = len(h2d_copies)                     # (the bank went up at construction, in uploads of its own)
            got = [(b.entries, b.draws, b.tensors()) for b in feeder]
            torch.cuda.synchronize()
            assert len(got) == 2 and len(h2d_copies) - before == feeder._uploaded in (2, 3), h2d_copies[before:]
            assert {n for _, n in h2d_copies[before:]} == {feeder._dev[0].flat.numel()}
        rooms_seen = 0
        with BatchFeeder(ds, 4, cuda, crop_length=CROP + shift, seed=9) as longer:
            for (entries, draws, (clean, noisy)), plain in zip(got, longer):
                assert entries == plain.entries and clean.shape == (4, 1, CROP)
                C, Y = plain.tensors()
                want = apply(C, Y, draws, reverb=rooms)
                assert torch.equal(clean, want[0]) and torch.equal(noisy, want[1])
                if draws.reverberant:
                    rooms_seen += 1
                    assert not torch.equal(clean, apply(C, Y, draws.without_reverb())[0])
        assert rooms_seen >= 1


def test_rated_feeder_batch_equals_apply_on_the_unaugmented_crops(cuda, tmp_path):
    from cleanumamba_amd.training.augment import apply
    from cleanumamba_amd.training.feeder import BatchFeeder
    root = str(tmp_path)
    mixed_tree(root, [(16000, 9000), (48000, 30000), (16000, 3000), (16000, 5000)], seed=40)
    ds = _dataset(root)
    rooms = _rooms()
    with BatchFeeder(ds, 2, cuda, crop_length=CROP, seed=6, sample_rate=MODEL, augment=_augment(rooms)) as feeder, \
            BatchFeeder(ds, 2, cuda, crop_length=CROP + SHIFT, seed=6, sample_rate=MODEL) as longer:
        n, rooms_seen = 0, 0
        for batch, plain in zip(feeder, longer):
            assert batch.entries == plain.entries and batch.windows == plain.windows
            want = apply(*plain.tensors(), batch.draws, reverb=rooms)
            clean, noisy = batch.tensors()
            assert torch.equal(clean, want[0]) and torch.equal(noisy, want[1])
            rooms_seen += int(batch.draws.reverberant)
            n += 1
        assert n == 2 and rooms_seen >= 1


def test_captured_step_replays_on_a_reverberating_feeder(cuda, tmp_path):
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
    losses, rooms_seen = [], 0
    with BatchFeeder(ds, 2, cuda, crop_length=8000, seed=1, augment=_augment(_rooms())) as feeder:
        while len(losses) < 8:
            for batch in feeder:
                loss, _ = step(batch)
                losses.append(float(loss))
                rooms_seen += int(batch.draws.reverberant)
                last = batch
                if len(losses) == 8:
                    break
        assert step.graph_status == "captured", step.graph_status
        clean, noisy = last.tensors()                    # the last step was a replay: the graph's input is the batch
        assert torch.equal(step._graph["clean"], clean) and torch.equal(step._graph["noisy"], noisy)
    assert rooms_seen >= 1
    assert all(np.isfinite(l) for l in losses) and len(set(losses)) == len(losses), losses
