"""csrc/augment.hip (cum_augment_pairs) through ``training.augment.apply`` against the f64 oracle of augment_ref.py, and
the augmenting BatchFeeder on the device.  Every case meets the per-element bound ``(n_terms + 8) 2^-24 M`` and two runs
give the same bits."""
import numpy as np
import pytest
import torch

import augment_ref as R
import wavtree
from test_augment_host import augment_argument_errors
from test_feeder_host import expected_batch
from test_feeder_rates_host import MODEL, mixed_tree

pytestmark = pytest.mark.gpu

L, S = 4099, 37                      # three tiles of 2048 per row, a tail that is no multiple of 8, odd offsets
SENTINEL = 7.0


@pytest.fixture(autouse=True)
def leave_global_state_as_found():
    """Tests that run later draw from torch's global generators without seeding them: their states are put back."""
    cpu = torch.get_rng_state()
    gpu = torch.cuda.get_rng_state_all() if torch.cuda.is_available() else None
    yield
    torch.set_rng_state(cpu)
    if gpu is not None:
        torch.cuda.set_rng_state_all(gpu)


def _full_taps(seed, n=512, reach=L + 300):
    """n taps, delays over [1, reach): some reach behind the clip and are dropped."""
    rng = np.random.default_rng(seed)
    gains = rng.uniform(-1, 1, n) * 0.97 ** np.arange(n) * 0.3
    return [(int(d), float(g)) for d, g in zip(rng.integers(1, reach, n), gains)]


def _run(cuda, C, Y, draws, form):
    """apply() into guarded buffers.  form "flat": (B, L) rows L apart (off the 16-byte grid when L is odd); "padded":
    (B, 1, L) rows on the grid, a stride above L.  Returns (clean, noisy) as (B, L) numpy and checks the guards."""
    from cleanumamba_amd.training.augment import apply
    B, n = draws.batch, draws.length
    c_src, y_src = torch.from_numpy(C).to(cuda), torch.from_numpy(Y).to(cuda)
    if form == "flat":
        buf = torch.full((2, (B * n + 3) // 4 * 4 + 8), SENTINEL, device=cuda)        # (both halves on the 16-byte grid)
        clean, noisy = buf[0, :B * n].view(B, n), buf[1, :B * n].view(B, n)
    else:
        pitch = (n + 3) // 4 * 4 + 8
        buf = torch.full((2, B, 1, pitch), SENTINEL, device=cuda)
        clean, noisy = buf[0, :, :, :n], buf[1, :, :, :n]
        c_src, y_src = c_src[:, None], y_src[:, None]
    apply(c_src, y_src, draws, clean, noisy)
    torch.cuda.synchronize()
    first = buf.clone()
    apply(c_src, y_src, draws, clean, noisy)
    torch.cuda.synchronize()
    assert torch.equal(buf, first), "two runs differ"
    if form == "flat":
        assert (buf[:, B * n:] == SENTINEL).all()
    else:
        assert (buf[..., n:] == SENTINEL).all()
    assert torch.equal(c_src.reshape(B, -1).cpu(), torch.from_numpy(C))          # the sources were only read
    return clean.reshape(B, n).cpu().numpy(), noisy.reshape(B, n).cpu().numpy()


@pytest.fixture(scope="module")
def main_case():
    """B = 3, a permutation with a fixed point and a 2-cycle; a full list of 512 taps (some beyond the clip), an empty
    one and one tap of delay 1; SNR kept on one row; offsets that put the reads on 4-, 8- and 16-byte boundaries."""
    draws = R.make_draws(L, S, [0, 2, 1], off_clean=[1, 37, 0], off_noise=[36, 2, 4], snr_db=[5.0, np.nan, -3.25],
                         gain=[0.5, 1.0, 1.7], kappa=0.1, taps=[_full_taps(1), [], [(1, 0.3)]])
    C, Y = R.signals(3, L + S, seed=21)
    return C, Y, draws, R.reference(C, Y, draws)


@pytest.mark.parametrize("form", ["flat", "padded"])
def test_all_transforms_meet_the_bound(cuda, main_case, form):
    C, Y, draws, ref = main_case
    assert int(draws.n_taps[0]) == 512 and (draws.delay[0] >= L).any()
    clean, noisy = _run(cuda, C, Y, draws, form)
    R.check(clean, noisy, ref, f"main {form}")
    assert R.snr_check(clean, noisy, ref, draws) == 2


@pytest.mark.parametrize("form", ["flat", "padded"])
def test_one_launch_when_no_row_rescales(cuda, main_case, form):
    C, Y, draws, _ = main_case
    keep = R.make_draws(L, S, draws.perm, draws.off_clean, draws.off_noise, None, draws.gain, 0.1,
                        [list(zip(draws.delay[b, :n].tolist(), draws.tap_gain[b, :n].tolist()))
                         for b, n in enumerate(draws.n_taps)])
    assert not keep.rescales
    clean, noisy = _run(cuda, C, Y, keep, form)
    R.check(clean, noisy, R.reference(C, Y, keep), f"one launch {form}")


CASES = {
    "remix": dict(perm=[0, 2, 1]),
    "shift": dict(off_clean=[0, 37, 5], off_noise=[36, 1, 8]),
    "snr": dict(snr_db=[5.0, np.nan, -3.25]),
    "gain": dict(gain=[0.5, 1.0, 1.7]),
    "echo": dict(taps=[_full_taps(2, 51), [(L, 0.5), (L + 5, 0.5)], [(1, 0.3)]]),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_each_transform_alone(cuda, case):
    kw = dict(CASES[case])
    draws = R.make_draws(L, S, kw.pop("perm", [0, 1, 2]), **kw)
    C, Y = R.signals(3, L + S, seed=22)
    ref = R.reference(C, Y, draws)
    clean, noisy = _run(cuda, C, Y, draws, "padded")
    R.check(clean, noisy, ref, case)
    if case == "snr":
        assert R.snr_check(clean, noisy, ref, draws) == 2
    if case in ("remix", "shift"):                       # nothing but moves and one add: exact
        assert np.array_equal(clean, ref["clean"].astype(np.float32))


@pytest.mark.parametrize("B,n,shift", [(1, 1, 0), (1, 1, 3), (1, L, S), (3, 1, 2), (2, 2048, 0), (2, 2049, 1)])
def test_smallest_shapes(cuda, B, n, shift):
    """L = 1, B = 1, and the tile edge (2048 samples per workgroup)."""
    rng = np.random.default_rng(B * 10000 + n)
    draws = R.make_draws(n, shift, rng.permutation(B), rng.integers(0, shift + 1, B), rng.integers(0, shift + 1, B),
                         snr_db=[2.0] * B, gain=[1.25] * B, taps=[[(1, 0.5), (7, -0.25)]] * B)
    C, Y = R.signals(B, n + shift, seed=n)
    ref = R.reference(C, Y, draws)
    for form in ("flat", "padded"):
        clean, noisy = _run(cuda, C, Y, draws, form)
        R.check(clean, noisy, ref, f"B={B} L={n} S={shift} {form}")
        assert R.snr_check(clean, noisy, ref, draws) == B


def test_silent_rows_keep_a_at_one(cuda):
    """A silent clean row (Ec = 0) and a silent noise row (En = 0; without taps, or the speech's echo is its noise): a = 1
    and no NaN, with and without an echo on the other rows."""
    draws = R.make_draws(L, S, [0, 1, 2], off_clean=[3, 4, 5], off_noise=[3, 4, 6], snr_db=[3.0, 3.0, 3.0],
                         taps=[[(2, 0.5)], [], [(2, 0.5)]])
    C, Y = R.signals(3, L + S, seed=3, silent_clean=[0], silent_noise=[1])
    ref = R.reference(C, Y, draws)
    assert ref["a"][0] == 1.0 and ref["a"][1] == 1.0 and ref["a"][2] != 1.0
    clean, noisy = _run(cuda, C, Y, draws, "flat")
    R.check(clean, noisy, ref, "silent")
    assert not clean[0].any() and np.array_equal(noisy[1], clean[1])


def test_argument_errors_return_the_error_code_without_a_launch(cuda):
    augment_argument_errors()
    from cleanumamba_amd.training.augment import apply
    C, Y = (torch.from_numpy(x).to(cuda) for x in R.signals(2, 64, seed=1))
    draws = R.make_draws(60, 4, [1, 0])
    with pytest.raises(ValueError):
        apply(C, Y, draws, C[:, :60], None)              # an output over a source
    with pytest.raises(RuntimeError):
        apply(C, Y, draws, torch.empty(2, 61, device=cuda)[:, 1:], None)         # off the 16-byte grid: the library's -1
    torch.cuda.synchronize()


# ---- the feeder ---------------------------------------------------------------------------------------------------------
LENGTHS = [3000, 9000, 4099, 4100, 5000, 3500, 8000, 4098]
CROP, SHIFT = 4000, 37


def _augment():
    from cleanumamba_amd.training.augment import Augment, Echo
    return Augment(remix=True, shift=SHIFT, snr_db=(-5, 15), gain_db=(-6, 3), echo=Echo(rt60=(0.05, 0.1)))


def _dataset(root):
    from cleanumamba_amd.util.dataset import CleanNoisyPairDataset
    return CleanNoisyPairDataset(root=root, subset="training", crop_length_sec=CROP / MODEL)


@pytest.fixture
def h2d_copies(monkeypatch):
    """Counts host-to-device tensor copies (Tensor.copy_ and Tensor.to, the two ways the package moves a tensor)."""
    seen = []
    copy_, to = torch.Tensor.copy_, torch.Tensor.to

    def counted_copy(self, src, *a, **k):
        if self.is_cuda and isinstance(src, torch.Tensor) and not src.is_cuda:
            seen.append(("copy_", src.numel()))
        return copy_(self, src, *a, **k)

    def counted_to(self, *a, **k):
        out = to(self, *a, **k)
        if out.is_cuda and not self.is_cuda:
            seen.append(("to", self.numel()))
        return out
    monkeypatch.setattr(torch.Tensor, "copy_", counted_copy)
    monkeypatch.setattr(torch.Tensor, "to", counted_to)
    return seen


def test_feeder_batch_equals_apply_on_the_unaugmented_crops(cuda, tmp_path, h2d_copies):
    """Unrated: the augmenting feeder's batch == apply() on the L + S tensors of a plain feeder with the same plan, bit
    for bit; and still one host-to-device copy per batch (the existing feeder tests do not count copies; here every
    Tensor.copy_ / Tensor.to from host to device memory is counted)."""
    from cleanumamba_amd.training.augment import apply
    from cleanumamba_amd.training.feeder import BatchFeeder
    root = str(tmp_path)
    wavtree.training_tree(root, LENGTHS, seed=100)       # three clips are shorter than the crop: tiled, then shifted
    ds = _dataset(root)
    with BatchFeeder(ds, 4, cuda, crop_length=CROP, seed=9, augment=_augment()) as feeder:
        before = len(h2d_copies)
        got = [(b.entries, b.draws, b.tensors()) for b in feeder]
        torch.cuda.synchronize()
        # one copy per uploaded batch (the feeder is one batch ahead, into the next epoch), each a whole slot
        assert len(got) == 2 and len(h2d_copies) - before == feeder._uploaded in (2, 3), h2d_copies[before:]
        assert {n for _, n in h2d_copies[before:]} == {feeder._dev[0].flat.numel()}
    with BatchFeeder(ds, 4, cuda, crop_length=CROP + SHIFT, seed=9) as longer:
        for (entries, draws, (clean, noisy)), plain in zip(got, longer):
            assert entries == plain.entries and clean.shape == (4, 1, CROP)
            C, Y = plain.tensors()
            want = apply(C, Y, draws)
            assert torch.equal(clean, want[0]) and torch.equal(noisy, want[1])
            assert int(draws.n_taps.min()) > 0 and draws.rescales
            R.check(clean[:, 0].cpu().numpy(), noisy[:, 0].cpu().numpy(),
                    R.reference(C[:, 0].cpu().numpy(), Y[:, 0].cpu().numpy(), draws), "feeder")


def test_rated_feeder_batch_equals_apply_on_the_unaugmented_crops(cuda, tmp_path):
    """Rated, one 48 kHz pair among 16 kHz pairs."""
    from cleanumamba_amd.training.augment import apply
    from cleanumamba_amd.training.feeder import BatchFeeder
    root = str(tmp_path)
    mixed_tree(root, [(16000, 9000), (48000, 30000), (16000, 3000), (16000, 5000)], seed=40)
    ds = _dataset(root)
    with BatchFeeder(ds, 2, cuda, crop_length=CROP, seed=6, sample_rate=MODEL, augment=_augment()) as feeder, \
            BatchFeeder(ds, 2, cuda, crop_length=CROP + SHIFT, seed=6, sample_rate=MODEL) as longer:
        assert feeder.pitch == longer.pitch >= 3 * (CROP + SHIFT)
        n = 0
        for batch, plain in zip(feeder, longer):
            assert batch.entries == plain.entries and batch.windows == plain.windows and batch.shape == (2, 1, CROP)
            want = apply(*plain.tensors(), batch.draws)
            clean, noisy = batch.tensors()
            assert torch.equal(clean, want[0]) and torch.equal(noisy, want[1])
            n += 1
        assert n == 2


def test_no_augmentation_is_the_feeder_as_it_was(cuda, tmp_path, h2d_copies):
    from cleanumamba_amd.training.augment import Augment
    from cleanumamba_amd.training.feeder import BatchFeeder
    root = str(tmp_path)
    pairs = wavtree.training_tree(root, LENGTHS, seed=100)
    ds = _dataset(root)
    for augment in (None, Augment()):
        with BatchFeeder(ds, 4, cuda, crop_length=CROP, seed=9, augment=augment) as feeder:
            assert feeder.augment is None and feeder._dev[0].scratch is None
            assert feeder._dev[0].flat.numel() == 2 * 4 * feeder.pitch + 2 * 4
            before = len(h2d_copies)
            for batch, entries in zip(feeder, feeder.plan(0)):
                assert batch.entries == entries and batch.draws is None
                clean, noisy = batch.tensors()
                want = expected_batch(pairs, entries, CROP)
                assert torch.equal(clean.cpu(), want[0]) and torch.equal(noisy.cpu(), want[1])
            assert len(h2d_copies) - before == feeder._uploaded in (2, 3)


TINY = dict(channels_input=1, channels_output=1, channels_H=8, max_H=16, encoder_n_layers=3, kernel_size=4, stride=2,
            tsfm_n_layers=2, tsfm_n_head=2, tsfm_d_model=32, tsfm_d_inner=64)


def test_captured_step_replays_on_an_augmenting_feeder(cuda, tmp_path):
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
