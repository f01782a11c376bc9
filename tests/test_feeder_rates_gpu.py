"""Pairs at any sample rate on the device (training/feeder.py with ``sample_rate``, csrc/resample.hip:
cum_pcm_batch_resample_f32, util/denoise_eval.validate(resample=True)).  The yardstick throughout is
``resample_ragged`` (cum_resample_ragged) on the WHOLE file, sliced or tiled by hand: the same fma chains, so every
comparison is ``torch.equal``."""
import copy
import os
import warnings

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import wavtree
from conftest import load_ckpt, load_golden, rel_l2
from test_feeder_rates_host import MODEL, mixed_tree

pytestmark = pytest.mark.gpu

RATES = [8000, 16000, 22050, 32000, 44100, 48000]        # up = 2, copy, up = 320, up = 1, up = 160, up = 1
LENS = [767, 768, 769, 1537]
SENTINEL = 7.0
FILL = 32767                                             # behind every row's n_src: read, it would change the sums


@pytest.fixture(autouse=True)
def leave_global_state_as_found(monkeypatch):
    """Tests that run later draw from torch's global generators without seeding them and expect python_eval's one-time
    ``pesq`` warning: the generators' states and that flag are put back after every test here."""
    from cleanumamba_amd.util import python_eval
    monkeypatch.setattr(python_eval, "_PESQ_WARNED", python_eval._PESQ_WARNED)
    cpu = torch.get_rng_state()
    gpu = torch.cuda.get_rng_state_all() if torch.cuda.is_available() else None
    yield
    torch.set_rng_state(cpu)
    if gpu is not None:
        torch.cuda.set_rng_state_all(gpu)


def _factors(rate):
    from cleanumamba_amd.util.resample import plan
    if rate == MODEL:
        return 1, 1, 0, 1
    p = plan(rate, MODEL)
    return p.up, p.down, p.H, p.K


def _frames_for(M, up, down):
    """A file length with exactly M outputs, or None (up = 2 has no file with an odd count)."""
    from cleanumamba_amd.util.resample import out_length
    for N in range(max(1, (M - 1) * down // up), M * down // up + 2):
        if out_length(N, up, down) == M:
            return N
    return None


@pytest.fixture(scope="module")
def files(cuda):
    """Per rate: [(clean int16, noisy int16, clean f32 at 16 k, noisy f32 at 16 k)] -- a long file, files of K - 1, K and
    K + 1 samples, and files whose output counts sit on the tile (768) and on every ``len`` of LENS.  Converted once, by
    cum_resample_ragged on the whole files."""
    from cleanumamba_amd.util.resample import out_length, resample_ragged
    out = {}
    for rate in RATES:
        up, down, H, K = _factors(rate)
        frames = [_frames_for(5003, up, down) or _frames_for(5004, up, down), max(K - 1, 1), K, K + 1]
        frames += [N for N in (_frames_for(M, up, down) for M in (1, 2, 3, 766, 767, 768, 769, 1536, 1537)) if N]
        frames = sorted(set(frames))
        raw = [(wavtree.pcm(N, rate + 2 * i), wavtree.pcm(N, rate + 2 * i + 1)) for i, N in enumerate(frames)]
        x = torch.zeros(2 * len(raw), max(frames), dtype=torch.int16)
        for i, (c, n) in enumerate(raw):
            x[2 * i, :len(c)], x[2 * i + 1, :len(n)] = torch.from_numpy(c), torch.from_numpy(n)
        y, lens = resample_ragged(x.to(cuda), [N for N in frames for _ in range(2)], rate, MODEL)
        y = y.cpu()
        out[rate] = []
        for i, (c, n) in enumerate(raw):
            M = out_length(len(c), up, down)
            assert lens[2 * i] == M
            out[rate].append((c, n, y[2 * i, :M].clone(), y[2 * i + 1, :M].clone()))
    return out


def _blob(cuda):
    """Plans of RATES (the 16 k rows take plan -1) and their tables, as the entry takes them."""
    from cleanumamba_amd.util.resample import plan
    ids, ints, tabs, off = {MODEL: -1}, [], [], 0
    for rate in RATES:
        if rate == MODEL:
            continue
        p = plan(rate, MODEL)
        ids[rate] = len(ints)
        ints.append([p.up, p.down, len(p.taps), p.K, p.pitch, off, 0, 0])
        tabs.append(p.host_table().reshape(-1))
        off += p.up * p.pitch
    host = torch.tensor(ints, dtype=torch.int32)
    return ids, host, host.to(cuda), torch.cat(tabs).to(cuda)


@pytest.mark.parametrize("length", LENS)
def test_kernel_alone_equals_the_whole_file_conversion_sliced_or_tiled(cuda, files, length):
    """ONE launch whose rows cover every rate of RATES (both chain routes and the copy route), crops at m0 in {0, 1, middle,
    M - len} and repeated files with M in {1, 2, 3, 73 .. 220 (K - 1, K, K + 1 samples), 766 .. 769, len - 1, len}."""
    from cleanumamba_amd import hip
    from cleanumamba_amd.util.resample import crop_window, window_bound
    ids, plans_host, plans_dev, tables = _blob(cuda)
    cases = []                                           # (rate, file, m0)
    for rate in RATES:
        for f in files[rate]:
            M = len(f[2])
            starts = [0] if M <= length else sorted({0, 1, (M - length) // 2, M - length})
            cases += [(rate, f, m0) for m0 in starts]
    B = len(cases)
    assert {M for _, f, _ in cases for M in [len(f[2])]} >= {1, 3, 767, 768, 769, length - 1, length}
    need = max(window_bound(length, *_factors(r)[:2], _factors(r)[3]) for r in RATES)
    pitch = (need + 7) // 8 * 8 + 24                     # a row pitch above the need
    rows = torch.full((2, B, pitch), FILL, dtype=torch.int16)
    recs = torch.zeros(B, 16, dtype=torch.int32)
    pos = recs.view(torch.int64)
    want = torch.empty(2, B, length)
    for b, (rate, (c, n, yc, yn), m0) in enumerate(cases):
        up, down, H, K = _factors(rate)
        M = len(yc)
        n_lo, n_cnt = crop_window(len(c), up, down, H, K, m0, min(length, M))
        rows[0, b, :n_cnt] = torch.from_numpy(c[n_lo:n_lo + n_cnt])
        rows[1, b, :n_cnt] = torch.from_numpy(n[n_lo:n_lo + n_cnt])
        recs[b, :4] = torch.tensor([ids[rate], n_cnt, M, len(c)], dtype=torch.int32)
        pos[b, 6], pos[b, 7] = n_lo, m0
        idx = (m0 + torch.arange(length)) % M
        want[0, b], want[1, b] = yc[idx], yn[idx]
    rows_d, recs_d = rows.to(cuda), recs.to(cuda)
    # clean: (B, L) rows 13 floats longer than the crop (odd: the rows start off the 16-byte grid); noisy: (B, 1, L) rows
    # on the grid, another stride
    clean_buf = torch.full((B, length + 13), SENTINEL, device=cuda)
    noisy_buf = torch.full((B, 1, (length + 3) // 4 * 4 + 8), SENTINEL, device=cuda)
    clean, noisy = clean_buf[:, :length], noisy_buf[:, :, :length]
    assert clean.stride(0) != noisy.stride(0)

    def launch():
        hip.check(hip.lib().cum_pcm_batch_resample_f32(
            hip.ptr(rows_d), pitch, hip.ptr(recs), hip.ptr(recs_d), B, hip.ptr(plans_host), hip.ptr(plans_dev),
            plans_host.shape[0], hip.ptr(tables), tables.numel(), length, hip.ptr(clean), clean.stride(0), hip.ptr(noisy),
            noisy.stride(0), hip.stream_ptr()))
        torch.cuda.synchronize()
    launch()
    got = torch.stack([clean.cpu(), noisy[:, 0].cpu()])
    for b, (rate, f, m0) in enumerate(cases):
        for k in range(2):
            assert torch.equal(got[k, b], want[k, b]), (rate, len(f[0]), len(f[2]), m0, "clean noisy".split()[k])
    assert (clean_buf[:, length:] == SENTINEL).all() and (noisy_buf[:, :, length:] == SENTINEL).all()
    assert torch.equal(rows_d.cpu(), rows)               # nothing was written into the staging rows
    first = (clean_buf.clone(), noisy_buf.clone())
    launch()
    assert torch.equal(clean_buf, first[0]) and torch.equal(noisy_buf, first[1])


# ---- the feeder, end to end ------------------------------------------------------------------------------------------
TREE = [(8000, 9000), (16000, 9000), (22050, 14000), (44100, 30000), (48000, 30000), (48000, 9000)]
CROP = 4000                                              # 48 k / 9000 gives 3000 outputs, 22.05 k / 14000 gives 10159 ...
TREE_SHORT = [(8000, 1500)]                              # ... and 8 k / 1500 gives 3000: two files shorter than the crop


@pytest.fixture(scope="module")
def mixed(cuda, tmp_path_factory):
    """(root, [(clean f32, noisy f32) at 16 k per pair]): the tree of TREE with pair 0 replaced by a short 8 k file, and
    every file converted whole by ``resample_ragged``."""
    from cleanumamba_amd.util.resample import resample_ragged
    root = str(tmp_path_factory.mktemp("pairs_rated"))
    spec = TREE_SHORT + TREE[1:]
    pairs = mixed_tree(root, spec, seed=40)
    whole = []
    for (rate, N), (c, n) in zip(spec, pairs):
        x = torch.from_numpy(np.stack([c, n])).to(cuda)
        y, lens = resample_ragged(x, [N, N], rate, MODEL)
        whole.append((y[0, :lens[0]].cpu(), y[1, :lens[1]].cpu()))
    return root, spec, whole


def _dataset(root):
    from cleanumamba_amd.util.dataset import CleanNoisyPairDataset
    return CleanNoisyPairDataset(root=root, subset="training", crop_length_sec=CROP / MODEL)


def _hand_made(whole, batch, crop):
    out = []
    for k in range(2):
        rows = []
        for (index, _, _), (m0, M, _) in zip(batch.entries, batch.windows):
            assert M == len(whole[index][k])
            rows.append(whole[index][k][(m0 + torch.arange(crop)) % M])
        out.append(torch.stack(rows)[:, None, :])
    return out


def test_rated_feeder_batches_equal_the_hand_made_chain(cuda, mixed):
    from cleanumamba_amd.training.feeder import BatchFeeder
    root, spec, whole = mixed
    ds = _dataset(root)
    seen = {}
    for workers in (1, 4):
        with BatchFeeder(ds, 3, cuda, crop_length=CROP, seed=6, workers=workers, sample_rate=MODEL) as feeder:
            assert feeder.pitch >= 12000 and feeder.pitch % 8 == 0       # 48 k: three source samples per output
            got = []
            for epoch in range(2):
                plan = feeder.plan(epoch)
                for batch, entries in zip(feeder, plan):
                    assert batch.entries == entries and batch.epoch == epoch
                    assert [r for _, _, r in batch.windows] == [spec[i][0] for i, _, _ in entries]
                    clean, noisy = batch.tensors()
                    assert clean.shape == (3, 1, CROP) and clean.device == cuda and clean.dtype == torch.float32
                    want = _hand_made(whole, batch, CROP)
                    assert torch.equal(clean.cpu(), want[0]) and torch.equal(noisy.cpu(), want[1]), batch.windows
                    flat = torch.empty(3, CROP + 5, device=cuda)[:, :CROP]       # (B, L) outputs, rows off the grid
                    batch.into(flat, noisy)
                    assert torch.equal(flat.cpu(), want[0][:, 0])
                    got.append((batch.entries, batch.windows, clean.cpu(), noisy.cpu()))
            assert len(got) == 4
            windows = [w for _, ws, _, _ in got for w in ws]
            assert sum(M <= CROP for _, M, _ in windows) == 4 and any(m0 > 0 for m0, _, _ in windows)
        seen[workers] = got
    for a, b in zip(seen[1], seen[4]):
        assert a[0] == b[0] and a[1] == b[1] and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


def test_rated_stale_batch_raises_instead_of_reading_new_data(cuda, mixed):
    from cleanumamba_amd.training.feeder import BatchFeeder
    root, _, whole = mixed
    depth = 2
    with BatchFeeder(_dataset(root), 2, cuda, crop_length=1000, seed=4, depth=depth, sample_rate=MODEL) as feeder:
        first = feeder.next()
        want = _hand_made(whole, first, 1000)
        for _ in range(depth - 1):
            feeder.next()
        assert torch.equal(first.tensors()[0].cpu(), want[0])       # depth - 1 further calls: still its own data
        feeder.next()
        with pytest.raises(RuntimeError):
            first.tensors()
        with pytest.raises(RuntimeError):
            first.into(torch.empty(2, 1, 1000, device=cuda), torch.empty(2, 1, 1000, device=cuda))


def test_rated_feeder_on_a_16k_tree_equals_the_unrated_feeder(cuda, tmp_path):
    from cleanumamba_amd.training.feeder import BatchFeeder
    root = str(tmp_path)
    wavtree.training_tree(root, [3000, 9000, 4000, 4001, 5000, 3999, 8000, 6001], seed=21)
    ds = _dataset(root)
    with BatchFeeder(ds, 4, cuda, crop_length=CROP, seed=2) as plain, \
            BatchFeeder(ds, 4, cuda, crop_length=CROP, seed=2, sample_rate=MODEL) as rated:
        assert plain.pitch == rated.pitch
        n = 0
        for a, b in zip(plain, rated):
            assert a.entries == b.entries and a.windows is None and b.windows is not None
            (ca, na), (cb, nb) = a.tensors(), b.tensors()
            assert torch.equal(ca, cb) and torch.equal(na, nb)
            n += 1
        assert n == 2


TINY = dict(channels_input=1, channels_output=1, channels_H=8, max_H=16, encoder_n_layers=3, kernel_size=4, stride=2,
            tsfm_n_layers=2, tsfm_n_head=2, tsfm_d_model=32, tsfm_d_inner=64)


def test_step_fed_a_rated_batch_equals_step_fed_its_tensors(cuda, mixed):
    """test_feeder_gpu.py::test_step_fed_a_batch_equals_step_fed_its_tensors on the mixed tree: two copies of a tiny
    model, 8 captured steps each on the rated feeder's batches, one fed ``step(batch)`` (the replay converts into the
    graph's own inputs), the other ``step(*batch.tensors())``.  Same kernels, same inputs: that test's bounds."""
    from cleanumamba_amd.network import CleanUMamba
    from cleanumamba_amd.training.feeder import BatchFeeder
    from cleanumamba_amd.training.train_step import TrainStep
    root, _, _ = mixed
    torch.manual_seed(0)
    net_a, net_b = CleanUMamba(**TINY), CleanUMamba(**TINY)
    net_b.load_state_dict(copy.deepcopy(net_a.state_dict()), strict=True)
    net_a, net_b = net_a.to(cuda).train(), net_b.to(cuda).train()
    steps = [TrainStep(net_a, optimization={"n_iters": 200}, use_graph=True),
             TrainStep(net_b, optimization={"n_iters": 200}, use_graph=True)]
    losses = [[], []]
    with BatchFeeder(_dataset(root), 2, cuda, crop_length=CROP, seed=1, sample_rate=MODEL) as feeder:
        done = 0
        while done < 8:
            for batch in feeder:
                clean, noisy = batch.tensors()
                la, _ = steps[0](batch)
                lb, _ = steps[1](clean, noisy)
                losses[0].append(float(la))
                losses[1].append(float(lb))
                done += 1
                if done == 8:
                    break
        assert steps[0].graph_status == "captured", steps[0].graph_status
        assert steps[1].graph_status == "captured", steps[1].graph_status
        # the last step was a replay: the graph's input is the batch itself
        assert torch.equal(steps[0]._graph["clean"], clean) and torch.equal(steps[0]._graph["noisy"], noisy)
    for (ka, pa), (kb, pb) in zip(net_a.named_parameters(), net_b.named_parameters()):
        assert rel_l2(pa, pb) < 1e-6, ka
    assert max(abs(a - b) for a, b in zip(*losses)) < 1e-5 * max(losses[1])
    assert all(l == l for l in losses[0])


# ---- validate(resample=True) -------------------------------------------------------------------------------------------
def _write_dns(root, rate, clean, noisy):
    os.makedirs(os.path.join(root, "clean"))
    os.makedirs(os.path.join(root, "noisy"))
    for i, (c, n) in enumerate(zip(clean, noisy)):
        wavfile.write(os.path.join(root, "clean", f"clean_fileid_{i}.wav"), rate, c)
        wavfile.write(os.path.join(root, "noisy", f"book_{i:05d}_snr5_fileid_{i}.wav"), rate, n)


def test_validate_resample_equals_validate_on_a_folder_converted_by_hand(cuda, tmp_path):
    """A 48 kHz test folder through ``validate(resample=True)`` against the same folder converted beforehand -- noisy
    written as float32, clean as int16 by ``(y * 32768).round().clamp(-32768, 32767)`` -- through plain ``validate``.
    Both routes run the same kernels on the same inputs: the dicts are equal (NaN where the other is NaN)."""
    from cleanumamba_amd.network import CleanUMamba
    from cleanumamba_amd.util.denoise_eval import validate
    from cleanumamba_amd.util.resample import resample_ragged
    sd, cfg = load_ckpt("442k")
    net = CleanUMamba(**cfg)
    net.load_state_dict(sd, strict=True)
    net = net.to(cuda).eval()
    g = load_golden("metrics")
    rng = np.random.default_rng(3)
    # speech at 16 k held three samples each: 48 k files of 1 s and (one clip) 1.5 s
    clean = [np.repeat(g[f"clean_{i}"][:n], 3) for i, n in ((0, 16000), (1, 16000), (2, 24000))]
    noisy = [np.clip(c + 1500 * rng.standard_normal(c.size), -32768, 32767).astype(np.int16) for c in clean]
    there, here = str(tmp_path / "at48k"), str(tmp_path / "at16k")
    _write_dns(there, 48000, clean, noisy)
    conv_clean, conv_noisy = [], []
    for c, n in zip(clean, noisy):
        y, lens = resample_ragged(torch.from_numpy(np.stack([c, n])).to(cuda), [c.size, n.size], 48000, MODEL)
        conv_clean.append((y[0, :lens[0]] * 32768).round().clamp(-32768, 32767).to(torch.int16).cpu().numpy())
        conv_noisy.append(y[1, :lens[1]].cpu().numpy())
    assert conv_noisy[0].dtype == np.float32 and conv_clean[0].shape == (16000,) and conv_clean[2].shape == (24000,)
    _write_dns(here, MODEL, conv_clean, conv_noisy)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = validate(net, there, resample=True)
        want = validate(net, here)
        cropped = validate(net, there, resample=True, crop=1)
        with pytest.raises(Exception):                   # without the switch the metrics refuse the rate, as before
            validate(net, there)
    assert got["Test/count"] == want["Test/count"] == 2 * 16000 + 24000 and set(got) == set(want)
    for k in want:
        assert np.array_equal(np.float64(got[k]), np.float64(want[k]), equal_nan=True), (k, got[k], want[k])
    assert np.isfinite(got["Test/stoi"]) and np.isfinite(got["Test/segSNR"]) and got["Test/stoi"] > 0
    assert cropped["Test/count"] == 3 * 16000            # ``crop`` counts seconds at 16 kHz
