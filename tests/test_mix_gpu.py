"""csrc/mix.hip (cum_mix_pairs) on the device against mix_ref.py, through the C ABI on buffers with padding and poison,
and the mixing BatchFeeder on the device: against the CPU feeder, into given tensors, with an Augment behind it, and
feeding a replayed TrainStep.

Bounds (all from the arithmetic, none from the kernel's results): the integer sums are exact, so the active levels, the
active shares and the flag equal the reference's; the peak is exact given the row's own a; a and g are within 2 ulp of
f32 -- two IEEE evaluation orders of the half dozen f64 operations behind each can differ in the last f64 bits, which
moves the f32 rounding by at most one step, and the guard's f32 division adds one more; the outputs are bit-equal to
steps 6 and 8 evaluated in NumPy from the kernel's own a and g."""
import numpy as np
import pytest
import torch

import mix_ref as R
import mixcases
from conftest import load_ckpt

pytestmark = pytest.mark.gpu

LENS = [1, 7, 1599, 1600, 1601, 3200 + 5, 40003]
POISON = 0x7F7F                                  # int16 has no NaN: a value that would move every sum
SNR = [5.0, 0.0, 10.0, -20.0, 3.0]
LEVEL = [-25.0, float("nan"), -30.0, -1.0, float("nan")]


def _rows(L):
    """Five rows that take every branch (confirmed on the reference in the test): 0 speech shorter than the row, loud then
    quiet (active and inactive frames), the guard idle;  1 all-zero speech;  2 quiet speech everywhere (no active frame:
    the whole row's level) over all-zero noise;  3 every frame active, SNR -20 dB at -1 dBFS: the guard acts;
    4 full scale, -32768 against +-32767 / -32768: the largest sums."""
    rng = np.random.default_rng(L)
    speech = rng.integers(-6000, 6000, (5, L)).astype(np.int16)
    noise = rng.integers(-20000, 20000, (5, L)).astype(np.int16)
    n_speech = [L] * 5
    n_speech[0] = max(1, (2 * L) // 3 + 1)
    speech[0, n_speech[0] // 2:] //= 200
    speech[1] = 0
    speech[2] = rng.integers(-20, 21, L)
    noise[2] = 0
    speech[3] = rng.integers(-32768, 32768, L)
    noise[3] = rng.integers(-32768, 32768, L)
    speech[4] = -32768
    noise[4] = np.where(np.arange(L) % 3 == 0, -32768, 32767)
    return speech, n_speech, noise


def _ulps(a, b):
    return int(abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32))))


def _records(n_speech, snr, level, frame, clip=0.99, activity_db=-50.0):
    from cleanumamba_amd.training import mix as M
    return M.MixDraws(snr, level, activity_db=activity_db, frame=frame, clip=clip).pack(n_speech)


def _run(cuda, speech, n_speech, noise, snr, level, frame, pad=(8, 4, 8), stats=True):
    """cum_mix_pairs through the C ABI: rows ``pitch`` > len apart with poison behind len, outputs with strides > len
    filled with NaN.  Returns (clean, noisy, stats) as numpy arrays with their padding."""
    from cleanumamba_amd import hip
    lib = hip.lib()
    nb, L = speech.shape
    pitch = (L + 7) // 8 * 8 + pad[0]
    pcm = np.full((2 * nb, pitch), POISON, np.int16)
    pcm[:nb, :L], pcm[nb:, :L] = speech, noise
    for b in range(nb):
        pcm[b, n_speech[b]:L] = POISON                          # behind a short speech clip too
    csb, nsb = (L + 3) // 4 * 4 + pad[1], (L + 3) // 4 * 4 + pad[2]
    d_pcm = torch.from_numpy(pcm).to(cuda)
    d_recs = torch.from_numpy(_records(n_speech, snr, level, frame)).to(cuda)
    clean = torch.full((nb, csb), float("nan"), device=cuda)
    noisy = torch.full((nb, nsb), float("nan"), device=cuda)
    st = torch.full((nb, 8), float("nan"), device=cuda)
    ws = torch.empty(lib.cum_mix_workspace_elems(nb, L) // 2, dtype=torch.float64, device=cuda)
    rc = lib.cum_mix_pairs(hip.ptr(d_pcm), pitch, hip.ptr(d_recs), nb, L, hip.ptr(ws), hip.ptr(clean), csb, hip.ptr(noisy),
                           nsb, hip.ptr(st) if stats else None, hip.stream_ptr())
    assert rc == 0, lib.cum_last_error()
    torch.cuda.synchronize()
    return clean.cpu().numpy(), noisy.cpu().numpy(), st.cpu().numpy()


def _check_against_reference(got, speech, n_speech, noise, snr, level, frame, where):
    clean, noisy, stats = got
    nb, L = speech.shape
    want = R.mix_batch(speech, n_speech, noise, snr, level, frame=frame)
    assert np.isnan(clean[:, L:]).all() and np.isnan(noisy[:, L:]).all(), f"{where}: wrote behind len"
    for b in range(nb):
        S, N = R.signals(speech[b], noise[b], n_speech[b], L)
        ref, st = want[2][b], stats[b]
        print(f"{where} row {b}: a {st[0]!r} vs {ref[0]!r} ({_ulps(st[0], ref[0])} ulp), g {st[1]!r} vs {ref[1]!r} "
              f"({_ulps(st[1], ref[1])} ulp), peak {st[4]!r}, shares {st[5]!r} {st[6]!r}, guard {st[7]!r}")
        assert _ulps(st[0], ref[0]) <= 2 and _ulps(st[1], ref[1]) <= 2, (where, b)
        assert st[2] == ref[2] and st[3] == ref[3], (where, b, "active levels")
        assert st[4] == np.abs(R.mixture(st[0], S, N)).max(), (where, b, "peak")
        assert st[5] == ref[5] and st[6] == ref[6] and st[7] == ref[7], (where, b, "shares and flag")
        c, y = R.outputs(st[0], st[1], S, N)
        assert np.array_equal(clean[b, :L].view(np.int32), c.view(np.int32)), (where, b, "clean")
        assert np.array_equal(noisy[b, :L].view(np.int32), y.view(np.int32)), (where, b, "noisy")
    return want


@pytest.mark.parametrize("frame", [1600, 37])
@pytest.mark.parametrize("L", LENS)
def test_kernel_meets_the_reference_on_every_branch(cuda, L, frame):
    speech, n_speech, noise = _rows(L)
    got = _run(cuda, speech, n_speech, noise, SNR, LEVEL, frame)
    want = _check_against_reference(got, speech, n_speech, noise, SNR, LEVEL, frame, f"len {L} frame {frame}")
    facts = want[3]
    # the reference confirms that the rows take the branches they were built for
    assert facts[1]["a"] == 1.0 and want[2][1, 2] == 0                           # all-zero speech
    assert facts[2]["a"] == 1.0 and want[2][2, 3] == 0                           # all-zero noise
    assert not any(facts[2]["active_s"]) and want[2][2, 2] > 0                   # no active frame: the whole row's level
    assert all(facts[3]["active_s"]) and all(facts[3]["active_n"]) and all(facts[4]["active_s"])
    assert np.isnan(LEVEL[1]) and facts[1]["g"] == 1.0 and facts[4]["g"] == 1.0  # level NaN
    assert want[2][4, 2] == 1.0                                                  # full scale: Ps = 2^30 exactly
    if L > 1:
        assert facts[0]["n_s"] < L                                               # tiled speech
    if L >= 1599:
        nf = -(-L // frame)
        if facts[0]["n_s"] - facts[0]["n_s"] // 2 >= 2 * frame:                   # a whole frame inside the quiet half
            assert 0 < sum(facts[0]["active_s"]) < nf                            # active and inactive frames
        assert facts[0]["n_s"] % frame != 0                                      # the tiling passes through a frame
        assert facts[3]["guard"] and not facts[0]["guard"] and not facts[2]["guard"]
    # two runs give the same bits
    again = _run(cuda, speech, n_speech, noise, SNR, LEVEL, frame)
    for a, b in zip(got, again):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    # a row alone gives the bits it gives inside the batch
    for b in range(5):
        alone = _run(cuda, speech[b:b + 1], n_speech[b:b + 1], noise[b:b + 1], SNR[b:b + 1], LEVEL[b:b + 1], frame)
        for a, full in zip(alone, got):
            assert np.array_equal(a[0].view(np.int32), full[b].view(np.int32)), (L, frame, b)


@pytest.mark.parametrize("L", [7, 3200 + 5])
def test_unaligned_output_rows_and_no_stats(cuda, L):
    """Output strides that put rows off the 16-byte grid (the element stores), and stats = NULL."""
    speech, n_speech, noise = _rows(L)
    got = _run(cuda, speech, n_speech, noise, SNR, LEVEL, 1600, pad=(16, 5, 7))
    _check_against_reference(got, speech, n_speech, noise, SNR, LEVEL, 1600, f"len {L} unaligned")
    quiet = _run(cuda, speech, n_speech, noise, SNR, LEVEL, 1600, pad=(16, 5, 7), stats=False)
    assert np.isnan(quiet[2]).all()
    for a, b in zip(got[:2], quiet[:2]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_a_bad_table_stays_inside_its_rows(cuda):
    """n_speech and frame outside [1, len] are clamped in the kernel: the result is the clamped record's."""
    L = 1601
    speech, n_speech, noise = _rows(L)
    from cleanumamba_amd.training import mix as M
    from cleanumamba_amd import hip
    lib = hip.lib()
    recs = _records(n_speech, SNR, LEVEL, 1600).reshape(5, M.REC_INTS)
    recs[0, M.REC_N_SPEECH], recs[1, M.REC_N_SPEECH], recs[2, M.REC_FRAME], recs[3, M.REC_FRAME] = -5, 2 ** 31 - 1, 0, 2 ** 31 - 1
    pitch = 1608
    pcm = np.full((10, pitch), POISON, np.int16)
    pcm[:5, :L], pcm[5:, :L] = speech, noise
    clean, noisy = torch.full((5, 1604), float("nan"), device=cuda), torch.full((5, 1604), float("nan"), device=cuda)
    st = torch.zeros(5, 8, device=cuda)
    ws = torch.empty(lib.cum_mix_workspace_elems(5, L) // 2, dtype=torch.float64, device=cuda)
    d_pcm, d_recs = torch.from_numpy(pcm).to(cuda), torch.from_numpy(recs.reshape(-1)).to(cuda)
    rc = lib.cum_mix_pairs(hip.ptr(d_pcm), pitch, hip.ptr(d_recs), 5, L, hip.ptr(ws), hip.ptr(clean), 1604, hip.ptr(noisy),
                           1604, hip.ptr(st), hip.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    got = (clean.cpu().numpy(), noisy.cpu().numpy(), st.cpu().numpy())
    for b, (n, frame) in enumerate([(1, 1600), (L, 1600), (L, 1), (L, L), (L, 1600)]):
        _check_against_reference(tuple(g[b:b + 1] for g in got), speech[b:b + 1], [n], noise[b:b + 1], SNR[b:b + 1],
                                 LEVEL[b:b + 1], frame, f"clamped row {b}")


def test_argument_errors_of_the_c_abi(cuda):
    assert mixcases.argument_errors() == 18


def test_apply_on_device_tensors_equals_the_host_within_the_bounds(cuda):
    from cleanumamba_amd.training import mix as M
    L = 3205
    speech, n_speech, noise = _rows(L)
    draws = M.MixDraws(SNR, LEVEL, frame=160)
    host = M.apply(torch.from_numpy(speech), n_speech, torch.from_numpy(noise), draws)
    out = torch.full((5, 1, L), float("nan"), device=cuda)
    dev = M.apply(torch.from_numpy(speech).to(cuda), n_speech, torch.from_numpy(noise).to(cuda), draws, noisy_out=out)
    assert dev[1] is out and dev[0].shape == (5, L) and dev[2].shape == (5, 8)
    got = (dev[0].cpu().numpy(), dev[1][:, 0].cpu().numpy(), dev[2].cpu().numpy())
    _check_against_reference(got, speech, n_speech, noise, SNR, LEVEL, 160, "apply")
    assert all(_ulps(a, b) <= 2 for a, b in zip(got[2][:, :2].reshape(-1), host[2][:, :2].numpy().reshape(-1)))
    off = torch.empty(5 * L + 1, device=cuda)[1:].view(5, L)
    with pytest.raises(RuntimeError):                            # an unaligned output is the library's -1
        M.apply(torch.from_numpy(speech).to(cuda), n_speech, torch.from_numpy(noise).to(cuda), draws, clean_out=off)
    with pytest.raises(ValueError):
        M.apply(torch.from_numpy(speech).to(cuda), n_speech, torch.from_numpy(noise).to(cuda), draws,
                clean_out=out[:, 0], noisy_out=out)


# ---------------------------------------------------------------------------------------------------------------- feeder
CROP = 1000
MIX = dict(snr_db=(-5.0, 20.0), level_db=(-35.0, -15.0), frame=160, gap=50, max_pieces=3)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return mixcases.mix_tree(str(tmp_path_factory.mktemp("unpaired_gpu")), seed=300)


def _dataset(tree, crop=CROP):
    from cleanumamba_amd.util.dataset import SpeechNoiseDataset
    return SpeechNoiseDataset(tree[0], tree[1], crop_length_sec=crop / 16000)


def test_device_feeder_equals_the_cpu_feeder_and_writes_into_given_tensors(cuda, tree):
    from cleanumamba_amd.training import mix as M
    from cleanumamba_amd.training.feeder import BatchFeeder
    _, _, speech, noise = tree
    ds, mix = _dataset(tree), M.Mix(**MIX)
    with BatchFeeder(ds, 4, cuda, seed=9, mix=mix) as dev, BatchFeeder(ds, 4, "cpu", seed=9, mix=mix) as host:
        seen = 0
        for _ in range(2):
            for batch in dev:
                ref = host.next()
                assert batch.entries == ref.entries and batch.noise == ref.noise and batch.shape == (4, 1, CROP)
                want_clean, want_noisy = ref.tensors()
                clean, noisy = batch.tensors()
                assert clean.device == cuda and clean.dtype == torch.float32 and clean.shape == (4, 1, CROP)
                S, n_speech, N = mixcases.planned_rows(batch.entries, batch.noise, speech, noise, CROP)
                got = (clean[:, 0].cpu().numpy(), noisy[:, 0].cpu().numpy(), batch.mix_stats().cpu().numpy())
                _check_against_reference(got, S, n_speech, N, batch.mix.snr_db, batch.mix.level_db, 160, f"batch {seen}")
                stats = ref.mix_stats().numpy()
                assert np.array_equal(got[2][:, 2:], stats[:, 2:])
                if np.array_equal(got[2][:, :2], stats[:, :2]):          # the same two scalars: the same bits
                    assert torch.equal(clean.cpu(), want_clean) and torch.equal(noisy.cpu(), want_noisy)
                # into(): straight into the tensors it is given, nothing beside them
                flat = torch.full((4, CROP + 4), 7.0, device=cuda)
                given = torch.full((4, 1, CROP), 7.0, device=cuda)
                out = batch.into(flat[:, :CROP], given)
                assert out[0].data_ptr() == flat.data_ptr() and out[1] is given
                assert torch.equal(flat[:, :CROP], clean[:, 0]) and torch.equal(given, noisy) and (flat[:, CROP:] == 7).all()
                seen += 1
            with pytest.raises(StopIteration):                   # the CPU feeder's epoch ends with the device feeder's
                host.next()
        assert seen == 4


def test_device_feeder_with_augment_behind_the_mix(cuda, tree):
    from cleanumamba_amd.training import augment as A
    from cleanumamba_amd.training import mix as M
    from cleanumamba_amd.training.feeder import BatchFeeder
    _, _, speech, noise = tree
    ds, mix, shift = _dataset(tree), M.Mix(**MIX), 37
    aug = A.Augment(remix=True, shift=shift, snr_db=(0, 10), gain_db=(-6, 3))
    with BatchFeeder(ds, 4, cuda, seed=9, mix=mix, augment=aug) as feeder:
        for k, batch in enumerate(feeder):
            S, n_speech, N = mixcases.planned_rows(batch.entries, batch.noise, speech, noise, CROP + shift)
            mixed = M.apply(torch.from_numpy(S).to(cuda), n_speech, torch.from_numpy(N).to(cuda), batch.mix)
            want = A.apply(mixed[0], mixed[1], batch.draws)
            clean, noisy = batch.tensors()
            assert clean.shape == (4, 1, CROP)
            assert torch.equal(clean[:, 0], want[0]) and torch.equal(noisy[:, 0], want[1])
            assert torch.equal(batch.mix_stats(), mixed[2])
        assert k == 1


def test_train_step_takes_mixed_batches_under_graph_replay(cuda, tree):
    """The shipped 442k model, fed ``step(batch)`` from the mixing feeder: the warm-up, the capture and three replayed
    steps, which assemble into the graph's own inputs."""
    from cleanumamba_amd.network import CleanUMamba
    from cleanumamba_amd.training import mix as M
    from cleanumamba_amd.training.feeder import BatchFeeder
    from cleanumamba_amd.training.train_step import GRAPH_WARMUP_STEPS, TrainStep
    sd, cfg = load_ckpt("442k")
    net = CleanUMamba(**cfg)
    net.load_state_dict(sd, strict=True)
    net = net.to(cuda).train()
    before = [p.detach().clone() for p in net.parameters()]
    step = TrainStep(net, optimization={"n_iters": 200}, use_graph=True)
    losses, crop = [], 2048
    with BatchFeeder(_dataset(tree, crop), 2, cuda, crop_length=crop, seed=1, mix=M.Mix(**MIX)) as feeder:
        while len(losses) < GRAPH_WARMUP_STEPS + 3:
            for batch in feeder:
                loss, _ = step(batch)
                losses.append(float(loss))
                if len(losses) == GRAPH_WARMUP_STEPS + 3:
                    break
        assert step.graph_status == "captured", step.graph_status
        # the last step was a replay: the graph's inputs are the batch itself
        clean, noisy = batch.tensors()
        assert torch.equal(step._graph["clean"], clean) and torch.equal(step._graph["noisy"], noisy)
        assert float(batch.mix_stats()[:, 0].min()) > 0
    assert all(np.isfinite(l) for l in losses), losses
    assert any(not torch.equal(p.detach(), q) for p, q in zip(net.parameters(), before))
