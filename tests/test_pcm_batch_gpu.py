"""cum_pcm_batch_f32 (csrc/pcm.hip) at the smallest shapes where it can go wrong: one row and several, lengths around
the 8-sample vector (1, 7, 8, 9) and past one workgroup's sweep with a tail (1027), padded rows, every kind of entry in
the clip-length table (tiled, full, too long, zero), and outputs that are windows of larger buffers whose row starts are
and are not 16-byte aligned.

Acceptance is exact: an int16 times 2^-15 is a float32, so the result must be bit-identical to the numpy statement of
the formula in include/cleanumamba_hip.h; nothing outside the (batch, len) windows may change, and pcm is read only."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -7.5


def _tables(batch, length):
    kinds = [1, 3, length - 1, length, length + 5, 0]            # the last two exercise the clamp
    if batch == 1:
        return [[k] for k in kinds]
    return [kinds[:3], kinds[3:], [length, length - 1, length]]


def _expected(pcm, table, length):
    """clean[b, t] = pcm[b][t mod n_b] 2^-15 with n_b = clamp(src_len[b], 1, len); likewise noisy from row batch + b."""
    batch = len(table)
    out = np.empty((2, batch, length), np.float32)
    for b, n in enumerate(table):
        n = min(max(int(n), 1), length)
        idx = np.arange(length) % n
        out[0, b] = pcm[b, idx].astype(np.float32) * np.float32(2.0 ** -15)
        out[1, b] = pcm[batch + b, idx].astype(np.float32) * np.float32(2.0 ** -15)
    return out


@pytest.mark.parametrize("extra_pitch", [0, 64])
@pytest.mark.parametrize("length", [1, 7, 8, 9, 1027])
@pytest.mark.parametrize("batch", [1, 3])
def test_pcm_batch_is_exact_and_stays_in_its_windows(cuda, batch, length, extra_pitch):
    from cleanumamba_amd import hip
    lib = hip.lib()
    pitch = (length + 7) // 8 * 8 + extra_pitch
    rng = np.random.default_rng(1000 * batch + length + extra_pitch)
    pcm_host = rng.integers(-32768, 32768, size=(2 * batch, pitch)).astype(np.int16)
    pcm_host[0, 0], pcm_host[-1, length - 1] = -32768, 32767
    pcm = torch.from_numpy(pcm_host).to(cuda)
    # clean rows: an odd stride (rows after the first start off the 16-byte grid: the element path also for full rows);
    # noisy rows: a multiple of 4 floats (full rows take the 16-byte path).  Both windows start 32 bytes into their buffer.
    clean_sb, noisy_sb = length + 13 - length % 2, (length + 3) // 4 * 4 + 8
    assert clean_sb % 2 == 1 and noisy_sb % 4 == 0
    assert clean_sb != noisy_sb and min(clean_sb, noisy_sb) > length
    for table in _tables(batch, length):
        src_len = torch.tensor(table, dtype=torch.int32, device=cuda)
        bufs = [torch.full((8 + batch * sb + 5,), SENTINEL, device=cuda) for sb in (clean_sb, noisy_sb)]
        views = [buf[8:8 + batch * sb].view(batch, sb)[:, :length] for buf, sb in zip(bufs, (clean_sb, noisy_sb))]
        hip.check(lib.cum_pcm_batch_f32(hip.ptr(pcm), pitch, hip.ptr(src_len), batch, length, hip.ptr(views[0]), clean_sb,
                                        hip.ptr(views[1]), noisy_sb, hip.stream_ptr()))
        torch.cuda.synchronize()
        want = _expected(pcm_host, table, length)
        for k, (buf, view, sb) in enumerate(zip(bufs, views, (clean_sb, noisy_sb))):
            assert torch.equal(view.cpu(), torch.from_numpy(want[k])), (table, "clean" if k == 0 else "noisy")
            outside = torch.ones_like(buf, dtype=torch.bool)
            outside[8:8 + batch * sb].view(batch, sb)[:, :length] = False
            assert (buf[outside] == SENTINEL).all(), (table, "wrote outside its window")
        assert torch.equal(pcm.cpu(), torch.from_numpy(pcm_host))
