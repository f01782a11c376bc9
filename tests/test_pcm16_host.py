"""Host side of the on-device validation route (no GPU): the numpy statement of the two quantisers against torch's own
expressions in util/denoise_eval.py, what ``validate(batching=...)`` refuses before it reads a file, the checks of
``metrics.Batch.from_flat``, and the ABI of the two new entries (rejections happen before any launch)."""
import ctypes

import numpy as np
import pytest
import torch

import pcm16_ref as P
from conftest import load_ckpt


def _torch_rule(v, mode):
    y = torch.from_numpy(np.asarray(v, np.float32))
    if mode == 0:
        return (y * 32767).clamp(-32768, 32767).to(torch.int16).numpy()
    return (y * 32768).round().clamp(-32768, 32767).to(torch.int16).numpy()


@pytest.mark.parametrize("mode", [0, 1])
def test_numpy_rule_is_torchs_expression(mode):
    table = P.case_table(nan=False)
    assert table.dtype == np.float32 and table.size > 80
    assert np.array_equal(P.quantise(table, mode), _torch_rule(table, mode))
    rng = np.random.default_rng(16 + mode)
    v = np.concatenate([rng.uniform(-1.1, 1.1, 50000), rng.standard_normal(50000) * 0.2]).astype(np.float32)
    assert np.array_equal(P.quantise(v, mode), _torch_rule(v, mode))


def test_the_rules_differ_where_they_should():
    q0, q1 = P.quantise(P.case_table(), 0), P.quantise(P.case_table(), 1)
    assert q0[-1] == 0 and q1[-1] == 0                                         # NaN
    v = np.array([1.0, -1.0, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.99999, np.inf, -np.inf], np.float32)
    assert P.quantise(v, 0).tolist() == [32767, -32767, 0, 1, 2, -32766, 32767, -32768]
    assert P.quantise(v, 1).tolist() == [32767, -32768, 0, 2, 2, -32768, 32767, -32768]


def test_validate_refuses_before_any_file_is_read():
    from cleanumamba_amd.network import CleanUMamba
    from cleanumamba_amd.util.denoise_eval import validate
    nowhere = "/nonexistent/testset"
    with pytest.raises(ValueError, match="unknown batching"):
        validate(None, nowhere, batching="nope")
    _, cfg = load_ckpt("442k")
    net = CleanUMamba(**cfg)

    class Hooks:
        def prepare_input(self, x):
            return x

    class Finish:
        def finish_output(self, y):
            return y
    for proc in (Hooks(), Finish()):
        with pytest.raises(ValueError, match="network_processor"):
            validate(net, nowhere, network_processor=proc, batching="ragged")
    with pytest.raises(ValueError, match="quantize_audio_input"):
        validate(net, nowhere, quantize_audio_input=True, batching="ragged")
    with pytest.raises(ValueError, match="float32"):
        validate(CleanUMamba(**cfg).half(), nowhere, batching="ragged")
    with pytest.raises(ValueError, match="forward_ragged"):
        validate(torch.nn.Linear(4, 4), nowhere, batching="ragged")
    two_out = CleanUMamba(**dict(cfg, channels_output=2))
    with pytest.raises(ValueError, match="forward_ragged"):
        validate(two_out, nowhere, batching="ragged")
    # a processor without the two hooks and the default route are not refused: they get as far as the missing folder
    with pytest.raises(OSError):
        validate(net, nowhere, network_processor=object(), batching="ragged")
    with pytest.raises(OSError):
        validate(net, nowhere)


def test_from_flat_checks_on_fake_tensors():
    from cleanumamba_amd.util.metrics import Batch
    flat = torch.zeros(4000, dtype=torch.int16)                                # never touched: the tables are checked first
    with pytest.raises(ValueError, match="empty batch"):
        Batch.from_flat(flat, flat, [], 16000)
    with pytest.raises(ValueError, match="fewer than one 480-sample window"):
        Batch.from_flat(flat, flat, [480, 479], 16000)
    with pytest.raises(ValueError, match="at most 65535 clips"):
        Batch.from_flat(flat, flat, [480] * 65536, 16000)
    with pytest.raises(ValueError, match="offsets"):
        Batch.from_flat(flat, flat, [480, 480], 16000, offsets=[0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Batch.from_flat(flat, flat, [480, 480], 16000)
    with pytest.raises(ValueError, match="int16"):
        Batch.from_flat(flat.float(), flat, [480], 16000)


def test_new_entries_are_bound_and_reject_before_any_launch():
    from cleanumamba_amd import hip
    lib = hip.lib()
    assert "cum_unframe_rows_ragged_pcm16" in hip.SIGNATURES and "cum_pcm16_from_f32_ragged" in hip.SIGNATURES
    assert lib.cum_abi_version() == 16
    p = lambda a: ctypes.c_void_p(a)
    ok = dict(dt=hip.CUM_F32, rows=p(4096), B=2, lmax=100, T=128, len=p(4096), scale=p(4096), mode=0, out=p(4096), off=p(4096))

    def unframe(**kw):
        a = dict(ok, **kw)
        return lib.cum_unframe_rows_ragged_pcm16(a["dt"], a["rows"], a["B"], a["lmax"], a["T"], a["len"], a["scale"], a["mode"],
                                                 a["out"], a["off"], None)
    for bad in (dict(mode=2), dict(mode=-1), dict(B=0), dict(lmax=0), dict(T=99), dict(rows=None), dict(len=None),
                dict(out=None), dict(off=None), dict(dt=7), dict(rows=p(4104)), dict(len=p(4098)), dict(scale=p(4098)),
                dict(out=p(4097)), dict(off=p(4100))):
        assert unframe(**bad) == -1, bad
    assert b"mode" in (unframe(mode=2), lib.cum_last_error())[1]
    okf = dict(x=p(4096), B=2, lmax=100, stride=104, len=p(4096), mode=1, out=p(4096), off=p(4096))

    def from_f32(**kw):
        a = dict(okf, **kw)
        return lib.cum_pcm16_from_f32_ragged(a["x"], a["B"], a["lmax"], a["stride"], a["len"], a["mode"], a["out"], a["off"],
                                             None)
    for bad in (dict(mode=2), dict(B=0), dict(lmax=0), dict(stride=99), dict(x=None), dict(len=None), dict(out=None),
                dict(off=None), dict(x=p(4098)), dict(off=p(4100)), dict(out=p(4097))):
        assert from_f32(**bad) == -1, bad
