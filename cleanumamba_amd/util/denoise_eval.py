"""Validation while training (reference src/util/denoise_eval.py:validate): denoise a test set and score it.

The test set layouts are the reference's: DNS (``clean/clean_fileid_{i}.wav`` and ``noisy/*_fileid_{i}.wav``, or
``fileid_{i}.wav`` in both folders with ``validation=False``) and VCTK_DEMAND (the same file name in ``clean/`` and
``noisy/``).  Differences from the reference:
  * clips of equal length are denoised together, ``batch_size`` per ``forward`` (the DNS test clips are all 10 s); a
    batched forward need not be bit-identical to one clip at a time;
  * the denoised signal is quantised with ``* 32767``, clamped to the int16 range and cast (truncating); the reference's
    cast is unclamped and wraps on overshoot;
  * every clip is scored in one batched call on the GPU (cleanumamba_amd.util.python_eval.eval_waveforms); PESQ and
    the composites built on it are NaN unless the ``pesq`` package is installed.
  * ``metrics`` is accepted and, as in the reference, not used.
  * ``extra_metrics`` (not in the reference) names extended metrics of cleanumamba_amd.util.metrics.EXT_METRICS
    (``estoi``, ``si_sdr``, ``snr``, ``cep_dist``, ``fwsegSNR``); each adds a ``Test/<name>`` length-weighted sum.  An
    infinite or NaN clip value (a silent clip, an exact copy) makes that sum infinite or NaN.
  * ``resample=True`` takes a test set that is not at 16 kHz (VCTK-DEMAND and full-band DNS ship at 48 kHz): both files
    of such a pair are converted on the GPU (util/resample.py) before anything else, and the pair is denoised and scored
    at 16 kHz.  Without it such a pair is denoised as if it were 16 kHz and the metrics refuse its rate, as before.
  * ``batching="ragged"`` (opt-in; ``"length"`` is the route above, unchanged) keeps the audio on the device from the
    files to the scores: clips of ANY lengths share forwards (network/ragged.py ``denoise_batch_pcm16``), the last
    kernel of each forward quantises into one flat int16 buffer with the rule above, the clean signals stand in a second
    flat buffer with the same offsets, and both are scored where they are (``python_eval.eval_batch``).  With
    ``resample=True`` each source rate is converted a ragged batch per launch, the clean signal quantised on the device
    by the same ``(y * 32768).round().clamp(...)`` rule.  It takes mono pairs whose two files have one rate and one
    length, an f32 model on the fused conv stack and no per-tensor hooks (``network_processor``,
    ``quantize_audio_input``), and refuses anything else before a file is read.  A ragged forward is not bit-identical
    to the forward of an equal-length group, so the two routes' sums differ in the last digits.
"""
import concurrent.futures
import os

import numpy as np
import torch
from scipy.io import wavfile

from .python_eval import eval_waveforms

MODEL_RATE = 16000
READ_THREADS = 4
BATCHINGS = ("length", "ragged")
KEYS = ("pesq_wb", "pesq_nb", "stoi", "CSIG", "CBAK", "COVL", "wss_dist", "segSNR", "llr_mean", "count")


def _read_float(path):
    """(rate, (channels, samples) float32), int16 scaled by 1 / 32768 as torchaudio.load does."""
    rate, x = wavfile.read(path)
    if x.dtype == np.int16:
        x = x.astype(np.float32) / 32768.0
    elif x.dtype == np.int32:
        x = x.astype(np.float32) / 2147483648.0
    else:
        x = x.astype(np.float32)
    x = x.reshape(x.shape[0], -1).T if x.ndim == 2 else x[None]
    return rate, torch.from_numpy(np.ascontiguousarray(x))


def _to_model_rate(path, rate, device):
    """Channel rows of ``path`` at MODEL_RATE: (channels, M) float32 on the host, through ``resample_ragged`` -- from the
    int16 samples themselves where the file is 16-bit PCM, from ``_read_float``'s floats otherwise."""
    from .resample import resample_ragged
    _, x = wavfile.read(path)
    if x.dtype == np.int16:
        rows = torch.from_numpy(np.ascontiguousarray(x.reshape(x.shape[0], -1).T if x.ndim == 2 else x[None]))
    else:
        rows = _read_float(path)[1]
    rows = rows.contiguous().reshape(-1).reshape(rows.shape)     # (a numpy ``x[None]`` row comes with stride 0)
    y, lens = resample_ragged(rows.to(device), [rows.shape[1]] * rows.shape[0], rate, MODEL_RATE)
    return y[:, :lens[0]].cpu()


def _pairs(testset_path, validation, VCTK_DEMAND, test_factor):
    """[(clean path, noisy path)] in the reference's order; missing files are skipped as the reference skips them."""
    noisy_dir, clean_dir = os.path.join(testset_path, "noisy"), os.path.join(testset_path, "clean")
    noisy_files = os.listdir(noisy_dir)
    n = len(noisy_files) * (1 if VCTK_DEMAND else 2)
    out = []
    for i in range(int(n * test_factor)):
        if VCTK_DEMAND:
            if i >= len(noisy_files):
                continue
            c, nz = os.path.join(clean_dir, noisy_files[i]), os.path.join(noisy_dir, noisy_files[i])
        elif validation:
            c = os.path.join(clean_dir, "clean_fileid_{}.wav".format(i))
            match = [f for f in noisy_files if f.split("_")[-1][0:-4] == str(i)]
            if not match:
                continue
            nz = os.path.join(noisy_dir, match[0])
        else:
            c, nz = os.path.join(clean_dir, "fileid_{}.wav".format(i)), os.path.join(noisy_dir, "fileid_{}.wav".format(i))
        if os.path.exists(c) and os.path.exists(nz):
            out.append((c, nz))
    return out


def _check_ragged(net, quantize_audio_input, network_processor):
    """ValueError for what the ragged route cannot take -- from the arguments alone."""
    from ..network.ragged import ragged_supported
    if network_processor is not None and (hasattr(network_processor, "prepare_input")
                                          or hasattr(network_processor, "finish_output")):
        raise ValueError("validate: batching='ragged' does not run network_processor's prepare_input / finish_output "
                         "(they are per-tensor hooks); use batching='length'")
    if quantize_audio_input:
        raise ValueError("validate: batching='ragged' does not take quantize_audio_input; use batching='length'")
    params = list(getattr(net, "parameters", lambda: iter(()))())
    if any(p.dtype != torch.float32 for p in params if p.is_floating_point()):
        raise ValueError("validate: batching='ragged' takes float32 weights (autocast around the call is allowed); "
                         "a .half() model goes through batching='length'")
    if not ragged_supported(net):
        raise ValueError("validate: batching='ragged' needs a model forward_ragged runs: the fused conv stack (kernel 4 / "
                         "stride 2 / ungrouped / sigmoid-GLU layers) with one output channel")


def _host_clip(x):
    """A mono file's samples as ``denoise_batch`` takes them: int16 as it is, anything else as ``_read_float``'s float32."""
    if x.dtype == np.int16:
        return torch.from_numpy(np.ascontiguousarray(x))
    if x.dtype == np.int32:
        return torch.from_numpy(x.astype(np.float32) / 2147483648.0)
    return torch.from_numpy(np.ascontiguousarray(x.astype(np.float32)))


def _validate_ragged(net, pairs, result, device, crop, resample, extra_metrics, max_batch=32):
    """The ragged route of ``validate``: ``result`` filled from the pairs, the audio on the device throughout."""
    from ..network import ragged as rg
    from .metrics import Batch, _as_int16
    from .python_eval import eval_batch
    from .resample import out_length, plan

    def read(path):
        rate, x = wavfile.read(path)
        if x.ndim != 1:
            raise ValueError("validate: batching='ragged' takes mono files (%s has %d channels)" % (path, x.shape[1]))
        return rate, x
    with concurrent.futures.ThreadPoolExecutor(max_workers=READ_THREADS) as pool:
        files = list(pool.map(read, [p for pair in pairs for p in pair]))
    cleans, noisys = files[0::2], files[1::2]
    rates, lengths, convert = [], [], {}
    for i, ((rc, c), (rn, nz)) in enumerate(zip(cleans, noisys)):
        if rc != rn or c.shape[0] != nz.shape[0]:
            raise ValueError("validate: batching='ragged' takes pairs of one rate and one length (%s: clean %d samples at "
                             "%d Hz, noisy %d at %d Hz)" % (pairs[i][0], c.shape[0], rc, nz.shape[0], rn))
        if resample and rc != MODEL_RATE:
            p = plan(rc, MODEL_RATE)
            convert.setdefault(int(rc), []).append(i)
            rates.append(MODEL_RATE)
            lengths.append(out_length(c.shape[0], p.up, p.down))
        else:
            rates.append(int(rc))
            lengths.append(int(c.shape[0]))
    lengths = np.array(lengths, np.int64)
    offsets = (np.cumsum(lengths) - lengths).astype(np.int64)

    noisy = [_host_clip(nz) for _, nz in noisys]
    for rate, idx in convert.items():              # one launch per source rate and ``max_batch`` clips
        for i, y in zip(idx, rg._resample_group([noisy[i] for i in idx], rate, MODEL_RATE, device, max_batch)):
            noisy[i] = y
    flat, off2, len2 = rg.denoise_batch_pcm16(net, noisy, mode=0, max_batch=max_batch)
    assert np.array_equal(off2, offsets) and np.array_equal(len2, lengths)

    # the clean signals in a second flat buffer under the same table: files at their own rate staged and uploaded once,
    # converted ones quantised where the resampler left them
    converted = {i for idx in convert.values() for i in idx}
    if len(converted) < len(pairs):
        stage = torch.empty(flat.numel(), dtype=torch.int16, pin_memory=True)
        for i, (_, c) in enumerate(cleans):
            if i not in converted:
                stage[offsets[i]:offsets[i] + lengths[i]].copy_(_as_int16(c, "clean"))
        clean_flat = stage.to(device, non_blocking=True)
    else:
        clean_flat = torch.empty_like(flat)
    offsets_dev = torch.from_numpy(offsets).to(device) if convert else None
    for rate, idx in convert.items():
        rg._resample_group([_host_clip(cleans[i][1]) for i in idx], rate, MODEL_RATE, device, max_batch,
                           pcm16=(clean_flat, offsets_dev[torch.tensor(idx, device=device)], 1))

    # ``crop`` shortens clips where they stand: the batch's table keeps the offsets and takes the cropped lengths
    scored = lengths if crop is None else np.minimum(lengths, crop * np.array(rates, np.int64))
    for rate in sorted(set(rates)):
        sel = [i for i, r in enumerate(rates) if r == rate]
        batch = Batch.from_flat(clean_flat, flat, scored[sel], rate, offsets=offsets[sel])
        for r in eval_batch(batch, rate, extra=extra_metrics):
            for k in r:
                result["Test/" + k] += r[k]
    return result


def validate(net, testset_path, quantize_audio_input=False, network_processor=None, validation=True, VCTK_DEMAND=False,
             metrics=("pesq_wb", "pesq_nb", "stoi", "DNSMOS"), test_factor=1.0, crop=None, batch_size=16, resample=False,
             extra_metrics=(), batching="length"):
    """Denoise the test set with ``net`` and return the reference's dict of length-weighted sums ('Test/pesq_wb', ...,
    'Test/llr_mean') plus 'Test/count', the total length; divide by 'Test/count' for the means.

    resample: convert a pair whose header rate is not 16000 first, on the GPU: noisy from its samples to float32, clean
    likewise and back to int16 as ``(y * 32768).round().clamp(-32768, 32767)``; ``crop`` then counts seconds at 16 kHz.

    batching: "length" groups clips of equal length, ``batch_size`` per forward, and quantises and scores through the
    host; "ragged" batches clips of any lengths and keeps the audio on the device up to the per-clip scores (the module
    docstring: what it takes, and ValueError before any file is read for what it does not)."""
    from .metrics import EXT_METRICS
    if batching not in BATCHINGS:
        raise ValueError("validate: unknown batching %r (have %s)" % (batching, ", ".join(BATCHINGS)))
    if batching == "ragged":
        _check_ragged(net, quantize_audio_input, network_processor)
    extra_metrics = tuple(extra_metrics)
    for k in extra_metrics:                       # before any file is read or denoised
        if k not in EXT_METRICS:
            raise ValueError("validate: unknown extra metric %r (have %s)" % (k, ", ".join(EXT_METRICS)))
    result = {"Test/" + k: 0 for k in KEYS + extra_metrics}
    device, half = torch.device("cuda"), False
    for p in getattr(net, "parameters", lambda: iter(()))():
        device, half = p.device, p.dtype is torch.float16
        break
    if batching == "ragged":
        pairs = _pairs(testset_path, validation, VCTK_DEMAND, test_factor)
        return _validate_ragged(net, pairs, result, device, crop, resample, extra_metrics) if pairs else result

    clips = []                                    # (rate, clean int16, noisy (1, L) float32)
    for c, nz in _pairs(testset_path, validation, VCTK_DEMAND, test_factor):
        rate, clean = wavfile.read(c)
        if resample and rate != MODEL_RATE:
            noisy = _to_model_rate(nz, rate, device)
            clean = (_to_model_rate(c, rate, device)[0] * 32768).round().clamp(-32768, 32767).to(torch.int16).numpy()
            rate = MODEL_RATE
        else:
            _, noisy = _read_float(nz)
        clips.append((rate, clean, noisy))

    def prepare(x):
        if network_processor is not None and hasattr(network_processor, "prepare_input"):
            return network_processor.prepare_input(x)
        return x

    def finish(y):
        if network_processor is not None and hasattr(network_processor, "finish_output"):
            return network_processor.finish_output(y)
        return y

    denoised = [None] * len(clips)
    by_len = {}
    for i, (_, _, noisy) in enumerate(clips):
        by_len.setdefault(tuple(noisy.shape), []).append(i)
    with torch.no_grad():
        for idx in by_len.values():
            for s in range(0, len(idx), batch_size):
                part = idx[s:s + batch_size]
                x = torch.stack([prepare(clips[i][2]) for i in part]).to(device)
                if half:
                    x = x.half()
                y = finish(net(x)).float()
                q = (y * 32767).clamp(-32768, 32767).to(torch.int16).cpu().numpy()
                for j, i in enumerate(part):
                    denoised[i] = q[j].squeeze()

    cleans, targets, rates = [], [], []
    for (rate, clean, _), d in zip(clips, denoised):
        if crop is not None:
            clean, d = clean[:crop * rate], d[:crop * rate]
        cleans.append(clean)
        targets.append(d)
        rates.append(rate)
    if not cleans:
        return result
    for rate in sorted(set(rates)):
        sel = [i for i, r in enumerate(rates) if r == rate]
        for r in eval_waveforms([cleans[i] for i in sel], [targets[i] for i in sel], rate, extra=extra_metrics):
            for k in r:
                result["Test/" + k] += r[k]
    return result
