"""The reference's evaluation functions (src/util/python_eval.py) with its signatures, numpy in and numpy out, computed
on the GPU by cleanumamba_amd.util.metrics.

Deviations, by design:
  * ``snr`` returns the overall SNR computed in float.  The reference squares the int16 arrays in int16 arithmetic,
    which wraps; ``eval_waveform`` never reports that value.
  * PESQ is not reimplemented.  When the ``pesq`` package imports, it is called on the CPU as the reference calls it;
    otherwise ``pesq_wb``, ``pesq_nb`` and the composites built on PESQ (CSIG, CBAK, COVL) are NaN, with one warning.
  * The frame metrics exist at 16 kHz only (the reference's eval_waveform calls them at 16 kHz whatever the rate).

Beyond the reference: ``cepstrum_distance``, ``fwsegsnr`` and ``si_sdr`` mirror the extended metrics of
cleanumamba_amd.util.metrics (restated published definitions, not compared with pysepm, pystoi or torchmetrics), and
``eval_waveforms(..., extra=...)`` adds any of ``metrics.EXT_METRICS`` to its result dicts.
"""
import math
import warnings
from collections import defaultdict

import numpy as np

from . import metrics as M

_PESQ_WARNED = False


def _pesq_fn():
    global _PESQ_WARNED
    try:
        from pesq import pesq
        return pesq
    except ImportError:
        if not _PESQ_WARNED:
            warnings.warn("pesq is not installed: pesq_wb, pesq_nb, CSIG, CBAK and COVL are NaN")
            _PESQ_WARNED = True
        return None


def _same_length(a, b, msg):
    if np.size(a) != np.size(b):
        raise ValueError(msg)


def _frames(clean_speech, processed_speech, sample_rate, name):
    if sample_rate != M.FRAME_RATE:
        raise ValueError("%s: only 16 kHz is supported (got %r)" % (name, sample_rate))
    return M.frame_metrics([np.asarray(clean_speech)], [np.asarray(processed_speech)], sample_rate)


def wss(clean_speech, processed_speech, sample_rate):
    """Per-frame weighted spectral slope distortion (python_eval.py:139)."""
    _same_length(clean_speech, processed_speech, "Files must have same length.")
    return _frames(clean_speech, processed_speech, sample_rate, "wss")["wss"][0].cpu().numpy()


def llr(clean_speech, processed_speech, sample_rate):
    """Per-frame log-likelihood ratio of order-16 LPC (python_eval.py:336); NaN where a frame is all zeros."""
    _same_length(clean_speech, processed_speech, "Both Speech Files must be same length.")
    return _frames(clean_speech, processed_speech, sample_rate, "llr")["llr"][0].cpu().numpy()


def snr(clean_speech, processed_speech, sample_rate):
    """(overall SNR, per-frame segmental SNR clamped to [-10, 35] dB) (python_eval.py:409).  The overall SNR is computed
    in float (the reference's int16 arithmetic wraps)."""
    _same_length(clean_speech, processed_speech, "Both Speech Files must be same length.")
    c = np.asarray(clean_speech, np.float64)
    p = np.asarray(processed_speech, np.float64)
    overall = 10 * np.log10(np.sum(np.square(c)) / np.sum(np.square(c - p)))
    seg = _frames(clean_speech, processed_speech, sample_rate, "snr")["segSNR"][0].cpu().numpy()
    return overall, seg


def cepstrum_distance(clean_speech, processed_speech, sample_rate):
    """Per-frame LPC cepstrum distance (Hu & Loizou 2008), limited to [0, 10]; NaN where a frame is all zeros."""
    _same_length(clean_speech, processed_speech, "Both Speech Files must be same length.")
    if sample_rate != M.FRAME_RATE:
        raise ValueError("cepstrum_distance: only 16 kHz is supported (got %r)" % (sample_rate,))
    fm = M.frame_metrics([np.asarray(clean_speech)], [np.asarray(processed_speech)], sample_rate, extended=True)
    return fm["cep"][0].cpu().numpy()


def fwsegsnr(clean_speech, processed_speech, sample_rate):
    """Per-frame frequency-weighted segmental SNR (Hu & Loizou 2008), limited to [-10, 35] dB; NaN where the clean frame
    is silent."""
    _same_length(clean_speech, processed_speech, "Both Speech Files must be same length.")
    if sample_rate != M.FRAME_RATE:
        raise ValueError("fwsegsnr: only 16 kHz is supported (got %r)" % (sample_rate,))
    fm = M.frame_metrics([np.asarray(clean_speech)], [np.asarray(processed_speech)], sample_rate, extended=True)
    return fm["fwseg"][0].cpu().numpy()


def si_sdr(clean, processed):
    """Scale-invariant SDR in dB (Le Roux et al. 2019, no mean removal) of one clip, from exact integer sums."""
    _same_length(clean, processed, "Both Speech Files must be same length.")
    return float(M.speech_metrics([np.asarray(clean)], [np.asarray(processed)], metrics=("si_sdr",))["si_sdr"][0])


def composites(pesq_mos, llr_mean, wss_dist, seg_snr):
    """CSIG, CBAK, COVL (Hu & Loizou 2008) limited to [1, 5]; NaN when PESQ is NaN."""
    if math.isnan(pesq_mos):
        return float("nan"), float("nan"), float("nan")
    lim = lambda v: min(5, max(1, v))
    csig = lim(3.093 - 1.029 * llr_mean + 0.603 * pesq_mos - 0.009 * wss_dist)
    cbak = lim(1.634 + 0.478 * pesq_mos - 0.007 * wss_dist + 0.063 * seg_snr)
    covl = lim(1.594 + 0.805 * pesq_mos - 0.512 * llr_mean - 0.007 * wss_dist)
    return csig, cbak, covl


def eval_waveforms(cleans, targets, rate, extra=()):
    """eval_waveform of every (clean, target) pair, with all clips scored in one batched call: a list of result dicts.
    ``extra``: names of ``metrics.EXT_METRICS`` to add as length-weighted sums like the rest (``cep_dist`` and
    ``fwsegSNR`` at 16 kHz like the other frame metrics, ``estoi``, ``si_sdr`` and ``snr`` at ``rate``)."""
    extra = tuple(extra)
    for k in extra:
        if k not in M.EXT_METRICS:
            raise ValueError("eval_waveforms: unknown extra metric %r (have %s)" % (k, ", ".join(M.EXT_METRICS)))
    ext_frame = tuple(k for k in extra if k in ("cep_dist", "fwsegSNR"))
    ext_rate = tuple(k for k in extra if k not in ext_frame)
    m = M.speech_metrics(cleans, targets, M.FRAME_RATE, metrics=("wss_dist", "llr_mean", "segSNR") + ext_frame)
    at_rate = M.speech_metrics(cleans, targets, rate, metrics=("stoi",) + ext_rate)
    st = at_rate.pop("stoi")
    m.update(at_rate)
    m = {k: v.cpu().numpy() for k, v in m.items()}
    st = st.cpu().numpy()
    pesq = _pesq_fn()
    out = []
    for i, (clean, target) in enumerate(zip(cleans, targets)):
        clean, target = np.asarray(clean), np.asarray(target)
        length = target.shape[-1]
        wss_dist, llr_mean, seg = float(m["wss_dist"][i]), float(m["llr_mean"][i]), float(m["segSNR"][i])
        if pesq is not None:
            pesq_wb, pesq_nb = pesq(16000, clean, target, "wb"), pesq(16000, clean, target, "nb")
        else:
            pesq_wb = pesq_nb = float("nan")
        csig, cbak, covl = composites(pesq_wb, llr_mean, wss_dist, seg)
        result = defaultdict(int)
        result["pesq_wb"] += pesq_wb * length
        result["pesq_nb"] += pesq_nb * length
        result["stoi"] += float(st[i]) * length
        result["CSIG"] += csig * length
        result["CBAK"] += cbak * length
        result["COVL"] += covl * length
        result["wss_dist"] += wss_dist * length
        result["segSNR"] += seg * length
        result["llr_mean"] += llr_mean * length
        result["count"] += 1 * length
        for k in extra:
            result[k] += float(m[k][i]) * length
        out.append(result)
    return out


def eval_batch(batch, rate, extra=()):
    """``eval_waveforms`` on one resident ``metrics.Batch`` (``Batch.from_flat``: both signals already on the device as
    flat int16 buffers): the same list of result dicts, from the same kernels -- the frame metrics on the batch at
    16 kHz, STOI and the rate metrics on the same buffers at ``rate``, with no copy and no second upload.  Only the
    per-clip scalars come back to the host; the int16 clips are downloaded for PESQ only where ``pesq`` imports."""
    extra = tuple(extra)
    for k in extra:
        if k not in M.EXT_METRICS:
            raise ValueError("eval_batch: unknown extra metric %r (have %s)" % (k, ", ".join(M.EXT_METRICS)))
    ext_frame = tuple(k for k in extra if k in ("cep_dist", "fwsegSNR"))
    ext_rate = tuple(k for k in extra if k not in ext_frame)
    m = M.speech_metrics(batch, None, M.FRAME_RATE, metrics=("wss_dist", "llr_mean", "segSNR") + ext_frame)
    at_rate = M.speech_metrics(batch, None, rate, metrics=("stoi",) + ext_rate)
    st = at_rate.pop("stoi")
    m.update(at_rate)
    m = {k: v.cpu().numpy() for k, v in m.items()}
    st = st.cpu().numpy()
    pesq = _pesq_fn()
    if pesq is not None:
        clean_host, target_host = batch.clean.cpu().numpy(), batch.processed.cpu().numpy()
    out = []
    for i in range(batch.n_clips):
        length = int(batch.lengths[i])
        wss_dist, llr_mean, seg = float(m["wss_dist"][i]), float(m["llr_mean"][i]), float(m["segSNR"][i])
        if pesq is not None:
            o = int(batch.offsets[i])
            clean, target = clean_host[o:o + length], target_host[o:o + length]
            pesq_wb, pesq_nb = pesq(16000, clean, target, "wb"), pesq(16000, clean, target, "nb")
        else:
            pesq_wb = pesq_nb = float("nan")
        csig, cbak, covl = composites(pesq_wb, llr_mean, wss_dist, seg)
        result = defaultdict(int)
        result["pesq_wb"] += pesq_wb * length
        result["pesq_nb"] += pesq_nb * length
        result["stoi"] += float(st[i]) * length
        result["CSIG"] += csig * length
        result["CBAK"] += cbak * length
        result["COVL"] += covl * length
        result["wss_dist"] += wss_dist * length
        result["segSNR"] += seg * length
        result["llr_mean"] += llr_mean * length
        result["count"] += 1 * length
        for k in extra:
            result[k] += float(m[k][i]) * length
        out.append(result)
    return out


def eval_waveform(clean, target_wav, rate):
    """Length-weighted metrics of one clip (python_eval.py:81): pesq_wb, pesq_nb, stoi, CSIG, CBAK, COVL, wss_dist,
    segSNR, llr_mean and count.  The frame metrics run at 16 kHz, STOI at ``rate``, as in the reference."""
    return eval_waveforms([clean], [target_wav], rate)[0]
