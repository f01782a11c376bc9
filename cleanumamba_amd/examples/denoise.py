"""Denoise every recording of a folder -- interface of src/examples/denoise.py:14-87.

  python -m cleanumamba_amd.examples.denoise -c CHECKPOINT -i NOISY_FOLDER -o OUTPUT_FOLDER

``denoise(checkpoint_path, input_directory, output_directory)`` returns ``(all_noisy_audio, all_cleaned_audio)``, two
lists of 1-D float32 numpy arrays, and writes ``enhanced_<name>`` as float32 WAV with ``scipy.io.wavfile.write``, as the
reference does.  Differences from the reference, on purpose:

  * files are taken in sorted name order (and the lists are returned in it); the reference's loader shuffles;
  * the reference runs one file per forward (``batch_size=1``).  Here files of different lengths share a forward:
    ``plan_batches`` (network/ragged.py) groups them by length under a batch, sample and padding-waste bound, at most 4
    threads read each batch as int16 into pinned memory (the next batch while the device runs the current one), the
    batch is uploaded once and denoised by ``model.forward_ragged``, whose result for every file equals its forward
    alone.  A file longer than ``budget_samples`` goes through ``model.denoise_long``;
  * a file whose sample rate is not 16000 raises ValueError naming the files, before any GPU work; the reference ignores
    the rate (torchaudio.load's second result is dropped, src/util/dataset.py:203) and so denoises such a file at the
    wrong rate.  With ``resample=True`` (``--resample``) such a file is converted to 16000 Hz on the GPU, denoised,
    converted back and written at its own rate and its own length (util/resample.py);
  * ``pcm16=True`` (``--pcm16``) writes (and returns) int16 PCM instead of float32: the last kernel of each forward
    quantises on the device, ``(y * 32768)`` rounded half to even and clamped (``denoise_batch_pcm16(mode=1)``), and
    the samples are downloaded as int16, half the bytes.  With ``resample=True`` the quantisation follows the conversion
    back to the file's own rate.  The default stays float32;
  * no ``torchinfo`` model summary is printed and there is no ``tqdm`` bar.
"""
import argparse
import concurrent.futures
import contextlib
import os

import numpy as np
import torch

from ..network import convstack as cs
from ..network.ragged import PCM_SCALE, pcm16_from_f32_ragged, plan_batches
from ..util.dataset import WAVE_FORMAT_PCM, NosyOnlyDataset, _read_whole_float
from ..util.resample import out_length, plan as resample_plan
from .loading_pretrained_models import load_pretrained_CleanUMamba

SAMPLE_RATE = 16000
READ_THREADS = 4


def check_rates(dataset, sample_rate=SAMPLE_RATE):
    """ValueError naming every file of the folder whose header gives another rate (host only: headers are parsed)."""
    bad = [f"{name} ({dataset.info(n).rate} Hz)" for n, name in enumerate(dataset.noisy_files)
           if dataset.info(n).rate != sample_rate]
    if bad:
        raise ValueError(f"denoise: the model runs at {sample_rate} Hz and nothing here resamples (resample=True / "
                         f"--resample converts); other rates in "
                         f"{dataset.folder}: " + ", ".join(bad))


def _is_pcm16(info):
    return info.tag == WAVE_FORMAT_PCM and info.bits == 16


def _stage(dataset, indices, pool):
    """Start reading the files ``indices`` into one pinned (B, pitch) tensor: int16 if every file is 16-bit PCM, else
    float32.  -> (pinned tensor, lengths, futures)."""
    infos = [dataset.info(n) for n in indices]
    lengths = [info.frames for info in infos]
    pitch = cs.rup(max(lengths), 8)
    raw = all(_is_pcm16(info) for info in infos)
    stage = torch.empty(len(indices), pitch, dtype=torch.int16 if raw else torch.float32, pin_memory=True)

    def read(b, n):
        row = stage[b].numpy()
        if raw:
            dataset.read_pcm(n, out=row)
        else:
            x = _read_whole_float(infos[b].path)[1]
            row[:len(x)] = x
    return stage, lengths, [pool.submit(read, b, n) for b, n in enumerate(indices)]


def _clip_f32(row):
    return row.to(torch.float32) * PCM_SCALE if row.dtype == torch.int16 else row


def _quantise(cleans, device, mode=1):
    """1-D f32 clips (host or device) -> their int16 PCM as host arrays: one quantising launch into one flat device
    buffer (``pcm16_from_f32_ragged``), one int16 download."""
    lens = np.array([int(c.shape[0]) for c in cleans], np.int64)
    offsets = np.cumsum(lens) - lens
    rows = torch.nn.utils.rnn.pad_sequence([c.to(device) for c in cleans], batch_first=True).contiguous()
    flat = torch.empty(int(lens.sum()), dtype=torch.int16, device=device)
    pcm16_from_f32_ragged(rows, torch.from_numpy(lens.astype(np.int32)).to(device), flat,
                          torch.from_numpy(offsets).to(device), mode)
    host = flat.cpu()
    return [host[o:o + n] for o, n in zip(offsets.tolist(), lens.tolist())]


def denoise(checkpoint_path, input_directory, output_directory=None, *, max_batch=32, budget_samples=32 * 160000,
            autocast_dtype=None, resample=False, pcm16=False):
    """
    Denoise audio

    Parameters:
    checkpoint_path (str):          path to the checkpoint to load
    input_directory (str):          denoise noisy audio from this path
    output_directory (str/None):    save generated speeches to this path if provided
    max_batch, budget_samples:      bounds of one ragged batch (network/ragged.py plan_batches)
    autocast_dtype:                 torch.float16 / torch.bfloat16 to run under autocast, None for float32
    resample:                       take files at any sample rate: each is converted to the model's rate, denoised,
                                    converted back and written (and returned) at its own rate and length
    pcm16:                          write (and return as all_cleaned_audio) int16 PCM, quantised on the device by
                                    ``(y * 32768).round().clamp(-32768, 32767)``, instead of float32
    """
    dataset = NosyOnlyDataset(folder=input_directory)
    rates = [dataset.info(n).rate for n in range(len(dataset))]
    if resample:
        plans = {r: resample_plan(r, SAMPLE_RATE) for r in set(rates)}     # ValueError for a rate that cannot be converted
    else:
        check_rates(dataset)

    model = load_pretrained_CleanUMamba(checkpoint_path)
    model.eval()

    if output_directory is not None and output_directory != '':
        print(f"output_directory: {output_directory}")
        if not os.path.isdir(output_directory):
            os.makedirs(output_directory)
            os.chmod(output_directory, 0o775)

    from scipy.io.wavfile import write as wavwrite
    device = next(model.parameters()).device
    lengths = [dataset.info(n).frames for n in range(len(dataset))]
    if resample:                                                           # batches hold what the model will see
        lengths = [out_length(n, plans[r].up, plans[r].down) for n, r in zip(lengths, rates)]
    batches = plan_batches(lengths, model.valid_length, max_batch=max_batch, budget_samples=budget_samples)
    all_noisy_audio, all_cleaned_audio = [None] * len(dataset), [None] * len(dataset)
    amp = torch.autocast("cuda", dtype=autocast_dtype) if autocast_dtype is not None else contextlib.nullcontext()
    with concurrent.futures.ThreadPoolExecutor(max_workers=READ_THREADS) as pool, torch.no_grad(), amp:
        staged = _stage(dataset, batches[0].indices, pool) if batches else None
        for k, batch in enumerate(batches):
            stage, lens, reads = staged
            for r in reads:
                r.result()
            # the next batch is read while the device runs this one
            staged = _stage(dataset, batches[k + 1].indices, pool) if k + 1 < len(batches) else None
            brates = [rates[n] for n in batch.indices]
            if pcm16 and all(r == SAMPLE_RATE for r in brates):
                # the batch as planned (its clips alone plan into the same one batch), quantised by its last kernel
                flat, offs, _ = model.denoise_batch_pcm16([stage[b, :lens[b]] for b in range(len(lens))], mode=1,
                                                          max_batch=max_batch, budget_samples=budget_samples)
                flat = flat.cpu()                                          # int16: half the bytes of the f32 result
                cleans = [flat[o:o + n] for o, n in zip(offs.tolist(), lens)]
            elif all(r == SAMPLE_RATE for r in brates):
                if batch.long:
                    clean = model.denoise_batch([stage[0, :lens[0]]], max_batch=max_batch, budget_samples=budget_samples)[0]
                    clean = clean.view(1, 1, -1)
                else:
                    rows = stage.to(device, non_blocking=True)             # one upload per batch
                    clean = model.forward_ragged(rows[:, :max(lens)], lens)
                clean = clean.cpu()
                cleans = [clean[b, 0, :lens[b]] for b in range(len(lens))]
            elif batch.long:                                               # host in, host out: a piece at a time
                cleans = [model.denoise_long(_clip_f32(stage[0, :lens[0]]).view(1, -1), rate=brates[0])[0, 0]]
            else:
                cleans = model.denoise_batch([stage[b, :lens[b]] for b in range(len(lens))], max_batch=max_batch,
                                             budget_samples=budget_samples, rates=brates)
                cleans = cleans if pcm16 else [c.cpu() for c in cleans]    # (quantised below, where they are)
            if pcm16 and cleans[0].dtype != torch.int16:                   # converted back to the files' rates first
                cleans = _quantise(cleans, device)
            for b, n in enumerate(batch.indices):
                noisy = stage[b, :lens[b]].numpy()
                noisy = noisy.astype(np.float32) * np.float32(PCM_SCALE) if noisy.dtype == np.int16 else noisy.copy()
                generated = cleans[b].numpy().copy()
                if output_directory:
                    wavwrite(os.path.join(output_directory, f'enhanced_{dataset.noisy_files[n]}'), brates[b], generated)
                all_noisy_audio[n] = noisy
                all_cleaned_audio[n] = generated
    return all_noisy_audio, all_cleaned_audio


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument('-c', '--checkpoint_path', default='checkpoints/pruned/CleanUMamba-3N-E8_pruned-5M.pkl',
                        help='Path to the checkpoint')
    parser.add_argument('-i', '--input_directory', type=str, required=True,
                        help='Input folder path to load noisy only data from')
    parser.add_argument('-o', '--output_directory', type=str, default=None,
                        help='Output folder path to save the audio to')
    parser.add_argument('--max_batch', type=int, default=32, help='Most files in one forward')
    parser.add_argument('--autocast', choices=['f16', 'bf16'], default=None, help='Run under autocast in this type')
    parser.add_argument('--pcm16', action='store_true',
                        help='Write int16 PCM (quantised on the GPU, round half to even) instead of float32')
    parser.add_argument('--resample', action='store_true',
                        help='Take files at any sample rate: convert to 16000 Hz, denoise, write at the file\'s own rate')
    args = parser.parse_args()
    denoise(args.checkpoint_path, args.input_directory, args.output_directory, max_batch=args.max_batch,
            autocast_dtype={None: None, 'f16': torch.float16, 'bf16': torch.bfloat16}[args.autocast], resample=args.resample,
            pcm16=args.pcm16)
