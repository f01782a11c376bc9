"""Batches for the train step straight from a dataset directory: the other half of the reference's hot loop
(src/training/train.py:255-260 -- ``for clean_audio, noisy_audio, _, _ in trainloader: clean_audio = clean_audio.cuda()``).

The reference's loader decodes both files of a pair to float on the CPU, crops, collates, and the loop uploads two float
batches from pageable memory on the compute stream.  Here the samples stay int16 until they are on the device:

  worker threads   dataset.read_pcm(index, start, count) straight into a pinned staging slot (the only time the host
                   touches a sample);
  next()           one ``copy_(non_blocking=True)`` of the slot -- the int16 rows of both signals and the table of clip
                   lengths -- on the feeder's own stream, followed by an event.  The upload of batch k + 1 is issued
                   while batch k is handed out, into one of depth + 1 device blocks, so it runs beside the steps
                   before the one that uses it;
  PcmBatch.into()  the current stream waits for that event (the host does not), and one launch of cum_pcm_batch_f32
                   (csrc/pcm.hip) scales to float and tiles short clips into the tensors it is given -- for a replayed
                   TrainStep these are the captured graph's own input buffers, so no float batch is ever copied.

One scheduler owns all randomness: the order and the crop starts of epoch e come from
``numpy.random.Generator(PCG64([seed, e]))`` and do not depend on the number of workers, on timing, or on the rank count
beyond the documented sharding, so a run can be repeated and resumed.

Every call into the GPU runtime is made on the consumer's thread (inside ``next()`` / ``into()``); the workers only read
files.  A worker can therefore never disturb a hipGraph capture that the consumer's thread has open, and the consumer
never calls ``next()`` while it captures.

``BatchFeeder(..., sample_rate=16000)`` -- a RATED feeder -- takes pairs at any sample rate (VCTK-DEMAND and full-band
DNS ship at 48 kHz; the reference feeds such a pair to the 16 kHz model as if it were 16 kHz, src/util/dataset.py:110-115).
The crop is drawn in model-rate samples; the workers read the file-rate window its outputs read (util/resample.py:
``crop_window``), still int16, into rows sized by ``window_bound``; one record per pair -- plan, window, position --
travels in the slot's tail in the same single upload; and ``into()`` launches cum_pcm_batch_resample_f32
(csrc/resample.hip) instead: the polyphase chains of DESIGN.md 7g from the int16 windows straight into the step's input
buffers, bit-identical to ``resample_ragged`` on the whole file, sliced.  Pairs at the model rate pass through it with
cum_pcm_batch_f32's arithmetic, so an all-16 kHz dataset gives the unrated feeder's plan and batches.  Without
``sample_rate`` no header rate is read and nothing here changes.

``BatchFeeder(..., augment=Augment(...))`` (training/augment.py) augments every batch on that last step:
the plan crops ``shift`` samples more, the batch's draws -- from a generator of their own per (seed, epoch, rank, batch)
-- ride in the slot's tail in the same upload, the assembling kernel writes the longer crops into float scratch the
feeder owns, and cum_augment_pairs (csrc/augment.hip) writes the batch into the step's inputs.  With a ``band_mask`` in
the config the band records follow the draw table in the same upload, and cum_band_mask_pairs (csrc/bandmask.hip) runs
between the two, from that scratch into a second pair the block owns.  With a ``reverb`` in the config the room records
follow the band records (or the draw table), still in the one upload; the bank of responses goes to the device once, at
construction, in uploads of its own; and cum_reverb_pairs (csrc/reverb.hip) runs first: assemble -> A, reverb A -> B,
band B -> A, augment A -> the step's inputs (two scratch pairs, never a third).  Without ``augment`` nothing here changes.

``BatchFeeder(SpeechNoiseDataset(...), ..., mix=Mix(...))`` (util/dataset.py, training/mix.py) -- a MIXING
feeder -- trains from separate speech and noise corpora, as the DNS challenge distributes them, without the offline
synthesiser: the plan above orders and crops the SPEECH files (one no longer than the crop is read whole and repeated
on the device); every row's noise is laid out afresh each epoch by a generator of its own per (seed, epoch, rank, batch,
row) -- pieces of random noise files from a random start to their end, ``gap`` zeros behind each, at most ``max_pieces``
of them, the last one cut (``noise_plan``); the workers read the speech crop into the clean row and the pieces into the
noisy row of the slot; the batch's SNR and level draws ride in the slot's tail as the records of cum_mix_pairs, in the
one upload; and ``into()`` launches cum_mix_pairs (csrc/mix.hip) in the assembling kernel's place: noise scaled to an SNR
against the active level of both signals, the mixture brought to a level in dBFS, a guard against clipping, straight
into the step's inputs -- or, with ``augment``, over the longer crops into the scratch the chain above reads, which
follows unchanged.  ``PcmBatch.mix_stats()`` is the rows' device table of what was applied.  ``workers=0`` (a mixing
feeder only) reads in ``next()`` itself.  Without ``mix`` nothing here changes.

``device="cpu"`` keeps the same pipeline without pinning or streams and does the kernel's arithmetic with torch on the
host, so the loop runs anywhere -- a rated feeder too, as long as every pair is at the model rate: there is no CPU
resampler (util/resample.py), so any other rate is a ValueError at construction.  A mixing feeder on the CPU runs
``mix.apply``'s NumPy arithmetic.
"""
import ctypes
import inspect
import threading
import time

import numpy as np
import torch

from .. import hip
from ..util import resample as rs
from . import augment as aug
from . import mix as mx

SAMPLE_RATE = 16000
PCM_SCALE = 1.0 / 32768.0


def _round_up(n, m):
    return (n + m - 1) // m * m


class _Slot:
    """One block of ``2 * batch * pitch`` int16 samples followed by ``batch`` int32 clip lengths -- in a rated feeder by
    ``batch`` records of 16 int32, in a mixing feeder by ``batch`` records of 12 -- and, in an augmenting feeder, by
    ``aug_ints`` int32 of draw table (with a band mask: the band records behind it, with a reverb: the room records behind
    those), as one int16 tensor so that it moves in one copy."""

    def __init__(self, batch, pitch, device, pin, tail_ints=1, aug_ints=0):
        self.batch, self.pitch = batch, pitch
        self._aug = 2 * batch * pitch + 2 * tail_ints * batch       # an augmenting feeder's draw table starts here
        self.flat = torch.zeros(self._aug + 2 * aug_ints, dtype=torch.int16, device=device, pin_memory=pin)
        self.scratch = self.workspace = None     # device blocks of an augmenting feeder: the L + S float crops, tile sums
        self.band_scratch = self.band_workspace = None       # ... with a band mask or a reverb: the second pair; the spectra
        self.reverb_workspace = None                         # ... with a reverb: its spectra
        self.mix_workspace = self.mix_stats = None           # device blocks of a mixing feeder: the totals; the rows' stats
        self.seq = -1                # the batch this block holds
        self.uploaded = None         # event after the upload (device blocks on a GPU)
        self.released = []           # events after the assembling kernels that read this block

    def rows(self, nb):
        """(2, nb, pitch) int16 view: [0] the clean rows, [1] the noisy rows of a batch of nb clips."""
        return self.flat[:2 * nb * self.pitch].view(2, nb, self.pitch)

    def src_len(self):
        return self.flat[2 * self.batch * self.pitch:self._aug].view(torch.int32)

    def aug_table(self, ints):
        """The first ``ints`` int32 of the draw table (training/augment.py: AugmentDraws.pack)."""
        return self.flat[self._aug:self._aug + 2 * ints].view(torch.int32)

    def band_table(self, at, ints):
        """``ints`` int32 of band records (AugmentDraws.pack_band) or room records (pack_reverb) that start ``at`` int32
        behind the start of the draw table."""
        return self.flat[self._aug + 2 * at:self._aug + 2 * (at + ints)].view(torch.int32)

    def mix_records(self):
        """(batch, 12) int32 view of a mixing slot's tail: the records of cum_mix_pairs (8-byte aligned likewise)."""
        return self.flat[2 * self.batch * self.pitch:self._aug].view(torch.int32).view(self.batch, mx.REC_INTS)

    def records(self):
        """(batch, 16) int32 view of a rated slot's tail (8-byte aligned: a row is 16 bytes times a whole number)."""
        return self.flat[2 * self.batch * self.pitch:self._aug].view(torch.int32).view(self.batch, rs.REC_INTS)


class _Pending:
    """A batch on its way through the staging slots."""

    def __init__(self, seq, epoch, entries, windows=None, records=None, draws=None, table=None, band=None,
                 rooms=None):
        self.seq, self.epoch, self.entries = seq, epoch, entries
        self.mix = self.mix_table = self.noise = None        # a mixing feeder's: MixDraws, its (nb, 12) records, the noise plan
        self.windows, self.records = windows, records        # a rated feeder's: [(m0, M, rate)], (nb, 16) int32 on the host
        self.draws, self.table = draws, table                # an augmenting feeder's: AugmentDraws, its packed int32 table
        self.band = band                                     # ... with a band mask: its packed band records
        self.rooms = rooms                                   # ... with a reverb: its packed room records
        self.todo = len(entries)     # rows not read yet
        self.error = None


class PcmBatch:
    """What ``BatchFeeder.next()`` returns: the int16 crops of one batch on the feeder's device.

    fileids: [(clean path, noisy path)] per clip;  entries: the plan's (index, start, count) per clip -- the samples read
    from the files;  epoch;  shape: the (B, 1, L) of the float tensors it assembles;  windows (a rated feeder's, else
    None): [(m0, M, rate)] per clip -- the clip is outputs [m0, m0 + L) of its file's M model-rate samples, or, with
    M <= L, all of them repeated;  draws (an augmenting feeder's, else None): the batch's ``AugmentDraws`` -- the plan's
    crops are then ``draws.shift`` samples longer than L, and ``into`` applies the draws to them.  From a mixing feeder
    (``mix=``): entries are the speech reads, fileids the speech paths, ``noise`` the noise rows' plan ([(noise file, start,
    count, position in the row)] per clip) and ``mix`` the batch's ``MixDraws``."""

    def __init__(self, feeder, seq, epoch, entries, slot, windows=None, records=None, draws=None, mix=None, noise=None):
        self._feeder, self._seq, self._slot = feeder, seq, slot
        self.epoch, self.entries = epoch, entries
        self.windows, self._records, self.draws = windows, records, draws
        self.mix, self.noise = mix, noise
        files = getattr(feeder.dataset, "files", None)
        if mix is not None:
            self.fileids = [feeder.dataset.speech_files[i] for i, _, _ in entries]
        else:
            self.fileids = [tuple(files[i]) if files is not None else i for i, _, _ in entries]
        self.device = feeder.device
        self.shape = torch.Size((len(entries), 1, feeder.crop_length))
        self.uploaded = slot.uploaded        # the event after this batch's upload (None on the CPU)

    def _live_slot(self):
        slot = self._slot
        if self._feeder._returned > self._seq + self._feeder.depth or slot.seq != self._seq:
            raise RuntimeError(f"PcmBatch {self._seq} was used after {self._feeder.depth} further next() calls: its "
                               "device slot holds another batch now (raise `depth` to keep batches longer)")
        return slot

    def into(self, clean, noisy):
        """Assemble the float batch into ``clean`` and ``noisy`` ((B, 1, L) or (B, L) float32 on the feeder's device,
        unit stride along time, 16-byte aligned) on the current stream.  Nothing here waits on the host."""
        slot = self._live_slot()
        nb, length = self.shape[0], self.shape[2]
        strides = []
        for name, t in (("clean", clean), ("noisy", noisy)):
            if t.dtype != torch.float32 or t.device != self.device or tuple(t.shape) not in ((nb, 1, length), (nb, length)):
                raise ValueError(f"PcmBatch.into: {name} must be a float32 {tuple(self.shape)} tensor on {self.device}; "
                                 f"got {t.dtype} {tuple(t.shape)} on {t.device}")
            if t.stride(-1) != 1 and length > 1:
                raise ValueError(f"PcmBatch.into: {name} must have unit stride along time")
            strides.append(t.stride(0) if nb > 1 else length)
        out_clean, out_noisy, out_strides = clean, noisy, strides
        if self.draws is not None:           # assemble the crops of length + shift samples, then augment into the outputs
            length += self.draws.shift
        if self.device.type == "cpu":
            if self.draws is not None:
                clean, noisy = torch.empty(nb, length), torch.empty(nb, length)
                strides = [length, length]
            rows = slot.rows(nb)
            if self.mix is not None:         # speech row, noise row -> (clean, noisy): training/mix.py on the host
                outs = [torch.as_strided(t, (nb, length), (sb, 1)) for t, sb in ((clean, strides[0]), (noisy, strides[1]))]
                mx.apply(rows[0][:, :length], slot.mix_records()[:nb, mx.REC_N_SPEECH], rows[1][:, :length], self.mix,
                         outs[0], outs[1], slot.mix_stats[:nb])
            else:
                n = slot.src_len()[:nb] if self._records is None else slot.records()[:nb, rs.FEED_N_SRC]     # (model rate)
                n = n.to(torch.int64).clamp(1, length)
                idx = torch.arange(length)[None, :] % n[:, None]
                for t, sb, src in ((clean, strides[0], rows[0]), (noisy, strides[1], rows[1])):
                    out = torch.as_strided(t, (nb, length), (sb, 1))
                    out.copy_(torch.gather(src, 1, idx).to(torch.float32) * PCM_SCALE)
            if self.draws is not None:
                aug.apply(clean, noisy, self.draws, out_clean, out_noisy, reverb=self._feeder.augment.reverb)
            return out_clean, out_noisy
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream()
            stream.wait_event(slot.uploaded)
            if self.draws is not None:       # the block's own float scratch: the release events below cover it too
                clean, noisy = slot.scratch
                strides = [clean.stride(0), noisy.stride(0)]
            if self.mix is not None:         # in the assembling kernel's place: csrc/mix.hip, three launches
                mx.launch(slot.flat, slot.pitch, slot.mix_records(), nb, length, slot.mix_workspace, clean, strides[0],
                          noisy, strides[1], slot.mix_stats)
            elif self._records is None:
                hip.check(hip.lib().cum_pcm_batch_f32(hip.ptr(slot.flat), slot.pitch, hip.ptr(slot.src_len()), nb, length,
                                                      hip.ptr(clean), strides[0], hip.ptr(noisy), strides[1],
                                                      ctypes.c_void_p(stream.cuda_stream)))
            else:
                hip.check(hip.lib().cum_pcm_batch_resample_f32(
                    hip.ptr(slot.flat), slot.pitch, hip.ptr(self._records), hip.ptr(slot.records()), nb,
                    *self._feeder._rs.args(), length, hip.ptr(clean), strides[0], hip.ptr(noisy), strides[1],
                    ctypes.c_void_p(stream.cuda_stream)))
            other = slot.band_scratch        # the stages ping-pong between the block's two pairs
            if self.draws is not None and self._feeder._reverb_at is not None:
                src = (clean, strides[0], noisy, strides[1])
                (clean, noisy), other = other, (clean, noisy)
                strides = [clean.stride(0), noisy.stride(0)]
                aug.launch_reverb(*src, nb, length, slot.band_table(self._feeder._reverb_at, aug.reverb_ints(nb)),
                                  self._feeder._bank, slot.reverb_workspace, clean, strides[0], noisy, strides[1])
            if self.draws is not None and self._feeder._band_at is not None:
                src = (clean, strides[0], noisy, strides[1])
                (clean, noisy), other = other, (clean, noisy)
                strides = [clean.stride(0), noisy.stride(0)]
                aug.launch_band(*src, nb, length, slot.band_table(self._feeder._band_at, aug.band_ints(nb)),
                                slot.band_workspace, clean, strides[0], noisy, strides[1])
            if self.draws is not None:
                k = self._feeder._aug_k
                aug.launch(clean, strides[0], noisy, strides[1], nb, self.shape[2], length,
                           slot.aug_table(aug.table_ints(nb, k)), k, slot.workspace, out_clean, out_strides[0], out_noisy,
                           out_strides[1])
            done = torch.cuda.Event()
            done.record(stream)
            slot.released.append(done)       # the next upload into this block waits for it (on the device)
        return out_clean, out_noisy

    def mix_stats(self):
        """A mixing feeder's batch: the (B, 8) float32 stats of its rows on the feeder's device (training/mix.py: a, g, the
        active levels, the peak, the active shares, the guard's flag), as the last ``into`` of this batch left them, for
        logging.  Nothing is waited for: on a GPU the tensor is valid in stream order behind that ``into``."""
        if self.mix is None:
            raise RuntimeError("PcmBatch.mix_stats: the feeder does not mix (BatchFeeder(..., mix=Mix(...)))")
        return self._live_slot().mix_stats[:self.shape[0]]

    def tensors(self):
        """(clean, noisy): two fresh (B, 1, L) float32 tensors, assembled by ``into``."""
        self._live_slot()
        clean = torch.empty(self.shape, dtype=torch.float32, device=self.device)
        noisy = torch.empty(self.shape, dtype=torch.float32, device=self.device)
        return self.into(clean, noisy)


class BatchFeeder:
    """``for batch in BatchFeeder(dataset, 16, "cuda:0"): loss, gn = step(batch)`` -- one pass of the loop is one epoch,
    the next ``for`` continues with the next epoch; the workers prefetch across the boundary.

    dataset: anything with ``__len__``, ``pair_length(n)``, ``read_pcm(n, start, count)``, (for the batch's ``fileids``)
      ``files`` and (for a rated feeder) ``pair_rate(n)``: util/dataset.CleanNoisyPairDataset.  With ``mix``: anything
      with ``__len__``, ``n_noise``, ``speech_length(i)``, ``noise_length(j)``, ``read_speech`` / ``read_noise(i, start,
      count, out)`` and ``speech_files``: util/dataset.SpeechNoiseDataset.
    crop_length: samples per clip of the batch, at the model's rate; default ``int(dataset.crop_length_sec * 16000)``.  A
      longer clip gives a random window, a shorter one is uploaded whole and repeated on the device.
    sample_rate: None -- no header rate is read, every file is taken as it is; or the model's rate (16000): every pair's
      rate is read once here and a pair at another rate is converted on the device while the batch is assembled.  A
      rate the resampler does not take (util/resample.py: factors above 1024, a tile span beyond the kernels' LDS) is a
      ValueError naming the file, as is, on the CPU, any rate but the model's.
    depth: staging slots, and the number of further ``next()`` calls a batch stays usable for.
    workers: reader threads (at most; never more than the rows in flight).  Reading is I/O and memcpy, which release the
      interpreter lock; a handful saturates the page cache, and the count is deliberately not taken from the machine's
      CPU count.
    rank / world: this process takes ``perm[rank::world]`` of every epoch's permutation, truncated to the common count.
    timeout_s: the longest ``next()`` waits for the readers or an upload before it raises TimeoutError.
    augment: None, or a ``training.augment.Augment``: every batch is augmented on its way into the step's inputs
      (csrc/augment.hip).  The draws of batch k of epoch e come from
      ``numpy.random.Generator(PCG64([seed, e, rank, k, 0x417567]))`` -- never from the plan's generator -- and are the
      batch's ``draws``; they travel in the slot's tail, in the same one upload.  With ``shift = S > 0`` the plan draws
      crops of ``crop_length + S`` (model-rate) samples; otherwise the plan is the one without augmentation.  A config
      with every transform off is taken as None.  With ``band_mask`` the band records ride behind the draw table and
      every batch takes one more launch pair (csrc/bandmask.hip) between the assembling kernel and the augmenting one.
      With ``reverb`` the room records ride behind those, the bank of responses is uploaded here, once, and every batch
      takes three more launches (csrc/reverb.hip) right behind the assembling kernel; every device block owns the
      stage's workspace (48 MB at the E8 batch).
    mix: None, or a ``training.mix.Mix`` with a ``util.dataset.SpeechNoiseDataset`` (the one without the other is a
      ValueError, as is ``mix`` with ``sample_rate``): the plan orders and crops the speech files, ``noise_plan(epoch, k)``
      lays out every row's noise, the ``MixDraws`` of batch k of epoch e come from
      ``PCG64([seed, e, rank, k, 0x4D6978])`` (``mix_draws``) and travel in the slot's tail as the records of
      cum_mix_pairs, which takes the assembling kernel's place (csrc/mix.hip, three launches).  ``workers`` may be 0:
      ``next()`` then reads the batch itself."""

    def __init__(self, dataset, batch_size, device, crop_length=None, shuffle=True, seed=0, drop_last=True, depth=2,
                 workers=4, rank=0, world=1, timeout_s=60, sample_rate=None, augment=None, mix=None):
        self.dataset = dataset
        unpaired = hasattr(dataset, "read_speech")
        if mix is not None and not isinstance(mix, mx.Mix):
            raise ValueError("BatchFeeder: mix must be a training.mix.Mix or None")
        if unpaired and mix is None:
            raise ValueError("BatchFeeder: a dataset of separate speech and noise needs mix=Mix(...)")
        if mix is not None and not unpaired:
            raise ValueError("BatchFeeder: mix= takes a SpeechNoiseDataset; a dataset of pairs is already mixed")
        if mix is not None and sample_rate is not None:
            raise ValueError("BatchFeeder: mix= and sample_rate= do not combine (a SpeechNoiseDataset is at one rate)")
        self.mix = mix
        self._length = dataset.speech_length if unpaired else dataset.pair_length        # samples of clip n
        self.batch_size = int(batch_size)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if crop_length is None:
            crop_length = int(getattr(dataset, "crop_length_sec", 0) * SAMPLE_RATE)
        self.crop_length = int(crop_length)
        if augment is not None and not isinstance(augment, aug.Augment):
            raise ValueError("BatchFeeder: augment must be a training.augment.Augment or None")
        self.augment = augment if augment is not None and augment.active else None
        self.shuffle, self.seed, self.drop_last = bool(shuffle), int(seed), bool(drop_last)
        self.depth, self.workers = int(depth), int(workers)
        self.rank, self.world = int(rank), int(world)
        self.timeout_s = float(timeout_s)
        if self.batch_size < 1 or self.crop_length < 1 or self.depth < 1 or self.workers < (0 if mix is not None else 1):
            raise ValueError("BatchFeeder: batch_size, crop_length, depth and workers must be at least 1")
        if not 0 <= self.rank < self.world:
            raise ValueError(f"BatchFeeder: rank {self.rank} outside world {self.world}")
        self.per_rank = len(dataset) // self.world
        if len(self) < 1:
            raise ValueError(f"BatchFeeder: {len(dataset)} pairs over {self.world} rank(s) give no batch of "
                             f"{self.batch_size}")
        self._read_into = unpaired or "out" in inspect.signature(dataset.read_pcm).parameters

        gpu = self.device.type == "cuda"
        if gpu:
            hip.lib()                                   # a missing library is an error now, not at the first batch
        self.sample_rate = None if sample_rate is None else rs._rate(sample_rate, "sample_rate")
        need = self._plan_length
        if self.sample_rate is not None:
            need = self._read_rates(gpu)
        self.pitch = _round_up(need, 8)
        tail = mx.REC_INTS if self.mix is not None else 1 if self.sample_rate is None else rs.REC_INTS
        self._aug_k = self.augment.max_taps if self.augment is not None else 0       # tap columns of the draw table
        table = aug.table_ints(self.batch_size, self._aug_k) if self.augment is not None else 0
        self._band_at = None                    # with a band mask: where its records start, in int32 behind the draw table
        if self.augment is not None and self.augment.band_mask is not None:
            self._band_at, table = table, table + aug.band_ints(self.batch_size)
        self._reverb_at = self._bank = None     # with a reverb: where its records start, likewise; the bank on the device
        if self.augment is not None and self.augment.reverb is not None:
            self._reverb_at, table = table, table + aug.reverb_ints(self.batch_size)
            if gpu:
                self._bank = self.augment.reverb.bank(self.device)
        self._stage = [_Slot(self.batch_size, self.pitch, "cpu", gpu, tail, table) for _ in range(self.depth)]
        self._stage_np = [s.flat.numpy() for s in self._stage]
        # one device block more than staging slots: batch k + 1 is uploaded while k and the depth - 1 before it are live
        self._dev = [_Slot(self.batch_size, self.pitch, self.device, False, tail, table) for _ in range(self.depth + 1)]
        if gpu and self.augment is not None:
            for block in self._dev:        # rows on the 16-byte grid, as the assembling kernels' wide stores want them
                block.scratch = tuple(torch.empty(self.batch_size, _round_up(self._plan_length, 4), dtype=torch.float32,
                                                  device=self.device)[:, :self._plan_length] for _ in range(2))
                if self.augment.snr_db is not None:
                    block.workspace = aug.workspace_for(self.batch_size, self.crop_length, self.device)
                if self._band_at is not None or self._reverb_at is not None:
                    block.band_scratch = tuple(torch.empty(self.batch_size, t.stride(0), dtype=torch.float32,
                                                           device=self.device)[:, :self._plan_length] for t in block.scratch)
                if self._band_at is not None:
                    block.band_workspace = aug.band_workspace_for(self.batch_size, self.device)
                if self._reverb_at is not None:
                    block.reverb_workspace = aug.reverb_workspace_for(self.batch_size, self._plan_length, self.device)
        if self.mix is not None:
            for block in self._dev:
                block.mix_stats = torch.zeros(self.batch_size, mx.STATS, dtype=torch.float32, device=self.device)
                if gpu:
                    block.mix_workspace = mx.workspace_for(self.batch_size, self._plan_length, self.device)
        self._stream = torch.cuda.Stream(self.device) if gpu else None

        self._cv = threading.Condition()
        self._closed = False
        self._failure = None           # an error outside any one batch (the plan)
        self._cursor = (0, 0, 0)       # next row to hand to a worker: (epoch, batch within the epoch, row)
        self._plan_cache = {}
        self._pending = {}             # seq -> _Pending, from the first row handed out until next() returns the batch
        self._next_seq = 0             # seq of the batch the cursor is in
        self._returned = 0             # batches next() has handed out
        self._uploaded = 0             # batches whose upload has been issued
        self._epoch_left = len(self)   # batches left in the epoch the consumer is in
        self.epoch = 0                 # the epoch the next batch belongs to
        self.wait_read_s = self.wait_upload_s = 0.0       # what next() spent waiting for the readers / for an upload
        self.uploads_late = 0          # uploads issued by the next() that returns the batch, not one call ahead
        self._threads = [threading.Thread(target=self._work, name=f"BatchFeeder-{i}", daemon=True)
                         for i in range(min(self.workers, self.depth * self.batch_size))]
        for t in self._threads:
            t.start()

    @property
    def _plan_length(self):
        """What the plan crops and the assembling kernel writes: the batch's length plus the room the shift moves in."""
        augment = getattr(self, "augment", None)
        return self.crop_length + (augment.shift if augment is not None else 0)

    # ------------------------------------------------------------------ rates
    def _read_rates(self, gpu):
        """Every pair's rate and the plan table (``_rs``; ``_rs_ids``: rate -> plan id, -1 the model's) of those that
        differ from the model's.  Returns the longest source window a crop can read, in samples."""
        files = getattr(self.dataset, "files", None)
        self._rates = [int(self.dataset.pair_rate(i)) for i in range(len(self.dataset))]
        self._rs, self._rs_ids = rs.PlanTable(self.device), {self.sample_rate: -1}
        need = self._plan_length                        # a pair at the model rate: the crop itself
        for i, rate in enumerate(self._rates):
            if rate in self._rs_ids:
                continue
            name = " / ".join(files[i]) if files is not None else f"pair {i}"
            if not gpu:
                raise ValueError(f"BatchFeeder: {name} is at {rate} Hz, not the model's {self.sample_rate}; converting "
                                 "needs the GPU (there is no CPU resampler)")
            try:
                p = rs.plan(rate, self.sample_rate)
                rs.check_fits(p)
            except ValueError as exc:
                raise ValueError(f"BatchFeeder: {name} is at {rate} Hz: {exc}") from exc
            self._rs_ids[rate] = self._rs.add(p)
            need = max(need, rs.window_bound(self._plan_length, p.up, p.down, p.K))
        return need

    def _factors(self, rate):
        """up, down, H, K of ``rate`` -> the model's rate (1, 1, 0, 1 for the model's rate itself: y[m] = x[m])."""
        k = self._rs_ids[rate]
        up, down, H, K, _ = self._rs.plans[k] if k >= 0 else (1, 1, 0, 1, None)
        return up, down, H, K

    def _records(self, entries, windows):
        """The (nb, 16) int32 record table of one batch (include/cleanumamba_hip.h: cum_pcm_batch_resample_f32)."""
        recs = torch.zeros(len(entries), rs.REC_INTS, dtype=torch.int32)
        pos = recs.view(torch.int64)
        for r, ((index, start, count), (m0, M, rate)) in enumerate(zip(entries, windows)):
            recs[r, rs.FEED_PLAN], recs[r, rs.FEED_N_SRC], recs[r, rs.FEED_M] = self._rs_ids[rate], count, M
            recs[r, rs.FEED_N] = int(self.dataset.pair_length(index))
            pos[r, rs.REC_IN0 // 2], pos[r, rs.REC_OUT0 // 2] = start, m0
        return recs

    # ------------------------------------------------------------------ plan
    def __len__(self):
        """Batches per epoch (of this rank)."""
        if self.drop_last:
            return self.per_rank // self.batch_size
        return -(-self.per_rank // self.batch_size)

    def plan(self, epoch):
        """[[(index, start, count)] per batch] of ``epoch`` for this rank -- the samples the workers read: a function of
        (seed, epoch, rank, world, the clips' lengths and, in a rated feeder, rates) alone.  The crop start of a clip is
        drawn for every position of the permutation, so a rank's draws do not depend on the other ranks' clip lengths.
        A rated feeder draws the crop in model-rate samples -- a file of M = ceil(N up / down) of them gives outputs
        [m0, m0 + crop_length), m0 = min(int(u (M - crop_length + 1)), M - crop_length), or all M when M <= crop_length
        -- and plans ``resample.crop_window`` of it; at the model rate that is the unrated plan."""
        return self._plan_full(epoch)[0]

    def _plan_full(self, epoch):
        """(the plan, [[(m0, M, rate)] per batch] or None)."""
        n, crop = len(self.dataset), self._plan_length
        rng = np.random.Generator(np.random.PCG64([self.seed, int(epoch)]))
        perm = rng.permutation(n) if self.shuffle else np.arange(n)
        u = rng.random(n)
        entries, windows = [], []
        for pos in range(self.rank, n, self.world)[:self.per_rank]:
            index = int(perm[pos])
            length = int(self._length(index))
            if length < 1:
                raise ValueError(f"pair {index} of the dataset is empty")
            if self.sample_rate is not None:
                rate = self._rates[index]
                up, down, H, K = self._factors(rate)
                M = rs.out_length(length, up, down)
                m0, count = 0, M
                if M > crop:
                    room = M - crop
                    m0, count = min(int(u[pos] * (room + 1)), room), crop
                entries.append((index,) + rs.crop_window(length, up, down, H, K, m0, count))
                windows.append((m0, M, rate))
            elif length <= crop:
                entries.append((index, 0, length))
            else:
                room = length - crop
                entries.append((index, min(int(u[pos] * (room + 1)), room), crop))
        cuts = range(0, len(self) * self.batch_size, self.batch_size)
        return ([entries[i:i + self.batch_size] for i in cuts],
                [windows[i:i + self.batch_size] for i in cuts] if self.sample_rate is not None else None)

    def draws(self, epoch, k, nb=None):
        """The ``AugmentDraws`` of batch ``k`` of ``epoch`` on this rank (None without augmentation): a function of
        (seed, epoch, rank, k) and the config alone, whatever the workers do and wherever a run is resumed."""
        if self.augment is None:
            return None
        rng = np.random.Generator(np.random.PCG64([self.seed, int(epoch), self.rank, int(k), 0x417567]))
        return self.augment.draw(rng, self.batch_size if nb is None else nb, self.crop_length)

    def mix_draws(self, epoch, k, nb=None):
        """The ``MixDraws`` of batch ``k`` of ``epoch`` on this rank (None without ``mix``): a function of (seed, epoch,
        rank, k) and the config alone."""
        if self.mix is None:
            return None
        rng = np.random.Generator(np.random.PCG64([self.seed, int(epoch), self.rank, int(k), 0x4D6978]))
        return self.mix.draw(rng, self.batch_size if nb is None else nb)

    def noise_plan(self, epoch, k, nb=None):
        """[[(noise file, start, count, position in the row)] per row] of batch ``k`` of ``epoch`` on this rank (None without
        ``mix``) -- the noise samples the workers read and where they put them: a function of (seed, epoch, rank, k, the
        row, the noise files' lengths, the config) alone.  Row r draws from ``PCG64([seed, epoch, rank, k, r, 0x4E6F69])``:
        a piece is a uniformly drawn file from a uniformly drawn start to its end, ``mix.gap`` zeros follow it, and pieces
        repeat until the row's ``crop_length`` (+ shift) samples are full; the last piece is cut, and what ``max_pieces``
        pieces leave open stays zero."""
        if self.mix is None:
            return None
        rows, need = [], self._plan_length
        for r in range(self.batch_size if nb is None else nb):
            rng = np.random.Generator(np.random.PCG64([self.seed, int(epoch), self.rank, int(k), r, 0x4E6F69]))
            pieces, pos = [], 0
            while pos < need and len(pieces) < self.mix.max_pieces:
                j = int(rng.integers(0, self.dataset.n_noise))
                length = int(self.dataset.noise_length(j))
                start = int(rng.integers(0, length))
                count = min(length - start, need - pos)
                pieces.append((j, start, count, pos))
                pos += count + self.mix.gap
            rows.append(pieces)
        return rows

    # ------------------------------------------------------------------ workers
    def _take_row(self):
        """Under the lock: the next (pending batch, row) whose staging slot is free, or None."""
        if self._failure is not None:
            return None
        epoch, b, row = self._cursor
        if self._next_seq >= self._returned + self.depth:       # the slot still holds a batch next() has not handed out
            return None
        plan = self._plan_cache.get(epoch)
        if plan is None:
            try:
                plan = self._plan_full(epoch)
            except Exception as exc:      # noqa: BLE001 - surfaces in the consumer's next()
                self._failure = exc
                self._cv.notify_all()
                return None
            self._plan_cache = {epoch: plan}
        plan, windows = plan
        pend = self._pending.get(self._next_seq)
        if pend is None:
            try:
                pend = _Pending(self._next_seq, epoch, plan[b])
                if windows is not None:
                    pend.windows, pend.records = windows[b], self._records(plan[b], windows[b])
                if self.mix is not None:
                    pend.mix, pend.noise = self.mix_draws(epoch, b, len(plan[b])), self.noise_plan(epoch, b, len(plan[b]))
                    pend.mix_table = torch.from_numpy(pend.mix.pack([count for _, _, count in plan[b]])).view(-1, mx.REC_INTS)
                if self.augment is not None:
                    pend.draws = self.draws(epoch, b, len(plan[b]))
                    pend.table = torch.from_numpy(pend.draws.pack(self._aug_k))
                    if self._band_at is not None:
                        pend.band = torch.from_numpy(pend.draws.pack_band())
                    if self._reverb_at is not None:
                        pend.rooms = torch.from_numpy(pend.draws.pack_reverb())
            except Exception as exc:      # noqa: BLE001 - surfaces in the consumer's next()
                self._failure = exc
                self._cv.notify_all()
                return None
            self._pending[self._next_seq] = pend
        taken, row = row, row + 1
        if row == len(plan[b]):
            row, b, self._next_seq = 0, b + 1, self._next_seq + 1
            if b == len(plan):
                b, epoch = 0, epoch + 1
        self._cursor = (epoch, b, row)
        return pend, taken

    def _work(self):
        while True:
            with self._cv:
                while True:
                    if self._closed:
                        return
                    job = self._take_row()
                    if job is not None:
                        break
                    self._cv.wait(0.5)
            self._read_row(*job)

    def _read_row(self, pend, r):
        """Read row ``r`` of a pending batch into its staging slot and count it off."""
        index, start, count = pend.entries[r]
        error = None
        try:
            nb = len(pend.entries)
            k = pend.seq % self.depth
            flat = self._stage_np[k]
            rows = flat[:2 * nb * self.pitch].reshape(2, nb, self.pitch)
            if self.mix is not None:
                self.dataset.read_speech(index, start, count, out=rows[0, r])
                row, pos = rows[1, r], 0
                for j, at_file, n, at in pend.noise[r]:          # the pieces, zeros between and behind them
                    row[pos:at] = 0
                    self.dataset.read_noise(j, at_file, n, out=row[at:at + n])
                    pos = at + n
                row[pos:self._plan_length] = 0
            elif self._read_into:
                self.dataset.read_pcm(index, start, count, out=(rows[0, r], rows[1, r]))
            else:
                pair = self.dataset.read_pcm(index, start, count)
                for dst, src in zip((rows[0, r], rows[1, r]), pair):
                    src = np.asarray(src)
                    if src.dtype != np.int16 or src.shape != (count,):
                        raise ValueError(f"read_pcm returned {src.dtype} {src.shape}, not int16 ({count},)")
                    dst[:count] = src
            if pend.records is None and pend.mix is None:    # (a rated or mixing batch's tail is its records: _upload)
                flat[2 * self.batch_size * self.pitch:].view(np.int32)[r] = count
        except Exception as exc:      # noqa: BLE001 - surfaces in the consumer's next() with the file's name
            files = getattr(self.dataset, "files", None)
            name = " / ".join(files[index]) if files is not None else f"pair {index}"
            if self.mix is not None:
                name = f"{self.dataset.speech_files[index]} (or the noise of its row)"
            error = RuntimeError(f"BatchFeeder: reading {name} failed: {exc!r}")
            error.__cause__ = exc
        with self._cv:
            if error is not None and pend.error is None:
                pend.error = error
            pend.todo -= 1
            if pend.todo == 0 or error is not None:
                self._cv.notify_all()

    # ------------------------------------------------------------------ consumer
    def _upload(self, pend):
        """Issue the upload of a fully staged batch into its device block (consumer's thread)."""
        stage, dev = self._stage[pend.seq % self.depth], self._dev[pend.seq % (self.depth + 1)]
        if pend.records is not None:
            stage.records()[:len(pend.entries)] = pend.records
        if pend.mix_table is not None:
            stage.mix_records()[:len(pend.entries)] = pend.mix_table
        if pend.table is not None:
            stage.aug_table(pend.table.numel()).copy_(pend.table)
        if pend.band is not None:
            stage.band_table(self._band_at, pend.band.numel()).copy_(pend.band)
        if pend.rooms is not None:
            stage.band_table(self._reverb_at, pend.rooms.numel()).copy_(pend.rooms)
        if self._stream is None:
            dev.flat.copy_(stage.flat)
        else:
            # The kernels that read the block's last batch (depth + 1 batches ago) must be done.  The HOST waits for them,
            # bounded, and the copy is then issued with no dependency: chaining the copy behind their events on the
            # device instead (stream.wait_event) cost the replayed E8 step one upload's duration, 0.2 ms in 19.7, although
            # every upload ended three steps before its batch was used (profiles/feeder_bench.json,
            # feeder_bench_device_gate.json).  A loop that synchronises every step never waits here; one that never
            # does is kept from running more than depth + 1 steps ahead of the device.
            t0, deadline = time.monotonic(), time.monotonic() + self.timeout_s
            for ev in dev.released:
                while not ev.query():
                    if time.monotonic() > deadline:
                        raise TimeoutError(f"BatchFeeder: a device block was not released within {self.timeout_s:g} s")
                    time.sleep(1e-3)
            self.wait_upload_s += time.monotonic() - t0
            with torch.cuda.stream(self._stream):
                dev.flat.copy_(stage.flat, non_blocking=True)
                dev.uploaded = torch.cuda.Event(enable_timing=True)      # (timed: tools/bench_feeder.py places it)
                dev.uploaded.record(self._stream)
        dev.released = []
        dev.seq = pend.seq
        self._uploaded = pend.seq + 1

    def _staged(self, seq):
        pend = self._pending.get(seq)
        return pend if pend is not None and pend.todo == 0 and pend.error is None else None

    def next(self):
        """The next batch of the current epoch; StopIteration once at the end of an epoch, after which the next call
        starts the following one."""
        if self._closed:
            raise RuntimeError("BatchFeeder is closed")
        if self._epoch_left == 0:
            self._epoch_left = len(self)
            self.epoch += 1
            raise StopIteration
        seq, deadline = self._returned, time.monotonic() + self.timeout_s
        t0 = time.monotonic()
        while not self._threads:                        # workers = 0: this thread reads, up to the end of batch seq
            with self._cv:
                job = self._take_row() if self._next_seq <= seq else None
            if job is None:
                break
            self._read_row(*job)
        with self._cv:
            while True:
                pend = self._pending.get(seq)
                if pend is not None and pend.error is not None:
                    raise pend.error
                if self._failure is not None:
                    raise RuntimeError(f"BatchFeeder: planning an epoch failed: {self._failure!r}") from self._failure
                if pend is not None and pend.todo == 0:
                    break
                left = deadline - time.monotonic()
                if left <= 0:
                    raise TimeoutError(f"BatchFeeder: batch {seq} was not read within {self.timeout_s:g} s")
                self._cv.wait(min(left, 0.5))
        t1 = time.monotonic()
        self.wait_read_s += t1 - t0
        if self._uploaded <= seq:                       # not prefetched (the first batch, or the readers were behind)
            self._upload(pend)
            self.uploads_late += 1
        dev = self._dev[seq % (self.depth + 1)]
        # The staging slot goes back to the readers once its upload has left it: a bounded host wait, normally over at
        # once because the upload was issued one next() earlier.  Polled sparsely: a query is a call into the runtime.
        if dev.uploaded is not None:
            while not dev.uploaded.query():
                if time.monotonic() > deadline:
                    raise TimeoutError(f"BatchFeeder: the upload of batch {seq} did not finish within "
                                       f"{self.timeout_s:g} s")
                time.sleep(1e-3)
        self.wait_upload_s += time.monotonic() - t1
        batch = PcmBatch(self, seq, pend.epoch, pend.entries, dev, pend.windows, pend.records, pend.draws, pend.mix,
                         pend.noise)
        with self._cv:
            del self._pending[seq]
            self._returned = seq + 1                    # frees staging slot seq % depth; batch seq - depth goes stale
            ahead = self._staged(seq + 1)
            self._cv.notify_all()
        if ahead is not None:                           # its device block held batch seq - depth, stale as of now
            self._upload(ahead)
        self._epoch_left -= 1
        return batch

    __next__ = next

    def __iter__(self):
        return self

    @property
    def idle_seconds(self):
        """Host time next() spent waiting, for the readers and for uploads."""
        return self.wait_read_s + self.wait_upload_s

    def close(self):
        """Stop and join the reader threads (a thread stuck inside the dataset is abandoned after a bounded wait; it
        is a daemon)."""
        with self._cv:
            self._closed = True
            self._cv.notify_all()
        for t in self._threads:
            t.join(timeout=max(1.0, min(self.timeout_s, 5.0)))
        self._threads = [t for t in self._threads if t.is_alive()]
        if self._stream is not None:
            self._stream.synchronize()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
