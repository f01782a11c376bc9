"""CleanUMamba module for MI355X -- drop-in for src/network/CleanUMamba.py:30-550.

Same constructor keywords and defaults (:33-54), same sub-module tree and therefore
the same state-dict keys and shapes, same public methods
(forward, feed, flush, load_pruned_state_dict, valid_length, pad_signal,
total_stride, frame_length, time_per_frame, reset_time_per_frame,
allocate_inference_cache).  The arithmetic of the Mamba bottleneck runs in the HIP
kernels of csrc/ (selective scan, causal depthwise conv, single-step update).

Differences from the reference, on purpose:
  * ``forward`` does not mutate its argument (the reference divides the caller's
    tensor by its std in place, :262); the returned value is identical.
  * ``feed``/``flush`` implement the intended streaming semantics (stream output ==
    ``forward`` output with normalize_input=False).  The reference's own feed()
    raises on every shipped model (skip order at :474) and its flush() drops the
    decoder overlap of the tail (:364); see SURVEY.md fact 9.
  * ablation variants (LSTM, MambaS4, residual_projection, rms_norm, fused_add_norm)
    are out of scope and raise NotImplementedError.  ``mamba_v2=True`` (the Mamba2
    bottleneck) is supported: mamba_ssm/modules/mamba2.py, csrc/ssd.hip.
"""
import os
import weakref
from functools import partial

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..mamba_ssm.models.mixer_seq_simple import _init_weights, create_block
from ..mamba_ssm.ops import layernorm as _ln
from ..util.util import weight_scaling_init
from .. import hip
from . import convstack as cs
from . import streaming
from .layers import Activation


class CleanUMamba(nn.Module):
    """CleanUNet encoder/decoder with a Mamba bottleneck."""

    def __init__(self, channels_input=1, channels_output=1, channels_H=64, max_H=768, encoder_n_layers=8,
                 kernel_size=4, stride=2, encoder_groups=1, bypass_channels=0, glu_activation="Sigmoid",
                 tsfm_n_layers=3, tsfm_n_head=8, tsfm_d_model=512, tsfm_d_inner=2048, fused_add_norm=False,
                 use_fast_path=False, rms_norm=False, mamba_s4=False, LSTM=False, mamba_v2=False,
                 residual_projection=False, norm_epsilon: float = 1e-5, normalize_input=True, device=None,
                 dtype=None):
        super().__init__()
        assert glu_activation in ["Sigmoid", "ReLU", "SiLU", "GELU"], f"glu_activation={glu_activation} not supported"
        for flag, name in ((mamba_s4, "mamba_s4"), (LSTM, "LSTM"), (residual_projection, "residual_projection"), (rms_norm, "rms_norm"),
                           (fused_add_norm, "fused_add_norm")):
            if flag:
                raise NotImplementedError(f"{name}=True is an ablation variant outside the MI355X hot path")
        factory_kwargs = {"device": device, "dtype": dtype}

        self.channels_input = channels_input
        self.channels_output = channels_output
        self.channels_H = channels_H
        self.max_H = max_H
        self.encoder_n_layers = encoder_n_layers
        self.kernel_size = kernel_size
        self.stride = stride
        self.tsfm_n_layers = tsfm_n_layers
        self.tsfm_n_head = tsfm_n_head
        self.tsfm_d_model = tsfm_d_model
        self.tsfm_d_inner = tsfm_d_inner
        self.residual_projection = residual_projection
        self.normalize_input = normalize_input
        self.dtype = dtype

        self.encoder = nn.ModuleList()
        self.decoder = nn.ModuleList()
        for i in range(encoder_n_layers):
            ec_groups = encoder_groups[i] if isinstance(encoder_groups, list) else encoder_groups
            bp_channels = bypass_channels[i] if isinstance(bypass_channels, list) else bypass_channels
            self.encoder.append(nn.Sequential(
                nn.Conv1d(channels_input, channels_H, kernel_size, stride, groups=ec_groups if i > 0 else 1,
                          **factory_kwargs),
                nn.ReLU(),
                nn.Conv1d(channels_H, bp_channels + (channels_H - bp_channels) * 2, 1, **factory_kwargs),
                Activation(glu_activation, bp_channels)))
            channels_input = channels_H
            decoder_i = nn.Sequential(
                nn.Conv1d(channels_H, bp_channels + (channels_H - bp_channels) * 2, 1, **factory_kwargs),
                Activation(glu_activation, bp_channels),
                nn.ConvTranspose1d(channels_H, channels_output, kernel_size, stride, **factory_kwargs))
            if i > 0:  # ReLU on all but the outermost decoder layer
                decoder_i.append(nn.ReLU())
            self.decoder.insert(0, decoder_i)
            channels_output = channels_H
            channels_H = min(channels_H * 2, max_H)

        self.tsfm_conv1 = nn.Conv1d(channels_output, tsfm_d_model, kernel_size=1, **factory_kwargs)
        ssm_cfg = {"d_state": tsfm_d_model // tsfm_n_head, "d_conv": 4, "expand": tsfm_d_inner // tsfm_d_model}
        if mamba_v2:        # as the reference builds it (src/network/CleanUMamba.py:141-151)
            ssm_cfg["layer"] = "Mamba2"
            ssm_cfg["headdim"] = tsfm_d_model // tsfm_n_head
            ssm_cfg["use_mem_eff_path"] = False
        else:
            ssm_cfg["use_fast_path"] = use_fast_path
        self.rms_norm = rms_norm
        self.residual_in_fp32 = True
        self.fused_add_norm = fused_add_norm
        self.LSTM = LSTM
        self.tsfm_Mamba_layers = nn.ModuleList([
            create_block(tsfm_d_model, ssm_cfg=ssm_cfg, norm_epsilon=norm_epsilon, rms_norm=rms_norm,
                         residual_in_fp32=self.residual_in_fp32, fused_add_norm=self.fused_add_norm, layer_idx=i,
                         **factory_kwargs)
            for i in range(tsfm_n_layers)])
        self.norm_f = nn.LayerNorm(tsfm_d_model, eps=norm_epsilon, **factory_kwargs)
        self.tsfm_conv2 = nn.Conv1d(tsfm_d_model, channels_output, kernel_size=1, **factory_kwargs)

        # initialisation order of the reference: weight scaling on every conv (the Mamba depthwise conv
        # included), then mamba's _init_weights on every sub-module (:197-206)
        for layer in self.modules():
            if isinstance(layer, (nn.Conv1d, nn.ConvTranspose1d)):
                weight_scaling_init(layer)
        self.apply(partial(_init_weights, n_layer=tsfm_n_layers))

        # True: encoder/decoder run on the fused HIP GEMM kernels (network/convstack.py).  False: the layers
        # are called as torch modules (needed only when forward hooks on the conv modules must fire, as the
        # reference's pruning tools expect); the Mamba bottleneck uses the HIP kernels either way.
        self.use_fused_convs = True
        # True: the encoder and the decoder are one autograd node each (cs.EncoderStack / cs.DecoderStack) whose
        # backward folds the ReLU gate, the GLU backward and the skip-gradient add into GEMM epilogues.  False: one
        # node per layer with separate elementwise kernels (CUM_STACK_BACKWARD=0 selects it for A/B timing).
        self.use_stack_backward = os.environ.get("CUM_STACK_BACKWARD", "1") != "0"
        # True: after the first hop of a stream the (launch-bound, ~100 tiny kernels) hop is captured once in a
        # hipGraph and replayed; stream state lives in static buffers updated in place.
        self.use_hop_graph = True
        # True: streaming hops run on the fused GEMM kernels (streaming.fused_hop); False: torch modules with
        # per-layer encoder caches (streaming.cached_hop, the reference's structure)
        self.use_fused_stream = True
        # True: the fused streaming hop stores activations and runs its GEMMs in bf16 (f32 accumulate; the Mamba
        # steps and all stream state stay f32).  Off by default: the hop then matches ``forward`` to 1e-4.
        self.stream_bf16 = False
        # True: behind a stream's first frame every hop of a call runs in ONE launch (csrc/hop.hip), where it covers the model
        self.use_hop_kernel = True
        # True: after a stream's first frame the fused hop computes only the new rows of every layer; False: whole windows
        self.stream_incremental = True
        # fewest streams for which the fused hop is taken over the cached one
        self.fused_min_streams = 1

        # streaming: timing counters here, everything else in ``stream`` (network/streaming.py)
        self.total_time = 0
        self.cat_time = 0
        self.frames = 0                 # frames denoised since reset_time_per_frame(): only for time_per_frame
        self.frame_length = self.valid_length(1)
        self.stream = streaming.Stream(torch.zeros(self.channels_input, 0, dtype=self.dtype, device=device))

    def __getstate__(self):
        state = self.__dict__.copy()        # (``stream`` leaves out what it cannot carry itself)
        state.pop("_pack_plans", None)      # device-side caches of packed weights are rebuilt on demand
        state.pop("_hop_plan", None)        # packed weights / plan of the one-launch hop
        state.pop("_stream_pools", None)    # (weak references to the stream pools of this model)
        return state

    # ------------------------------------------------------------------ geometry
    def valid_length(self, length):
        """Smallest length >= ``length`` that survives D strided convs and their transposes exactly."""
        D, K, S = self.encoder_n_layers, self.kernel_size, self.stride
        for _ in range(D):
            length = 1 if length < K else 1 + np.ceil((length - K) / S)
        for _ in range(D):
            length = (length - 1) * S + K
        return int(length)

    def pad_signal(self, input):
        return F.pad(input, (0, self.valid_length(input.shape[-1]) - input.shape[-1]))

    @property
    def total_stride(self):
        return self.stride ** self.encoder_n_layers

    # ------------------------------------------------------------------- forward
    @staticmethod
    def _pointwise_linear(conv, x):
        """A 1x1 Conv1d as a matmul over (B*T, C): for the one-column inputs of a streaming hop MIOpen falls back
        to a naive kernel (23 us against 6 us).  Module hooks on ``conv`` do not fire on this route."""
        w = conv.weight.squeeze(-1)
        if x.is_cuda and x.shape[-1] == 1 and x.dtype == torch.float32 and w.dtype == torch.float32 \
                and w.shape[1] <= 1024 and not torch.is_grad_enabled():
            # one-column input: a workgroup per stream with the matrix staged in LDS (csrc/mamba_step.hip)
            xin = x.reshape(x.shape[0], x.shape[1]).contiguous()
            out = torch.empty(x.shape[0], w.shape[0], dtype=torch.float32, device=x.device)
            # named locals: a contiguous() temporary must outlive the launch (ctypes passes bare addresses)
            wc = w.detach().contiguous()
            bc = None if conv.bias is None else conv.bias.detach().contiguous()
            with torch.cuda.device(x.device):
                hip.check(hip.lib().cum_small_linear(x.shape[0], w.shape[0], w.shape[1], hip.ptr(xin), w.shape[1],
                                                     hip.ptr(wc), hip.ptr(bc), hip.ptr(out), w.shape[0],
                                                     hip.stream_ptr()))
            return out.unsqueeze(-1)
        return F.linear(x.transpose(1, 2), w, conv.bias).transpose(1, 2)

    def _bottleneck(self, x, inference_params=None, pointwise_as_linear=False):
        """tsfm_conv1 -> Mamba blocks -> add + norm_f -> tsfm_conv2.  x: (B, C, T)."""
        if pointwise_as_linear:
            x = self._pointwise_linear(self.tsfm_conv1, x)
        else:
            x = self.tsfm_conv1(x)
        hidden_states = x.permute(0, 2, 1)
        residual = None
        for layer in self.tsfm_Mamba_layers:
            hidden_states, residual = layer(hidden_states, residual, inference_params=inference_params)
        if _ln.supported(hidden_states, self.norm_f):
            hidden_states, _ = _ln.add_layer_norm(hidden_states, residual, self.norm_f)
        else:
            residual = (hidden_states + residual) if residual is not None else hidden_states
            hidden_states = self.norm_f(residual.to(dtype=self.norm_f.weight.dtype))
        tsfm_out = hidden_states.permute(0, 2, 1)
        if pointwise_as_linear:
            return self._pointwise_linear(self.tsfm_conv2, tsfm_out), tsfm_out
        return self.tsfm_conv2(tsfm_out), tsfm_out

    def forward(self, noisy_audio, return_skip_connections=False):
        if noisy_audio.dim() == 2:
            noisy_audio = noisy_audio.unsqueeze(1)
        B, C, L = noisy_audio.shape
        assert C == 1
        if B == 0 and not return_skip_connections:          # an empty batch: the torch modules return an empty result too
            return noisy_audio.new_zeros(0, self.channels_output, L)
        fused = getattr(self, "use_fused_convs", True) and noisy_audio.is_cuda
        if fused and not cs.supported(self):
            raise NotImplementedError("fused conv stack covers kernel 4 / stride 2 / ungrouped / sigmoid-GLU "
                                      "layers; set model.use_fused_convs = False for other variants")
        if fused and noisy_audio.dtype == torch.float32 and not noisy_audio.requires_grad and self.channels_output == 1:
            # waveform ends on the library's own kernels (csrc/loss.hip): per-clip std, `noisy / std` + padding written
            # straight into the first conv's row buffer, `x[:, :, :L] * std` read straight from the last one's
            std = cs.clip_std(noisy_audio, 1e-3) if self.normalize_input else None
            T0 = self.valid_length(L)
            dt = self._fused_dtype()
            buf = cs.frame_input(noisy_audio, std, T0, dt)
            if torch.is_grad_enabled():
                buf, geo, skip_connections, tsfm_out = self._forward_fused(buf, B, T0, dt)
            else:
                with cs.small_m_gemms():     # inference on short inputs: few-tile GEMMs may split K over the waves
                    buf, geo, skip_connections, tsfm_out = self._forward_fused(buf, B, T0, dt)
            # (without input normalisation the reference returns the padded length: src/network/CleanUMamba.py:318-319)
            x = cs.Unframe.apply(buf, std, geo, L if self.normalize_input else T0)
            if return_skip_connections:
                skip_connections.append(tsfm_out)
                return x, skip_connections
            return x
        if self.normalize_input:
            std = noisy_audio.std(dim=2, keepdim=True) + 1e-3
            noisy_audio = noisy_audio / std
        x = self.pad_signal(noisy_audio)

        if fused:
            dt = self._fused_dtype()
            geo = cs.Geo(B, x.shape[-1], 1)
            buf = cs.to_rows(x, geo, dt)
            if torch.is_grad_enabled():
                buf, geo, skip_connections, tsfm_out = self._forward_fused(buf, B, x.shape[-1], dt)
            else:
                with cs.small_m_gemms():
                    buf, geo, skip_connections, tsfm_out = self._forward_fused(buf, B, x.shape[-1], dt)
            x = cs.from_rows(buf, geo).float()
        else:
            skip_connections = []
            for downsampling_block in self.encoder:
                x = downsampling_block(x)
                skip_connections.append(x)
            skip_connections = skip_connections[::-1]
            x, tsfm_out = self._bottleneck(x)
            for i, upsampling_block in enumerate(self.decoder):
                skip_i = skip_connections[i]
                x = x + skip_i[:, :, :x.shape[-1]]
                x = upsampling_block(x)

        if self.normalize_input:
            x = x[:, :, :L] * std
        if return_skip_connections:
            skip_connections.append(tsfm_out)
            return x, skip_connections
        return x

    def _fused_dtype(self):
        """Element type of every activation and GEMM operand of the fused path: the autocast dtype -- float16 (torch's
        default, what the reference trains with: src/training/train.py:278-280) or bfloat16 -- else float32;
        accumulation is f32 in every mode."""
        if torch.is_autocast_enabled("cuda"):
            dt = torch.get_autocast_dtype("cuda")
            if dt not in hip.HALF_TYPES:
                raise RuntimeError(f"autocast dtype {dt} is not supported by the fused conv stack")
            return dt
        return torch.float32

    def _forward_fused(self, buf, B, T0, dt, carry=None, ragged=None):
        """Encoder, bottleneck and decoder on channels-last row buffers (network/convstack.py).
        buf: row buffer of the (B, 1, T0 = valid_length) input in element type dt.  Returns (row buffer of the output,
        its Geo, skips deepest first as (B, C, T) views, tsfm_out).
        carry (network/blockdenoise.py, inference only): the input is one window of a longer signal -- its first
        ``carry.context`` bottleneck columns were already seen by the previous window.  The Mamba blocks then run on the
        new columns only, continuing from the states in ``carry.params``, and ``carry.join`` puts the previous window's
        last norm_f outputs back in front for tsfm_conv2 and the decoder.
        ragged (network/ragged.py RaggedTables, inference only): the batch holds clips of different lengths, zero padded
        to T0 -- every decoder layer keeps only the rows of its GLU output that a clip has when it runs alone; the
        encoder, the bottleneck, tsfm_conv2 and every GEMM are the same launches as without it."""
        E = self.encoder_n_layers
        save = torch.is_grad_enabled()
        self._activate_pack_plan(dt)
        geo = cs.Geo(B, T0, 1)
        enc_geos, enc_params = [], []
        for enc in self.encoder:
            T1 = (geo.T - self.kernel_size) // self.stride + 1
            g_mid = cs.Geo(B, T1, enc[0].weight.shape[0])
            if geo.P != 2 * g_mid.P:
                raise RuntimeError("fused conv stack needs an input of valid_length()")
            g_out = cs.Geo(B, T1, enc[2].weight.shape[0] // 2)
            enc_geos.append((geo, g_mid, g_out))
            enc_params += [enc[0].weight, enc[0].bias, enc[2].weight, enc[2].bias]
            geo = g_out
        if getattr(self, "use_stack_backward", True):
            outs = cs.EncoderStack.apply(buf, enc_geos, save, *enc_params)
        else:                              # per-layer autograd nodes (unfused elementwise backward), kept for A/B runs
            outs = []
            for (gi, gm, go), enc in zip(enc_geos, self.encoder):
                y1 = cs.ConvK4S2ReLU.apply(buf, enc[0].weight, enc[0].bias, gi, gm)
                buf = cs.PointwiseGLU.apply(y1, enc[2].weight, enc[2].bias, gm, go, save)
                outs.append(buf)
        cut = self.__dict__.get("_encoder_cut")
        if cut is not None and torch.is_grad_enabled():
            # training/train_step.py, captured multi-rank step: the backward is cut at the encoder's outputs so that the
            # decoder + bottleneck gradients can be exchanged while the encoder's backward runs (a second graph)
            leaves = tuple(o.detach().requires_grad_(True) for o in outs)
            cut.append((tuple(outs), leaves))
            outs = leaves
        skips = [(b, g[2]) for b, g in zip(outs, enc_geos)][::-1]
        buf = outs[-1]

        g_t = cs.Geo(B, geo.T, self.tsfm_conv1.weight.shape[0])
        hbuf = cs.Pointwise.apply(buf, self.tsfm_conv1.weight, self.tsfm_conv1.bias, None, geo, g_t)
        hidden_states = g_t.rows(hbuf)[:, :g_t.T, :g_t.C]
        if carry is not None:
            hidden_states = hidden_states[:, carry.context:]
        residual = None
        for layer in self.tsfm_Mamba_layers:
            hidden_states, residual = layer(hidden_states, residual,
                                            inference_params=None if carry is None else carry.params)
        if _ln.supported(hidden_states, self.norm_f):
            hidden_states, _ = _ln.add_layer_norm(hidden_states, residual, self.norm_f)
        else:
            residual = hidden_states + residual
            hidden_states = self.norm_f(residual.to(dtype=self.norm_f.weight.dtype))
        if carry is not None:
            hidden_states = carry.join(hidden_states)
        tsfm_out = hidden_states.permute(0, 2, 1)
        tbuf = cs.to_rows(tsfm_out, g_t, dt)
        # tsfm_conv2 with the deepest skip added in its epilogue
        buf = cs.Pointwise.apply(tbuf, self.tsfm_conv2.weight, self.tsfm_conv2.bias, skips[0][0], g_t, geo)

        dec_geos, dec_params, dec_skips = [], [], []
        for j, dec in enumerate(self.decoder):
            g_glu = cs.Geo(B, geo.T, dec[0].weight.shape[0] // 2)
            g_out = cs.Geo(B, 2 * geo.T + 2, dec[2].weight.shape[1])
            if j < E - 1:
                skip, g_skip = skips[j + 1]
                assert g_skip.T == g_out.T and g_skip.C == g_out.C
                dec_skips.append(skip)
            dec_geos.append((geo, g_glu, g_out))
            dec_params += [dec[0].weight, dec[0].bias, dec[2].weight, dec[2].bias]
            geo = g_out
        if ragged is not None:
            if save:
                raise RuntimeError("ragged batches are inference only: run them under torch.no_grad()")
            buf = cs.decoder_layers(buf, dec_geos, False, dec_skips + [None] * (E - len(dec_skips)), dec_params,
                                    ragged=ragged)[0][-1]
        elif getattr(self, "use_stack_backward", True):
            buf = cs.DecoderStack.apply(buf, dec_geos, save, len(dec_skips), *dec_skips, *dec_params)
        else:
            for j, ((gi, gg, go), dec) in enumerate(zip(dec_geos, self.decoder)):
                gbuf = cs.PointwiseGLU.apply(buf, dec[0].weight, dec[0].bias, gi, gg, save)
                buf = cs.ConvT4S2.apply(gbuf, dec[2].weight, dec[2].bias, dec_skips[j] if j < E - 1 else None, gg, go,
                                        j < E - 1)
        return buf, geo, [cs.from_rows(b, g) for b, g in skips], tsfm_out

    # --------------------------------------------------------------- long recordings
    def block_denoiser(self, streams, std=None, block_hops=None):
        """A BlockDenoiser (network/blockdenoise.py): ``push(x)`` / ``finish()`` denoise a signal of any length in blocks
        of ``block_hops`` bottleneck columns with the Mamba state carried across -- ``forward``'s result at one block's
        memory.  std: (streams, 1) per-clip std + eps of the WHOLE signal (required when ``normalize_input``)."""
        from .blockdenoise import BlockDenoiser
        return BlockDenoiser(self, streams, std=std, block_hops=block_hops)

    def denoise_long(self, noisy, block_size=160000, block_hops=None, rate=None, model_rate=16000):
        """``forward`` on a (B, L) / (B, 1, L) signal of any length, block by block (network/blockdenoise.py).  Host input
        gives host output, and device memory does not depend on L.  rate: the signal's sample rate if it is not the
        model's -- the signal is converted to ``model_rate``, denoised and converted back as one stream
        (util/resample.py StreamResampler), and comes back (B, 1, L) at its own rate."""
        from .blockdenoise import denoise_long
        return denoise_long(self, noisy, block_size=block_size, block_hops=block_hops, rate=rate, model_rate=model_rate)

    # ------------------------------------------------------------ ragged batches
    def forward_ragged(self, x, lengths, pcm16=None):
        """``forward`` on a batch of clips of DIFFERENT lengths in one pass (network/ragged.py).  x: (B, Lmax) int16 PCM, or
        (B, 1, Lmax) / (B, Lmax) f32, on the GPU, clip b in its first lengths[b] samples; lengths: a host sequence or a
        device i32 tensor.  -> (B, 1, Lmax) f32: clip b's ``forward`` in [b, 0, :lengths[b]], zeros behind.  no_grad only.
        pcm16 = (flat int16 device buffer, device i64[B] sample offsets, mode): clip b is quantised into
        flat[offsets[b] : offsets[b] + lengths[b]] instead (mode 0: * 32767, truncated; 1: * 32768, rounded) -> None."""
        from .ragged import forward_ragged
        return forward_ragged(self, x, lengths, pcm16=pcm16)

    def denoise_batch_pcm16(self, clips, mode=0, max_batch=32, budget_samples=32 * 160000, max_waste=0.25):
        """``denoise_batch`` into ONE flat int16 device buffer (network/ragged.py): -> (flat, offsets, lengths), clip i
        at flat[offsets[i] : offsets[i] + lengths[i]], quantised on the device by ``mode``."""
        from .ragged import denoise_batch_pcm16
        return denoise_batch_pcm16(self, clips, mode=mode, max_batch=max_batch, budget_samples=budget_samples,
                                   max_waste=max_waste)

    def denoise_batch(self, clips, max_batch=32, budget_samples=32 * 160000, max_waste=0.25, rates=None, model_rate=16000):
        """[model(c[None, None])[0, 0, :len(c)] for c in clips] for a list of 1-D clips (int16 PCM or f32, host or device)
        of any lengths, batched by network/ragged.py plan_batches and run by ``forward_ragged``; a clip longer than the
        sample budget goes through ``denoise_long``.  -> list of f32 device tensors, in the order of ``clips``.
        rates: one sample rate for all clips or one per clip; a clip at another rate than ``model_rate`` is converted to
        it, denoised, converted back and cropped to its own length (util/resample.py).  None: every clip is at the
        model's rate."""
        from .ragged import denoise_batch
        return denoise_batch(self, clips, max_batch=max_batch, budget_samples=budget_samples, max_waste=max_waste,
                             rates=rates, model_rate=model_rate)

    @property
    def ragged_dispatch(self):
        """The route every decoder layer took in the last ``forward_ragged``: "gemm+zero_tail", "dech_ragged",
        "dec7_ragged", or the plain name where no clip of the batch is shorter than the batch at that layer."""
        return list(self.__dict__.get("_ragged_routes", ()))

    def _activate_pack_plan(self, dt):
        """One batched re-pack of all conv weights for this forward (and its backward); see cs.PackPlan.  Skipped
        while no parameter has been modified since the last pack (inference loops, streaming hops)."""
        plans = self.__dict__.setdefault("_pack_plans", {})
        plan = plans.get(dt)
        conv_params = [p for m in (self.encoder, self.decoder, self.tsfm_conv1, self.tsfm_conv2) for p in m.parameters()]
        for layer in self.tsfm_Mamba_layers:              # the Mamba projections' GEMM operands ride in the same gather
            mixer = getattr(layer, "mixer", None)
            for name in ("in_proj", "x_proj", "dt_proj", "out_proj"):
                lin = getattr(mixer, name, None)
                if lin is not None:
                    conv_params.append(lin.weight)
        if plan is None or [p.data_ptr() for p in plan.params] != [p.data_ptr() for p in conv_params]:
            plan = plans[dt] = cs.PackPlan(conv_params)
        # tensor version counters see optimizer steps, load_state_dict and every other in-place update, but not
        # writes through ``param.data``: call invalidate_packed_weights() after those.  Training always re-packs.
        version = (sum(p._version for p in conv_params), len(plan.reqs))
        if torch.is_grad_enabled() or getattr(plan, "packed_version", None) != version or not plan.current:
            plan.refresh()
            plan.packed_version = (version[0], len(plan.reqs))
        cs.set_active_plan(plan)

    def invalidate_packed_weights(self):
        """Drop the cached GEMM-layout copies of the conv weights (rebuilt on the next forward)."""
        self.__dict__.pop("_pack_plans", None)
        self.stream.drop_caches(self)                   # (and the hop plan, the hop graph, the stream pools' blobs)

    # ----------------------------------------------------------------- streaming
    def reset_time_per_frame(self):
        self.total_time = 0
        self.frames = 0

    @property
    def time_per_frame(self):
        return 0 if self.frames == 0 else self.total_time / self.frames

    def allocate_inference_cache_layer(self, layer, batch_size, dtype=None):
        return layer.allocate_inference_cache(batch_size, 1, dtype=dtype)

    def allocate_inference_cache(self, batch_size, max_seqlen, dtype=None, **kwargs):
        return {i: self.allocate_inference_cache_layer(layer.mixer, batch_size, dtype=dtype)
                for i, layer in enumerate(self.tsfm_Mamba_layers)}

    def reset_stream(self):
        """Forget all streaming state (pending samples, conv tails, Mamba states): a fresh stream state replaces it."""
        dev = self.tsfm_conv1.weight.device
        self.stream.state = streaming.StreamState(torch.zeros(self.channels_input, 0, dtype=self.dtype, device=dev))

    @torch.no_grad()
    def feed(self, noisy_input):
        """noisy_input: (1, n) samples of one stream -> (1, m) denoised samples, m a multiple of total_stride
        (interface of src/network/CleanUMamba.py:370-418)."""
        if noisy_input.dim() != 2:
            raise ValueError("input should be two dimensional.")
        if noisy_input.shape[0] != 1:
            raise ValueError(f"Expected 1 channel, got {noisy_input.shape[0]}")
        return self.feed_batch(noisy_input)

    @torch.no_grad()
    def flush_batch(self):
        """End of the streams: emit the samples still pending so that feed + flush reproduce ``forward`` on the whole
        signal, tail included.  ``forward`` zero-pads the signal to ``valid_length`` and its last
        ``frame_length - total_stride`` output samples come from the transposed convs' overhang of the LAST real
        frame -- no later frame exists.  So flush (1) pads the stream with exactly the zeros ``forward`` would add
        and runs the hops of the frames that exist, then (2) drains the decoder (``streaming.drain``): the per-layer
        overlap tails and the not-yet-consumed encoder rows are pushed through the remaining decoder layers with no new
        frame.  (The reference's flush(), src/network/CleanUMamba.py:358-368, loses the tail: SURVEY fact 9.)"""
        return streaming.flush_batch(self)

    flush = flush_batch     # (one stream or many: interface of src/network/CleanUMamba.py:358-368)

    @torch.no_grad()
    def feed_batch(self, noisy_input):
        """S concurrent streams in lock-step: (S, n) new samples per stream -> (S, m).  Every stream owns a row of
        the pending buffer, of the per-layer conv tails and of the Mamba conv / SSM states; one hop costs the same
        number of kernel launches whatever S is (the reference streams one clip at a time, batch fixed to 1 at
        src/network/CleanUMamba.py:375-381)."""
        if noisy_input.dim() != 2:
            raise ValueError("input should be two dimensional: (streams, samples)")
        return streaming.feed_batch(self, noisy_input)

    def stream_pool(self, capacity, model_rate=16000, backend=None):
        """A pool of ``capacity`` stream slots on this model (network/streampool.py): streams that join, feed any number of
        samples and leave independently.  ``pool.backend`` says what runs the hops: "kernel", every call's hops in one
        launch of the one-launch hop, wherever that hop runs the model; "layers", the per-layer fused hop on dense batches
        of the slots that have a hop to run, for models that are only too LARGE for it (above hopplan.MAX_PARAMS, a layer
        wider than 1 024 channels, a plan that overruns LDS: the E6 / E8 networks).  ``backend`` forces one of the two.
        The pool keeps its own state; ``feed`` / ``feed_batch`` / ``flush`` of the model are not affected.  Models neither
        runs (Mamba2, non-f32, other kernel / stride, ``stream_bf16`` on the per-layer backend) raise ValueError.
        ``model_rate``: the sample rate the model works at; ``pool.open(rate=...)`` gives a slot that is fed and answers
        at its own rate."""
        from .streampool import StreamPool
        pool = StreamPool(self, capacity, model_rate, backend)
        self.__dict__.setdefault("_stream_pools", weakref.WeakSet()).add(pool)
        return pool

    @property
    def hop_kernel_status(self):
        """"active" while the one-launch hop owns the stream state, else why not ("off", "first frame pending", reason)."""
        if self.stream.state.kernel is not None:
            return "active"
        if not streaming.switch(self, "use_hop_kernel"):
            return "off"
        return self.stream.why or "first frame pending"

    @property
    def hop_graph_status(self):
        """"off" (disabled), "pending" (no hop captured yet), "captured", or "failed: <error>" (hops run eagerly)."""
        if not streaming.switch(self, "use_hop_graph"):
            return "off"
        hg = self.stream.state.graph
        if hg is None:
            return "pending"
        return "failed: " + hg["error"] if hg["failed"] else "captured"

    # ------------------------------------------------------------ pruned loading
    def load_pruned_state_dict(self, pruned_state_dict):
        """Load a structurally pruned checkpoint (interface of src/network/CleanUMamba.py:492-550, used by
        src/examples/loading_pretrained_models.py:12-13): every parameter takes the checkpoint's shape, the
        modules' size attributes follow their new weights, then the dict is loaded strictly.  Keys absent from the
        checkpoint keep their current tensors and are reported by the strict load."""
        resize = {
            nn.LayerNorm: lambda m, w: setattr(m, "normalized_shape", tuple(w.shape)),
            nn.Linear: lambda m, w: (setattr(m, "out_features", w.shape[0]), setattr(m, "in_features", w.shape[1])),
            nn.ConvTranspose1d: lambda m, w: (setattr(m, "in_channels", w.shape[0]),
                                              setattr(m, "out_channels", w.shape[1])),
            # a depthwise conv (the Mamba conv1d) stays depthwise: groups follows the channel count.  in_channels is
            # set to weight.shape[1] (= 1 there) as the reference does; F.conv1d only looks at the tensors.
            nn.Conv1d: lambda m, w: (setattr(m, "out_channels", w.shape[0]), setattr(m, "in_channels", w.shape[1]),
                                     setattr(m, "groups", w.shape[0] if m.groups > 1 else m.groups)),
        }
        for prefix, module in self.named_modules():
            dot = prefix + "." if prefix else ""
            own = list(module._parameters.items()) + [(k, b) for k, b in module._buffers.items()
                                                       if k not in module._non_persistent_buffers_set]
            for name, tensor in own:
                src = pruned_state_dict.get(dot + name)
                if tensor is not None and src is not None:
                    tensor.data = src.detach().clone().to(device=tensor.device)
            if getattr(module, "weight", None) is not None:
                for kind, fix in resize.items():
                    if isinstance(module, kind):
                        fix(module, module.weight)
                        break
        for module in self.modules():
            if type(module).__name__ == "Mamba":       # by name, as the reference does (:540): pickled models qualify
                module.d_model = module.in_proj.in_features
                module.d_inner = module.x_proj.in_features
                module.dt_rank = module.dt_proj.in_features
                module.d_state = (module.x_proj.out_features - module.dt_rank) // 2
                module.expand = module.d_inner / module.d_model
            elif type(module).__name__ == "Mamba2":
                module.d_model = module.in_proj.in_features
                module.nheads = module.A_log.shape[0]
                module.d_ssm = module.d_inner = module.norm.weight.shape[0]
                module.headdim = module.d_ssm // module.nheads
                module.d_state = (module.in_proj.out_features - 2 * module.d_ssm - module.nheads) // 2
                module.expand = module.d_inner / module.d_model
        self.load_state_dict(pruned_state_dict, strict=True)
        self.invalidate_packed_weights()
