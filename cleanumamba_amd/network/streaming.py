"""Streaming runtime behind ``feed`` / ``flush`` of CleanUMamba (semantics: src/network/CleanUMamba.py:358-490).

The state of one set of lock-step streams is ONE object (``StreamState``); "forget the stream" replaces it.  The model
holds a ``Stream`` (``model.stream``: that state and the caches that outlive it) and the path switches; nothing here
keeps a reference to the model -- every function takes it.  Three hops share the state: the cached hop (torch modules),
the fused hop (network/convstack.py; both replayed from a hipGraph where it is on) and the one-launch hop (csrc/hop.hip,
network/hopplan.py), which takes a stream over after its first frame.
"""
import time
import warnings

import torch

from ..mamba_ssm.utils.generation import InferenceParams
from .. import hip
from . import convstack as cs
from . import hopplan

_SWITCHES = {"use_hop_kernel": True, "stream_bf16": False, "stream_incremental": True, "use_fused_stream": True,
             "use_fused_convs": True, "fused_min_streams": 1, "use_hop_graph": False}


def switch(model, name):
    """A path switch of the model (plain attributes, set by name), or the fallback an instance that lacks it gets."""
    return getattr(model, name, _SWITCHES[name])


class StreamState:
    """One set of S lock-step streams."""

    def __init__(self, pending=None):
        self.pending = pending      # (S, n) samples no hop has consumed yet
        self.input_std = 0          # running mean of the per-frame std, (S, 1) ...
        self.frames = 0             # ... over this many frames: those of THIS stream (the model's ``frames`` only times)
        self.layers = {}            # per-layer buffers: 2-D row buffers (fused hop) or (S, C, T) (cached hop)
        self.params = None          # InferenceParams of the Mamba blocks
        self.kernel = None          # one-launch hop owns the stream: {"plan", "state" block, "plan_weights" version}
        self.graph = None           # captured hipGraph of the per-layer hop (it holds the addresses of ``layers``)
        self.wv = None              # weights version of the current call: they cannot change inside one

    def __getstate__(self):
        if self.kernel is not None:
            # a live stream of the one-launch hop keeps its state in the plan's device blocks, which are not pickled: the
            # copy starts a fresh stream (what is left in the per-layer fields is the first frame's state, stale by now)
            return StreamState(self.pending[:, :0].clone()).__dict__
        return dict(self.__dict__, graph=None, wv=None)


class Stream:
    """``model.stream``: the model's own streams and the streaming caches that outlive them (the hop plan itself sits in
    ``model.__dict__["_hop_plan"]``, where bench.py and tools/hop_phase_probe.py read it)."""

    def __init__(self, pending):
        self.state = StreamState(pending)
        self.why = None             # why the one-launch hop declines this model, "" if it does not, None: not asked yet
        self.plist = (None, 0)      # weights_version's parameter list and its age in calls

    def __getstate__(self):
        return {"state": self.state, "why": None, "plist": (None, 0)}

    @property
    def live(self):
        """Whether a stream is under way: pending samples, per-layer state or a state block of the one-launch hop."""
        return self.state.kernel is not None or bool(self.state.layers) or self.state.pending.numel() > 0

    def drop_caches(self, model):
        """Forget what was derived from the weights (hop plan, graph, version memos, the pools' blobs); the state stays."""
        model.__dict__.pop("_hop_plan", None)
        self.why, self.plist = None, (None, 0)      # (shapes may have changed: ask again)
        self.state.graph = self.state.wv = None
        if self.state.kernel is not None:           # a live stream of the one-launch hop holds its own weight blob:
            self.state.kernel["plan_weights"] = None    # re-pack it on the next call
        for pool in list(model.__dict__.get("_stream_pools", ())):
            pool.invalidate_packed_weights()


def weights_version(model):
    """(sum of the parameters' version counters, normalize_input): what a packed plan / captured graph was made at."""
    # In-place updates of any parameter (optimizer steps, load_state_dict) bump these counters.  Walking the module tree
    # costs ~60 us, a whole hop of one stream ~450: the parameter list is cached (pruning replaces Parameter objects).
    plist, age = model.stream.plist
    if plist is None or age >= 64:              # re-walk now and then: foreign code may swap Parameter objects
        plist, age = list(model.parameters()), 0
    model.stream.plist = (plist, age + 1)
    # (normalize_input: a hop plan made with it off has no running-std op, and must not be reused once it is on)
    return (sum(p._version for p in plist), bool(model.normalize_input))


def new_params(model, S):
    return InferenceParams(max_seqlen=1, max_batch_size=S, key_value_memory_dict=model.allocate_inference_cache(S, 1),
                           seqlen_offset=1)


def feed_batch(model, noisy_input):
    st = model.stream.state
    S = noisy_input.shape[0]
    if st.pending.shape[0] != S or st.pending.device != noisy_input.device:
        if st.pending.shape[0] != S and (st.pending.shape[1] != 0 or st.params is not None):
            raise ValueError(f"stream count changed from {st.pending.shape[0]} to {S}; call reset_stream()")
        st.pending = torch.zeros(S, 0, dtype=noisy_input.dtype, device=noisy_input.device)
    if st.params is None:
        st.params = new_params(model, S)
    begin = time.time()
    total_stride, frame_length = model.total_stride, model.frame_length
    st.pending = torch.cat([st.pending, noisy_input], dim=1)
    denoised_frames = []
    st.wv = None                                    # weights cannot change inside one call: checked on its first hop only
    while st.pending.shape[1] >= frame_length:
        ks = kernel_state(model, st) if S else None
        if S and ks is None:                        # one frame on the per-layer hop
            model.frames += 1
            denoised_frames.append(first_frame(model, st, st.pending[:, :frame_length], hop))
            st.pending = st.pending[:, total_stride:]
            continue
        n_hops = (st.pending.shape[1] - frame_length) // total_stride + 1
        if S == 0:                                  # no stream: only the bookkeeping of the hops that would have run
            out = st.pending.new_zeros(0, n_hops * total_stride)
        else:
            # every remaining hop of this call in ONE launch (csrc/hop.hip): a workgroup per stream walks them
            out = torch.empty(S, n_hops * total_stride, dtype=torch.float32, device=st.pending.device)
            ks["plan"].run(ks["state"], st.pending, out, n_hops)
            if model.normalize_input:
                st.input_std = ks["state"][:, 0:1]      # the kernel keeps the running std in the state block
        model.frames += n_hops
        st.frames += n_hops
        denoised_frames.append(out)
        st.pending = st.pending[:, n_hops * total_stride:]
        break
    model.total_time += time.time() - begin
    return torch.cat(denoised_frames, 1) if denoised_frames else torch.zeros(S, 0, device=noisy_input.device)


def first_frame(model, st, frame, denoise):
    """The next frame (S, frame_length) of ``st`` on the per-layer hop ``denoise``, with the running input std: the FIRST
    frame of every stream (the one-launch hop and the stream pools take over behind it) and all where that hop is out."""
    st.frames += 1
    if model.normalize_input:
        # running mean of the per-frame std, per stream (src/network/CleanUMamba.py:399-401), over the frames of THIS
        # stream: it ends at flush() (the reference shares one counter with time_per_frame and never resets either)
        n = st.frames
        st.input_std = (frame.std(dim=1, keepdim=True) + 1e-3) / n + (1 - 1 / n) * st.input_std
        frame = frame / st.input_std
    out = denoise(model, st, frame)[:, :model.total_stride]
    return out * st.input_std if model.normalize_input else out


def flush_batch(model):
    st = model.stream.state
    S, pending_length = st.pending.shape
    consumed = st.frames * model.total_stride
    if consumed + pending_length == 0:
        return torch.zeros(S, 0, device=st.pending.device)
    target = model.valid_length(consumed + pending_length)
    pad = torch.zeros(S, target - consumed - pending_length, device=st.pending.device, dtype=st.pending.dtype)
    head = model.feed_batch(pad)      # the frames forward() has: they count as timed frames like any other
    if S and st.kernel is not None:                     # the one-launch hop owns the state: bring it back
        st.layers = st.kernel["plan"].export_state(st, st.kernel["state"])
    out = torch.cat([head, drain(model, st.layers, st.input_std).to(head.dtype)], 1)[:, :pending_length] if S \
        else head.new_zeros(0, pending_length)
    model.reset_stream()              # the next clip starts a fresh stream: its running std starts over too
    return out


def drain(model, layers, std):
    """Output samples behind the last hop, (S, frame_length - total_stride): what ``forward`` produces there.
    Decoder layer j still holds 2 overhang rows of its transposed conv (``dec{j}``, bias excluded) and encoder
    layer i holds ``2^(E-i) - 2`` output rows no hop has consumed as skips yet; layer j maps its
    ``2^(j+1) - 2`` trailing input rows to ``2^(j+2) - 2`` trailing output rows.
    layers: per-layer buffers of S streams in the fused hop's layout, or the cached hop's (also that of
    hopplan.HopPlan.export_rows); std: their running std, (S, 1), read with normalize_input."""
    S, dev, E = layers["dec0"].shape[0], layers["dec0"].device, model.encoder_n_layers
    rows_layout = layers["enc0"].dim() == 2                # fused hop: 2-D row buffers; cached hop: (S, C, T)

    def trailing_skip(i):
        t = layers[f"enc{i}"]
        hop = model.total_stride // model.stride ** (i + 1)
        if not rows_layout:                                # cached path: (S, C, rows not yet consumed)
            return t.float()
        C = model.encoder[i][2].weight.shape[0] // 2       # fused path: row buffer of the frame's whole window
        T = model.frame_length
        for _ in range(i + 1):
            T = (T - model.kernel_size) // model.stride + 1
        return cs.from_rows(t, cs.Geo(S, T, C))[..., hop:].float()

    def tail(j):
        t = layers[f"dec{j}"]
        if rows_layout:                                    # fused path: (S, 2, Cp) channels-last
            return t.transpose(1, 2)[:, :model.decoder[j][2].weight.shape[1]].float()
        return t.float()                                   # cached path: (S, C, 2)

    from ..mamba_ssm.modules.mamba_simple import _proj       # cum_gemm_nt on padded operands: any channel count
    if dev.type == "cuda":
        # the drain's GEMM operands come out of the model's pack plan: re-pack if a parameter changed since the last
        # per-layer hop (the one-launch hop packs its own blob and never touches the plan)
        model._activate_pack_plan(torch.float32)

    def linear_ct(w2d, x):
        """(O, C) x (S, C, T) -> (S, O, T) on the library's GEMM (a handful of columns per stream: rows = S * T)."""
        return _proj(x.transpose(1, 2).contiguous(), w2d.contiguous()).transpose(1, 2)

    def conv_t(g, conv):
        """ConvTranspose1d on a handful of columns as one GEMM per tap + K strided adds (the few-column shapes of the
        drain are not worth a MIOpen solver search, and small transposed convs abort in MIOpen on some boxes)."""
        w, K, S = conv.weight.float(), model.kernel_size, model.stride           # (Cin, Cout, K)
        T = g.shape[-1]
        out = conv.bias.float().view(1, -1, 1).repeat(g.shape[0], 1, (T - 1) * S + K)
        for k in range(K):
            out[..., k:k + (T - 1) * S + 1:S] += linear_ct(w[:, :, k].t(), g)
        return out

    x = None
    for j, dec in enumerate(model.decoder):
        if j == 0:
            y = tail(0) + dec[2].bias.float().view(1, -1, 1)
        else:
            x = x + trailing_skip(E - 1 - j)[..., :x.shape[-1]]
            pre = linear_ct(dec[0].weight.float().squeeze(-1), x) + dec[0].bias.float().view(1, -1, 1)
            y = conv_t(dec[1](pre), dec[2])
            y[..., :model.stride] += tail(j)
        if j != E - 1:
            y = torch.relu(y)
        x = y
    return x[:, 0] * std if model.normalize_input else x[:, 0]


def kernel_state(model, st):
    """{"plan", "state", "plan_weights"} once the one-launch hop (csrc/hop.hip) can take this stream's hops, else None: it
    needs a model the plan supports (hopplan.unsupported_reason), f32 streams on the GPU, and the state the per-layer path
    leaves after the FIRST frame of the streams (whole windows, no history), which is converted here once."""
    ks = st.kernel
    if ks is not None:
        wv = st.wv = weights_version(model) if st.wv is None else st.wv
        if ks["plan_weights"] != wv:                  # weights changed under a live stream: re-pack them
            try:
                ks["plan"], ks["plan_weights"] = hopplan.HopPlan(model), wv
            except ValueError as exc:                   # (same guard as at creation; here the stream state already
                # lives in the old plan's layout, which the per-layer hop cannot take over mid-stream)
                raise RuntimeError("the weights changed under a live stream into a model the one-launch hop cannot "
                                   f"run ({exc}); flush() / reset_stream() before changing them") from exc
        return ks
    if not (switch(model, "use_hop_kernel") and switch(model, "stream_incremental")) or switch(model, "stream_bf16"):
        return None
    if "enc0" not in st.layers or st.layers["enc0"].dim() != 2 or not st.pending.is_cuda \
            or st.pending.dtype != torch.float32 or st.pending.stride(1) != 1:
        return None
    if model.stream.why is None:
        model.stream.why = hopplan.unsupported_reason(model) or ""
    if model.stream.why:
        return None
    wv = st.wv = weights_version(model)
    cached = model.__dict__.get("_hop_plan")        # (version, HopPlan): kept on the model under this key, across
    if cached is None or cached[0] != wv:           # streams -- bench.py and tools/hop_phase_probe.py read it there
        try:
            cached = (wv, hopplan.HopPlan(model))
        except ValueError as exc:                       # e.g. LDS budget: stay on the per-layer path
            model.stream.why = str(exc)
            return None
        model.__dict__["_hop_plan"] = cached
    st.kernel = {"plan": cached[1], "plan_weights": wv, "state": cached[1].import_state(st)}
    st.graph = None
    return st.kernel


def hop(model, st, frame):
    """One per-layer hop: eager the first time (it creates the state buffers), hipGraph replay afterwards."""
    denoise = cached_hop
    if frame.is_cuda and switch(model, "use_fused_stream") and switch(model, "use_fused_convs") \
            and cs.supported(model) and frame.shape[1] == model.valid_length(1) and frame.dtype == torch.float32 \
            and frame.shape[0] >= switch(model, "fused_min_streams"):
        # (single streams too: 0.45 ms per hop against 0.52 ms on the cached path)
        denoise = fused_hop
    if not (switch(model, "use_hop_graph") and frame.is_cuda and st.layers):
        return denoise(model, st, frame)
    hg = st.graph
    wv = st.wv = weights_version(model) if st.wv is None else st.wv
    if hg is not None and not hg.get("failed") and hg.get("weights") != wv:
        hg = None          # the graph replays kernels on the weight copies of its capture: capture again
    if hg is None:
        try:
            static_in = frame.clone()
            stream = torch.cuda.Stream(device=frame.device)
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):      # warm-up on a side stream, as graph capture requires
                live = list(st.layers.values()) + [t for v in st.params.key_value_memory_dict.values() for t in v]
                saved = [t.clone() for t in live]
                denoise(model, st, static_in, True)
                for dst, src in zip(live, saved):       # undo the warm-up's state changes
                    dst.copy_(src)
            torch.cuda.current_stream().wait_stream(stream)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                static_out = denoise(model, st, static_in, True)
            # capture does not execute: state is untouched
            hg = dict(failed=False, graph=graph, static_in=static_in, static_out=static_out, shape=frame.shape, weights=wv)
        except Exception as exc:                 # noqa: BLE001 - capture is an optimisation; stay eager
            hg = {"failed": True, "error": repr(exc)}
            warnings.warn(f"CleanUMamba: hipGraph capture of the streaming hop failed ({exc!r}); this stream "
                          "runs its hops eagerly (2-4x slower).  See model.hop_graph_status.")
        st.graph = hg
    if hg["failed"] or hg["shape"] != frame.shape:
        return denoise(model, st, frame)
    hg["static_in"].copy_(frame)
    hg["graph"].replay()
    return hg["static_out"].clone()


def fused_hop(model, st, frame, inplace=True):
    """One hop on the fused GEMM kernels, same arithmetic as ``cached_hop``.  Every encoder layer keeps a persistent
    window of its output (the decoder's skips read its oldest rows); the first hop of a stream computes the
    windows whole (S independent clips of valid_length(1) samples), later hops compute only the hop's new rows
    from the newest rows of the window below (cum_stream_tail_rows) and append them (cum_stream_window_update),
    so older activations keep the input scaling of the hop that produced them, as with the reference's per-layer
    caches (``stream_incremental = False`` recomputes the windows every hop); a decoder layer is
    1x1+GLU GEMM, transposed-conv GEMM and one overlap-add kernel (cum_stream_overlap_add) that also applies
    ReLU, adds the skip and keeps the tail for the next hop."""
    assert inplace, "the fused hop always updates its stream state in place"
    with cs.small_m_gemms():
        return _fused_hop(model, st.layers, st.params, frame)


def _fused_hop(model, state, inference_params, frame):
    S, E, dev = frame.shape[0], model.encoder_n_layers, frame.device
    dt = torch.bfloat16 if switch(model, "stream_bf16") else torch.float32
    model._activate_pack_plan(dt)
    geo = cs.Geo(S, frame.shape[1], model.encoder[0][0].weight.shape[1])
    lib, dc = hip.lib(), hip.dtype_code(dt)
    # After the first hop of a stream only the hop's new rows of every layer are computed: layer i emits
    # n = total_stride >> (i + 1) rows from the 2 n + 2 newest rows of its input (2 carried + 2 n new ones).
    incremental = state.get("enc0") is not None and switch(model, "stream_incremental")
    buf = None if incremental else cs.to_rows(frame.unsqueeze(1), geo, dt)
    enc_geos, outs, n_new = [], [], model.total_stride
    for i, enc in enumerate(model.encoder):
        T1 = (geo.T - model.kernel_size) // model.stride + 1
        g_mid = cs.Geo(S, T1, enc[0].weight.shape[0])
        g_out = cs.Geo(S, T1, enc[2].weight.shape[0] // 2)
        n_new //= model.stride
        window = state.get(f"enc{i}")
        t_in = model.stride * n_new + model.kernel_size - model.stride      # rows of the incremental hops' compact input
        g_cin = cs.Geo(S, t_in, geo.C)
        if incremental:
            xin = state.get(f"encin{i}")
            if xin is None:                   # persistent: its framing rows are zeroed once
                xin = state[f"encin{i}"] = g_cin.new(dt, dev, zero=True)
            if i == 0:
                g_cin.rows(xin)[:, :t_in, :1] = frame[:, frame.shape[1] - t_in:].unsqueeze(-1).to(dt)
            # (deeper layers: the window update of the layer below has already written xin)
            g_cm, g_co = cs.Geo(S, n_new, g_mid.C), cs.Geo(S, n_new, g_out.C)
            y1 = cs._conv_relu_fwd(xin, enc[0].weight, enc[0].bias, g_cin, g_cm)
            fresh, _ = cs._glu_fwd(y1, enc[2].weight, enc[2].bias, g_cm, g_co, False)
            nxt = state.get(f"encin{i + 1}")   # the next layer's compact input: 2 carried rows + the new ones
            with torch.cuda.device(dev):        # in place, one launch (windows are far below 8192 kept rows)
                hip.check(lib.cum_stream_window_update(dc, S, g_out.T, n_new, g_out.Cp, hip.ptr(window[1:]),
                                                       hip.ptr(fresh[1:]), g_out.P, g_co.P, g_out.T - n_new,
                                                       None, None if nxt is None else hip.ptr(nxt[1:]),
                                                       n_new + 4, hip.stream_ptr()))
        else:
            y1 = cs._conv_relu_fwd(buf, enc[0].weight, enc[0].bias, geo, g_mid)
            fresh, _ = cs._glu_fwd(y1, enc[2].weight, enc[2].bias, g_mid, g_out, False)
            # the layer's window keeps older rows as the hop that produced them left them (per-layer caches of
            # the reference, :425-447): only the n_new newest rows of the recomputed window are taken over
            if window is None:
                window = state[f"enc{i}"] = fresh
                # compact input of the incremental hops; allocated here so that the captured hop allocates nothing
                state[f"encin{i}"] = g_cin.new(dt, dev, zero=True)
            else:
                with torch.cuda.device(dev):
                    hip.check(lib.cum_stream_window_update(dc, S, g_out.T, n_new, g_out.Cp, hip.ptr(window[1:]),
                                                           hip.ptr(fresh[1:]), g_out.P, g_out.P, 0, None, None, 0,
                                                           hip.stream_ptr()))
        enc_geos.append((geo, g_mid, g_out))
        outs.append(window)
        buf, geo = window, g_out
    x, _ = model._bottleneck(cs.from_rows(outs[-1], geo).float(), inference_params=inference_params,
                             pointwise_as_linear=True)                                                     # (S, C, 1)
    L = x.shape[-1]
    x = x + cs.from_rows(outs[-1], geo)[..., :L].float()
    g_in = cs.Geo(S, L, x.shape[1])
    ubuf = cs.to_rows(x, g_in, dt)
    for j, dec in enumerate(model.decoder):
        last = j == E - 1
        g_glu = cs.Geo(S, L, dec[0].weight.shape[0] // 2)
        g_ct = cs.Geo(S, 2 * L + 2, dec[2].weight.shape[1])
        gbuf, _ = cs._glu_fwd(ubuf, dec[0].weight, dec[0].bias, g_in, g_glu, False)
        ybuf, _ = cs._convt_fwd(gbuf, dec[2].weight, dec[2].bias, None, g_glu, g_ct, False)
        tail = state.get(f"dec{j}")
        if tail is None:                       # first hop of the stream: nothing to overlap with
            tail = state[f"dec{j}"] = torch.zeros(S, 2, g_ct.Cp, dtype=dt, device=dev)
        g_next = cs.Geo(S, 2 * L, g_ct.C)
        # persistent between hops (the kernel rewrites every data row, the framing rows stay zero) -- except the
        # last layer's, which is handed to the caller
        nbuf = None if last else state.get(f"decbuf{j}")
        if nbuf is None or nbuf.dtype != dt:
            nbuf = g_next.new(dt, dev, zero=True)
            if not last:
                state[f"decbuf{j}"] = nbuf
        skip, skip_pitch = None, 0
        if not last:
            sbuf, g_skip = outs[E - 2 - j], enc_geos[E - 2 - j][2]
            assert g_skip.C == g_ct.C and g_skip.T >= 2 * L
            skip, skip_pitch = sbuf[1:], g_skip.P
        with torch.cuda.device(dev):
            hip.check(lib.cum_stream_overlap_add(
                hip.dtype_code(dt), S, 2 * L, g_ct.Cp, g_ct.C, hip.ptr(ybuf[1:]), g_ct.P, hip.ptr(tail),
                hip.ptr(dec[2].bias.float()), hip.ptr(skip), skip_pitch, hip.ptr(nbuf[1:]), g_next.P,
                int(not last), hip.stream_ptr()))
        ubuf, g_in, L = nbuf, g_next, 2 * L
    return cs.from_rows(ubuf, g_in)[:, 0].float()


def cached_hop(model, st, frame, inplace=False):
    """One hop on the torch modules: frame (S, frame_length) -> (S, >= total_stride) samples.  Encoder outputs that
    overlap the previous frame are cached per layer; the decoder keeps the last ``stride`` samples of every
    transposed conv for overlap-add with the next frame."""
    x = frame.unsqueeze(1)
    state = st.layers
    skip_connections = []
    hop = model.total_stride
    for i, encode in enumerate(model.encoder):
        hop //= model.stride                     # new outputs of this layer per frame
        prev = state.get(f"enc{i}")
        if prev is not None:
            length = x.shape[2]
            n_new = (length - model.kernel_size) // model.stride + 1 - prev.shape[-1]
            x = x[..., length - model.kernel_size - model.stride * (n_new - 1):]
        x = encode(x)
        if prev is not None:
            x = torch.cat([prev, x], -1)
        if inplace:
            prev.copy_(x[..., hop:])             # static buffer (hipGraph replay reads it next hop)
        else:
            state[f"enc{i}"] = x[..., hop:].clone()
        skip_connections.append(x)
    x, _ = model._bottleneck(x, inference_params=st.params)
    for i, upsampling_block in enumerate(model.decoder):
        skip_i = skip_connections[-1 - i]        # deepest first, as in forward()
        x = x + skip_i[..., :x.shape[-1]]
        x = upsampling_block[2](upsampling_block[1](upsampling_block[0](x)))
        prev = state.get(f"dec{i}")
        tail = x[..., -model.stride:] - upsampling_block[2].bias.view(-1, 1)
        x = x[..., :-model.stride]
        if prev is not None:
            x = torch.cat([x[..., :model.stride] + prev, x[..., model.stride:]], -1)
        if inplace:
            prev.copy_(tail)
        else:
            state[f"dec{i}"] = tail
        if i != model.encoder_n_layers - 1:
            x = upsampling_block[3](x)
    return x[:, 0]
