/*
 * cleanumamba_hip.h -- C ABI of libcleanumamba_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the CleanUMamba forward+backward hot path.  Each entry
 * point replaces one native op the reference reaches through third-party wheels
 * (mamba-ssm 1.2.2, causal-conv1d 1.1.0; pinned at /root/reference
 * environment.yml:29-30) or through cuDNN/cuBLAS via torch.nn:
 *
 *   cum_selective_scan_fwd/bwd    <- selective_scan_cuda.fwd/bwd, reached from
 *                                    Mamba.forward via create_block
 *                                    (src/network/CleanUMamba.py:172-189, 289-290)
 *   cum_causal_conv1d_fwd/bwd     <- causal_conv1d_cuda.causal_conv1d_fwd/bwd
 *                                    (call pattern src/network/S4/MambaS4.py:454-463)
 *   cum_causal_conv1d_update      <- causal_conv1d_cuda.causal_conv1d_update   (Mamba.step,
 *   cum_selective_state_update    <- selective_state_update                     CleanUMamba.py:451-454)
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the
 *     caller (PyTorch caching allocator).  Kernels never allocate or free.
 *   - strides are in ELEMENTS.  "len" is the time axis, "dim" the channel axis.
 *     The kernels are tuned for channel-contiguous (stride_dim == 1) tensors and
 *     remain correct for any stride.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it and
 *     the call returns immediately (no synchronisation, graph-capturable).
 *   - return value: CUM_OK (0) or a negative CUM_E* code; nothing throws.
 *     cum_last_error() returns a static description of the last failure on the
 *     calling thread.
 *   - re-entrant: no global mutable state besides the thread-local error string.
 */
#ifndef CLEANUMAMBA_HIP_H
#define CLEANUMAMBA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CUM_OK 0
#define CUM_EINVAL (-1)      /* bad argument / unsupported shape */
#define CUM_ELAUNCH (-2)     /* hipLaunch failed */
#define CUM_EWORKSPACE (-3)  /* workspace too small */

#define CUM_ABI_VERSION 16

int cum_abi_version(void);
const char *cum_last_error(void);

/* Time steps between saved scan states (fixed by the kernels). */
int cum_scan_chunk(void);

/* ------------------------------------------------------------ selective scan
 * Logical shapes: u, delta, z, out: (batch, dim, len); A: (dim, dstate) row-major
 * contiguous fp32; Bm, Cm: (batch, dstate, len); D, delta_bias: (dim) or NULL;
 * z may be NULL (no gate).  x_{t} = exp(delta_t A) x_{t-1} + delta_t B_t u_t,
 * y_t = <C_t, x_t> + D u_t, out = y * silu(z).   
 *
 * ckpt: NULL (inference) or fp32 buffer of cum_scan_ckpt_elems() elements that
 * receives the state entering every half of every chunk of cum_scan_chunk() steps
 * (opaque layout, 16-byte aligned); the backward consumes it.  last_state: NULL or (batch, dim, dstate) contiguous.
 */
#define CUM_SCAN_SOFTPLUS 1
#define CUM_SCAN_A_IS_LOG 2
typedef struct {
  int32_t batch, dim, dstate, len;
  int64_t u_sb, u_sd, u_sl;          /* u strides: batch, dim, len */
  int64_t dt_sb, dt_sd, dt_sl;       /* delta */
  int64_t z_sb, z_sd, z_sl;          /* z (ignored if z == NULL) */
  int64_t o_sb, o_sd, o_sl;          /* out */
  int64_t B_sb, B_sn, B_sl;          /* Bm */
  int64_t C_sb, C_sn, C_sl;          /* Cm */
  int32_t delta_softplus;            /* flag word.  bit 0: apply softplus (threshold 20) to delta + bias.
                                        bit 1 (CUM_SCAN_A_IS_LOG = 2): `A` holds A_log -- the op uses A = -exp(A_log), as
                                        upstream Mamba.forward forms it from its parameter, and the backward returns
                                        dA_log = dA * A in `dA` (no elementwise launches around the op) */
  int32_t io_dtype;                  /* CUM_F32 / CUM_BF16 / CUM_F16: element type of u, delta, z, out and of dout, du,
                                        ddelta, dz (what autocast hands over); all arithmetic and every other
                                        tensor stay fp32 */
} cum_scan_shape;

int64_t cum_scan_ckpt_elems(int32_t batch, int32_t dim, int32_t dstate, int32_t len);

int cum_selective_scan_fwd(const cum_scan_shape *s, const void *u, const void *delta,
                           const float *A, const float *Bm, const float *Cm, const float *D,
                           const void *z, const float *delta_bias, void *out,
                           float *last_state, float *ckpt, void *stream);

/* The same op with a workspace, which lets the library take its TIME-PARALLEL form where the sequential grid
 * (batch * ceil(dim/64) * ceil(dstate/8) waves) does not fill the chip -- file denoising at batch 1
 * (src/examples/denoise.py), the 442K model, the pruned checkpoints: the sequence is cut into segments, every segment is
 * walked from a zero state, the segments' (decay, end state) pairs are composed with the scan's associative operator
 * (a, b) o (a', b') = (a' a, a' b + b'), and every segment is re-walked from its true entering state (scan_seg.hip).
 * Outputs, last_state and the checkpoints have the same meaning and layout; results equal the sequential kernels' up to
 * f32 rounding of the segment decay.  workspace: f32, cum_scan_fwd_workspace_elems() elements -- 0 means the sequential
 * kernels run (pass NULL); a NULL workspace always selects them. */
int64_t cum_scan_fwd_workspace_elems(int32_t batch, int32_t dim, int32_t dstate, int32_t len);
int cum_selective_scan_fwd_ws(const cum_scan_shape *s, const void *u, const void *delta,
                              const float *A, const float *Bm, const float *Cm, const float *D,
                              const void *z, const float *delta_bias, void *out, void *y_pre,
                              float *last_state, float *ckpt, float *workspace, void *stream);
/* y_pre: NULL, or a buffer of out's element type and strides that receives y before the gate (y_t = <C_t, x_t> + D u_t),
 * which the backward then reads instead of rebuilding it (one packed fma per state pair and step saved there).  Only where
 * cum_scan_fwd_keeps_y() returns 1 for the shape (the sequential kernel for d_state > 16: the E6 / E8 bottleneck). */
int32_t cum_scan_fwd_keeps_y(int32_t batch, int32_t dim, int32_t dstate, int32_t len, int32_t with_workspace);

/* Inference forward that CONTINUES a sequence: cum_selective_scan_fwd_ws without ckpt and y_pre, plus the state entering
 * t = 0.  init_state: NULL (zero: the plain forward) or (batch, dim, dstate) contiguous f32 -- last_state's layout, so one
 * call's last_state is the next call's init_state and a sequence cut anywhere gives the uncut outputs up to f32 rounding
 * (the prefill of upstream's mamba_simple.py:356-371, which can hand a state out but not take one in).  Honoured by
 * every forward kernel the dispatcher picks; in the time-parallel form it is X_0 of the carry prologue.  init_state and
 * last_state must not overlap (later segments read the one while the last segment writes the other): CUM_EINVAL before
 * any launch.  len == 0 copies init_state to last_state. */
int cum_selective_scan_fwd_from(const cum_scan_shape *s, const void *u, const void *delta,
                                const float *A, const float *Bm, const float *Cm, const float *D,
                                const void *z, const float *delta_bias, void *out,
                                const float *init_state, float *last_state, float *workspace, void *stream);

/* Strides (batch, dim, len) of the three per-element gradient outputs. */
typedef struct {
  int64_t du_sb, du_sd, du_sl;
  int64_t dd_sb, dd_sd, dd_sl;       /* ddelta */
  int64_t dz_sb, dz_sd, dz_sl;       /* dz (ignored if z == NULL) */
} cum_scan_grad_strides;

/* Backward.  dout strides = the o_* strides of the shape; du/ddelta/dz use `gs`.
 * dB, dC: (batch, len, dstate) CONTIGUOUS fp32 outputs.
 * dA: (dim, dstate), dD, ddelta_bias: (dim) -- fully overwritten (not accumulated).
 * workspace: fp32, cum_scan_bwd_workspace_elems() elements.
 * y_pre: NULL, or the forward's y_pre (dout's strides): with z != NULL the kernel needs y before the gate and rebuilds it
 * when it is not given. */
int64_t cum_scan_bwd_workspace_elems(int32_t batch, int32_t dim, int32_t dstate, int32_t len);

int cum_selective_scan_bwd(const cum_scan_shape *s, const cum_scan_grad_strides *gs,
                           const void *u, const void *delta,
                           const float *A, const float *Bm, const float *Cm, const float *D,
                           const void *z, const float *delta_bias, const void *dout, const void *y_pre,
                           const float *ckpt, void *du, void *ddelta, float *dA, float *dB,
                           float *dC, float *dD, void *dz, float *ddelta_bias,
                           float *workspace, void *stream);

/* Time-parallel backward for grids that leave the chip mostly idle (d_state <= 16: the 442K model, the pruned
 * checkpoints, reached when the reference trains / fine-tunes them, src/network/CleanUMamba.py:289-290): the reverse
 * recurrence dx_t = C_t dy_t + a_{t+1} dx_{t+1} is the forward's linear operator run backwards, so time splits into
 * segments of whole 16-step chunks -- pass 1 walks every segment but the first from a zero carry (its leaving carry and
 * its sum of delta'), pass 2 walks every segment with the carry composed from the later ones and computes all
 * gradients from the forward's checkpoints (csrc/scan_bwd_small.hip).  Same arguments and results as
 * cum_selective_scan_bwd (bit-reproducible; equal to it up to the f32 rounding of the segment decay);
 * workspace: cum_scan_bwd_tp_workspace_elems() elements -- 0 means "the plan keeps this shape sequential: call
 * cum_selective_scan_bwd". */
int64_t cum_scan_bwd_tp_workspace_elems(int32_t batch, int32_t dim, int32_t dstate, int32_t len);
int cum_selective_scan_bwd_tp(const cum_scan_shape *s, const cum_scan_grad_strides *gs,
                              const void *u, const void *delta,
                              const float *A, const float *Bm, const float *Cm, const float *D,
                              const void *z, const float *delta_bias, const void *dout, const void *y_pre,
                              const float *ckpt, void *du, void *ddelta, float *dA, float *dB,
                              float *dC, float *dD, void *dz, float *ddelta_bias,
                              float *workspace, void *stream);

/* One time step for `batch` concurrent streams (Mamba.step).  state (batch, dim,
 * dstate) contiguous, updated in place.  x, dt, z, out: (batch, dim) contiguous;
 * Bv, Cv: (batch, dstate) with element stride 1 and row strides B_sb / C_sb. */
int cum_selective_state_update(int32_t batch, int32_t dim, int32_t dstate, float *state,
                               const float *x, const float *dt, const float *A,
                               const float *Bv, int64_t B_sb, const float *Cv, int64_t C_sb,
                               const float *D, const float *z, const float *dt_bias,
                               int32_t dt_softplus, float *out, void *stream);

/* ------------------------------------------------------- causal depthwise conv
 * y[b,d,t] = act(bias_d + sum_k w[d,k] x[b,d,t-(W-1)+k]), zero left pad, W <= 4.
 * (SURVEY.md Appendix A.4).  weight (dim, width) contiguous, bias (dim) or NULL.
 * silu: 1 -> SiLU activation, 0 -> identity. */
typedef struct {
  int32_t batch, dim, len, width;
  int64_t x_sb, x_sd, x_sl;
  int64_t y_sb, y_sd, y_sl;
  int32_t silu;
  int32_t io_dtype;                  /* CUM_F32 / CUM_BF16 / CUM_F16: element type of x, y, dy, dx; weights stay fp32 */
} cum_conv_shape;

int cum_causal_conv1d_fwd(const cum_conv_shape *s, const void *x, const float *weight,
                          const float *bias, void *y, void *stream);

/* The forward continuing a sequence.  state_in, state_out: NULL or (batch, dim, width) contiguous f32, the layout
 * cum_causal_conv1d_update keeps (column j of the state after `len` inputs = the input at time len - width + j), so a
 * later update continues from state_out.  Times t < 0 read state_in's newest width - 1 columns instead of zero (NULL:
 * zero); state_out takes its columns from state_in where len < width.  The two must not overlap: CUM_EINVAL before any
 * launch. */
int cum_causal_conv1d_fwd_from(const cum_conv_shape *s, const void *x, const float *weight,
                               const float *bias, void *y, const float *state_in, float *state_out,
                               void *stream);

/* dy has y's strides; dx has strides (dx_sb, dx_sd, dx_sl).  dweight (dim, width),
 * dbias (dim): overwritten.  workspace: cum_conv_bwd_workspace_elems() fp32 elements. */
int64_t cum_conv_bwd_workspace_elems(int32_t batch, int32_t dim, int32_t len, int32_t width);

int cum_causal_conv1d_bwd(const cum_conv_shape *s, const void *x, const float *weight,
                          const float *bias, const void *dy, void *dx, int64_t dx_sb,
                          int64_t dx_sd, int64_t dx_sl, float *dweight, float *dbias,
                          float *workspace, void *stream);

/* Streaming step: conv_state (batch, dim, width) contiguous is shifted left by one
 * and x (batch, dim) appended; y (batch, dim) = act(bias + <state, w>). */
int cum_causal_conv1d_update(int32_t batch, int32_t dim, int32_t width, float *conv_state,
                             const float *x, const float *weight, const float *bias,
                             int32_t silu, float *y, void *stream);

/* ------------------------------------------- encoder / decoder layers as fused GEMMs
 * Replaces cuDNN/cuBLAS behind nn.Conv1d / nn.ConvTranspose1d (+ ReLU / GLU / skip add)
 * of the encoder and decoder layers (src/network/CleanUMamba.py:108-113, 121-130,
 * 313-316; GLU src/network/layers.py:26-33).
 *
 *   out[m][n] = epilogue( sum_k A[m*lda + k] * W[n*ldw + k] + bias[n] )   (+ res[m][n])
 *
 * A rows may overlap (lda < K): with channels-last activations [B, T+2, C] a Conv1d
 * (k=4, s=2) output row reads 4*C contiguous elements at row stride 2*C, and a
 * ConvTranspose1d (k=4, s=2) output row pair reads 2*C contiguous elements at row
 * stride C, so both are this GEMM with re-packed weights (DESIGN.md "conv stack").
 * W is [N][ldw] with the K axis contiguous and zero-padded to K; bias is f32[N].
 * epilogue: 0 bias, 1 bias+ReLU, 2 bias+GLU (weights packed 16 a-rows then 16 b-rows per
 * 32 rows; the output has N/2 columns).  Rows with (m % pitch) >= valid are written as
 * zeros.  aux (optional): GLU -> the pre-activation [M][ldz] (N columns);
 * otherwise -> the activation before the residual add.  res is added after the activation.
 * Two backward-data epilogues fold the elementwise backward of the NEXT op into the GEMM
 * that produces its input gradient (autograd of ReLU / GLU in the same reference lines):
 *   3 (MASK): res = the ReLU output Y of the layer below; out = (Y > 0) ? acc + bias : 0 and,
 *     if aux != NULL, aux = acc + bias ungated (the gradient that also feeds a skip path);
 *   4 (GLU_BWD): d = acc (+ res, e.g. the gradient arriving over a skip path) is the gradient
 *     of a GLU output; aux = its saved pre-activation Z (INPUT, [M][ldz], 16 a | 16 b per 32
 *     columns); out = dZ in Z's layout ([M][ldc]): for the 16-column tile t of row m,
 *     out[32t + j] = d_j * sig(b_j), out[32t + 16 + j] = d_j * a_j * sig(b_j) * (1 - sig(b_j)).
 *     n_store counts columns of d; zero_head / zero_tail must be 0.
 * dtype: element type of A, W, res, out, aux; accumulation is always f32. */
#define CUM_F32 0
#define CUM_BF16 1
#define CUM_F16 2   /* IEEE half: what torch.autocast("cuda") hands over by default (the reference's training mode,
                       configs/config.json:14, src/training/train.py:158-160, 278-280) */

typedef struct {
  int32_t dtype, epilogue;
  int32_t M, N, K;           /* N multiple of 16 (32 for GLU); K multiple of 64 (bf16, f16) / 32 (f32) */
  int64_t lda, ldw, ldc, ldr, ldz;
  int32_t pitch, valid;
  int32_t n_store;           /* output columns written (multiple of 4) */
  int64_t zero_head;         /* elements in front of out[0] to clear (the buffer's leading zero row) */
  int64_t zero_tail;         /* elements behind out[M*ldc] to clear (the buffer's slack rows); both also */
                             /* applied to aux when it has out's geometry (epilogue != GLU)             */
  int32_t gate_only;         /* GLU (2): aux receives only the gate pre-activation b, [M][ldz] in the output's   */
                             /* column order (half the bytes of the (a | b) form).  GLU_BWD (4): aux is that b   */
                             /* and aux2 the GLU output y = a*sig(b) saved by the forward ([M][ldy]):            */
                             /* da = d*sig(b), db = d*y*(1 - sig(b)) -- a itself is never needed                 */
  int64_t ldy;
  int32_t mask_bits;         /* RELU (1): aux receives only the SIGN (activation > 0) of each element, four       */
                             /* consecutive channels per byte (low nibble; byte index (m*ldz + n) / 4).  MASK (3): */
                             /* res is such an array (byte index (m*ldr + n) / 4).  1/8 of the bytes of a bf16 mask */
  int32_t allow_split_k;     /* 1: launches with few tiles (M = streams x a handful of rows) may use the small-M      */
                             /* kernel, which splits the K axis over the four waves of a 64x64 tile: same result up  */
                             /* to summation order.  The host sets it for inference (streaming hops, no-grad forward);  */
                             /* training keeps one summation order for every shape.                                 */
} cum_gemm_desc;

int cum_gemm_nt(const cum_gemm_desc *d, const void *A, const void *W, const float *bias,
                const void *res, void *out, void *aux, const void *aux2, void *stream);
/* Which kernel cum_gemm_nt runs for this problem (only dtype, M, N, K, allow_split_k are read): 64 = 64 x 64 tiles with
 * K split over the waves, 128 = 128 x 128, 256 = 256 x 128 (f32), 384 = 128 x 256 through a three-stage LDS ring (16-bit,
 * launches with 40 ... 256 such tiles and K >= 512), 512 = 256 x 256 with two wave groups in ping-pong (16-bit).  Lets a
 * parity test state which kernel a shape was verified on. */
int cum_gemm_nt_tile(const cum_gemm_desc *d);

/* GLU backward on the packed pre-activation Z [M][ldz] (n_groups x (16 a | 16 b));
 * dOut [M][ldo] has 16 channels per group (n_out valid columns); dZ has Z's layout. */
int cum_glu_bwd(int32_t dtype, int64_t M, int32_t n_groups, int32_t n_out, const void *Z,
                int64_t ldz, const void *dOut, int64_t ldo, void *dZ, void *stream);
/* Same from the gate-only form: Bg [M][ldb] (gate pre-activations, 16 per group) and Y [M][ldy] (the GLU
 * output); dZ [M][ldz] in the packed (16 a | 16 b) layout. */
int cum_glu_bwd_gate(int32_t dtype, int64_t M, int32_t n_groups, int32_t n_out, const void *Bg,
                     int64_t ldb, const void *Y, int64_t ldy, const void *dOut, int64_t ldo, void *dZ,
                     int64_t ldz, void *stream);

/* dZ = dOut * (Y > 0) over M rows x n_cols columns (n_cols multiple of 4).  zero_head / zero_tail:
 * elements in front of dZ[0] / behind dZ[M*ldz] to clear (leading zero row / slack rows). */
int cum_relu_bwd(int32_t dtype, int64_t M, int32_t n_cols, const void *Y, int64_t ldy,
                 const void *dOut, int64_t ldo, void *dZ, int64_t ldz, int64_t zero_head,
                 int64_t zero_tail, void *stream);

/* out[c] = sum_m X[m*ld + c] in f32 (bias gradients); deterministic two-stage reduction.
 * workspace: cum_colsum_workspace_elems() f32 elements. */
int64_t cum_colsum_workspace_elems(int64_t M, int32_t n_cols);
int cum_colsum(int32_t dtype, int64_t M, int32_t n_cols, const void *X, int64_t ld, float *out,
               float *workspace, void *stream);

/* Weight gradient of any of the layers above, with the bias gradient fused:
 *   dW[n*ldw + k] = sum_m dZ[m*ldz + n] * X[m*ldx + k]   (n < N, k < K),   db[n] = sum_m dZ[m*ldz + n]
 * X rows may overlap (ldx < K) as in cum_gemm_nt.  dW, db are f32 and fully overwritten; db may
 * be NULL.  The m axis is split over workgroups and combined deterministically.
 * workspace: cum_gemm_tn_workspace_elems() f32 elements. */
int64_t cum_gemm_tn_workspace_elems(int32_t dtype, int64_t M, int32_t N, int32_t K);
int cum_gemm_tn(int32_t dtype, int64_t M, int32_t N, int32_t K, const void *dZ, int64_t ldz,
                const void *X, int64_t ldx, float *dW, int64_t ldw, float *db, float *workspace,
                void *stream);
/* Kernel cum_gemm_tn runs for this problem: 256 (ping-pong kernel, 256 x 256 tiles), 384 (streaming kernel: the whole
 * 128 x 256 / 256 x 128 result per workgroup) or 128 (128 x 128 tiles). */
int cum_gemm_tn_tile(int32_t dtype, int64_t M, int32_t N, int32_t K);

/* ---- multi-resolution STFT loss around rocFFT (src/util/stft_loss.py:16-184) -------------------------------------
 * One resolution = (n_fft, hop, win_length, window[win_length]); torch.stft(center=True, reflect) framing:
 * n_frames = 1 + len / hop, bins = n_fft / 2 + 1.  The caller runs the batched r2c / c2r (rocFFT) in between.
 *
 * cum_stft_frames: frames[b][f][n] = window[n - (n_fft - win_length)/2] * x_reflect[b][f*hop + n]  (:29-33)
 * cum_stft_loss_fwd: spec_x / spec_y are (batch, n_frames, bins) interleaved complex f32.  With
 *   X = sqrt(max(re^2 + im^2, 1e-7)) (:38) over frames >= frame0 (band == "high" keeps frames >= n_frames / 2, :117-119):
 *   stats = { |Y - X|_F / |Y|_F (:59),  mean |log Y - log X| (:80),  |Y - X|_F,  |Y|_F }.
 * cum_stft_loss_bwd: zspec = d(g_sc * stats[0] + g_mag * stats[1]) / d spec_x with interior bins halved, so that an
 *   unnormalised c2r (irfft(norm="forward")) of zspec is the gradient wrt the real frames.  g_sc, g_mag: device scalars.
 * cum_stft_fold: dx[b][m] (+)= sum of window * dframes over every frame position that reads sample m (incl. reflections). */
int cum_stft_frames(const float *x, int64_t batch, int64_t len, int64_t x_stride_b, int32_t n_fft, int32_t hop,
                    int32_t win_length, const float *window, float *frames, int64_t n_frames, void *stream);
int64_t cum_stft_loss_workspace_elems(int64_t batch, int64_t n_frames);
int cum_stft_loss_fwd(const float *spec_x, const float *spec_y, int64_t batch, int64_t n_frames, int32_t bins,
                      int64_t frame0, float *workspace, float *stats, void *stream);
int cum_stft_loss_bwd(const float *spec_x, const float *spec_y, int64_t batch, int64_t n_frames, int32_t bins,
                      int64_t frame0, const float *stats, const float *g_sc, const float *g_mag, float *zspec,
                      void *stream);
int cum_stft_fold(const float *dframes, int64_t batch, int64_t len, int32_t n_fft, int32_t hop, int32_t win_length,
                  const float *window, int64_t n_frames, float *dx, int64_t dx_stride_b, int32_t accumulate,
                  void *stream);

/* ---- operand packing: dst[i] = idx[i] < 0 ? 0 : (dst_dtype) src[idx[i]], i < n.  The GEMM operand layouts above are
 * index permutations (with zero padding) of the reference's parameter tensors (encoder/decoder state-dict keys,
 * src/network/CleanUMamba.py:108-130); the same call unpacks weight gradients into parameter layout. */
int cum_gather(int32_t src_dtype, const void *src, const int32_t *idx, int64_t n, int32_t dst_dtype, void *dst,
               void *stream);

/* cum_pack2d: the same re-pack without a per-element index, for layouts that separate into dst[r][c] =
 * src[rowoff[r] + coloff[c]] (all weight layouts of the conv stack and the projections: network/convstack.py PackPlan).
 * jobs: device array of { int64 dst_off; int32 rows, cols (multiple of 8), row_tab, col_tab, transpose, runs8 } -- dst_off
 * in elements (multiple of 8) from `dst`, row_tab / col_tab positions in `tables` (int32, INT32_MIN = zero padding),
 * transpose = 1 when the source is fast along destination rows (the 64 x 64 tile then goes through LDS); runs8 (only
 * read when transpose = 0): 0 = no promise; 1 = every aligned group of 8 destination columns is all padding or 8
 * consecutive source elements (one table entry and one run per group instead of eight gathers); 2 = and every run starts
 * at a multiple of 4 elements from `src` (16-byte loads).
 * tiles: device array of n_tiles x { job, tile row, tile column }.  src: f32, 16-byte aligned. */
int cum_pack2d(const float *src, const void *jobs, const int32_t *tiles, int32_t n_tiles, const int32_t *tables,
               int32_t dst_dtype, void *dst, void *stream);

/* Batched 1-D FFTs for the STFT loss, on hipFFT / rocFFT (torch.stft's transform, src/util/stft_loss.py:29-33, and its
 * autograd).  Unnormalised in both directions.  The library keeps NO plan cache and allocates NO device memory for a
 * transform: a plan is an object the caller creates once per (kind, n, batch), keeps, and destroys; its work area is
 * caller memory passed to every cum_fft_exec (size returned by cum_fft_plan_create; may be 0).
 *   kind 0: real -> complex, in [batch][n] real, out [batch][n/2+1] interleaved complex;
 *   kind 1: complex -> real, in [batch][n/2+1] complex, out [batch][n] real;
 *   kind 2: complex -> complex, [batch][n] interleaved complex, `inverse` selects the direction, in == out allowed.
 * The INPUT of the real transforms may be overwritten (rocFFT does that for some lengths): pass scratch.
 * A plan is not re-entrant (one stream / one thread at a time); cum_fft_exec is graph-capturable. */
int cum_fft_plan_create(int32_t kind, int32_t n, int64_t batch, void **plan, int64_t *work_bytes);
int cum_fft_plan_destroy(void *plan);
int cum_fft_exec(void *plan, float *in, float *out, int32_t inverse, void *work, void *stream);

/* The same loss on PACKED transforms: a frame's n_fft real samples are read as n_fft/2 complex numbers
 * (even samples real, odd imaginary) and transformed by a kind-2 plan (cum_fft_exec); zx / zy: [batch * n_frames][n_fft / 2] complex.  The
 * real-input spectrum X[k], k = 0..n_fft/2, is recovered inside the kernels (twiddle: [n_fft/2 + 1] complex,
 * e^{-2 pi i k / n_fft}).  cum_stft_loss_bwd_packed writes gz = dL/dRe(Z) + i dL/dIm(Z); an unnormalised inverse
 * complex transform of gz is the gradient wrt the frames (what cum_stft_fold takes).  Replaces rocFFT's r2c post- / c2r
 * pre-processing passes. */
int cum_stft_loss_fwd_packed(const float *zx, const float *zy, int64_t batch, int64_t n_frames, int32_t n_fft,
                             int64_t frame0, const float *twiddle, float *workspace, float *stats, void *stream);
int cum_stft_loss_bwd_packed(const float *zx, const float *zy, int64_t batch, int64_t n_frames, int32_t n_fft,
                             int64_t frame0, const float *stats, const float *g_sc, const float *g_mag,
                             const float *twiddle, float *gz, void *stream);

/* The same loss with framing, both transforms and the loss terms in ONE kernel per direction (n_fft 512 / 1024 / 2048:
 * cum_stft_fused_supported): a wave reads a frame's samples of x and y from the waveforms, transforms both in LDS
 * (n_fft / 2 packed complex points, in-place radix-4, spectrum consumed in digit-reversed order) and accumulates the
 * loss partial sums -- no frame and no spectrum reaches HBM.  The backward rebuilds the two transforms, forms the gradient
 * spectrum in place, inverts it in LDS and writes the frame gradient over the window's support only, which is what
 * cum_stft_fold reads (dframes [batch][n_frames][n_fft], elements outside the support are left untouched).
 * x, y: [batch][len] f32 with row strides x_stride_b / y_stride_b (any; 8-byte aligned frames load in pairs); window [win_length];
 * twiddle [n_fft/2 + 1] complex e^{-2 pi i k / n_fft}; frame0 / stats / g_sc / g_mag as above.
 * workspace: cum_stft_fused_workspace_elems() f32.  Same values as the rocFFT path up to f32 rounding of the transform. */
int cum_stft_fused_supported(int32_t n_fft);
int64_t cum_stft_fused_workspace_elems(int64_t batch, int64_t n_frames);
int cum_stft_fused_fwd(const float *x, const float *y, int64_t batch, int64_t len, int64_t x_stride_b,
                       int64_t y_stride_b, int32_t n_fft, int32_t hop, int32_t win_length, const float *window,
                       const float *twiddle, int64_t n_frames, int64_t frame0, float *workspace, float *stats,
                       void *stream);
int cum_stft_fused_bwd(const float *x, const float *y, int64_t batch, int64_t len, int64_t x_stride_b,
                       int64_t y_stride_b, int32_t n_fft, int32_t hop, int32_t win_length, const float *window,
                       const float *twiddle, int64_t n_frames, int64_t frame0, const float *stats,
                       const float *g_sc, const float *g_mag, float *dframes, void *stream);

/* ---- residual add + LayerNorm of the Mamba blocks (mamba-ssm Block.forward with fused_add_norm=False as the reference
 * runs it, src/network/CleanUMamba.py:156-189, 288-294, and the final add + norm_f, :292-294):
 *   residual_out = x + residual (fp32);   y = (residual_out - mean) * rstd * weight + bias
 * x: (batch, len, dim) of x_dtype with element strides (x_sb, x_sl, 1); residual: contiguous fp32 or NULL;
 * y: contiguous, y_dtype; mean, rstd: fp32 [batch*len] (saved for the backward).  1 <= dim <= 2048: 16-byte vector
 * kernels when dim and the hidden strides are multiples of 8, element-access kernels otherwise (pruned checkpoints'
 * d_model 55, 114, 477 ...).
 * Backward: dy (y_dtype) and dres_out (fp32 or NULL, the gradient arriving at residual_out) ->
 *   dx = d(x) = d(residual) written as fp32 (dx32, may be NULL) and/or in h_dtype (dxh, may be NULL);
 *   dweight, dbias (dbias may be NULL): fully overwritten.  workspace: cum_add_layernorm_bwd_workspace_elems(dim) fp32. */
int cum_add_layernorm_fwd(int32_t x_dtype, int32_t y_dtype, int64_t batch, int32_t len, int32_t dim, const void *x,
                          int64_t x_sb, int64_t x_sl, const float *residual, const float *weight, const float *bias,
                          float eps, float *residual_out, void *y, float *mean, float *rstd, void *stream);
int64_t cum_add_layernorm_bwd_workspace_elems(int32_t dim);
int cum_add_layernorm_bwd(int32_t y_dtype, int32_t h_dtype, int64_t rows, int32_t dim, const void *dy,
                          const float *dres_out, const float *residual_out, const float *mean, const float *rstd,
                          const float *weight, float *dx32, void *dxh, float *dweight, float *dbias, float *workspace,
                          void *stream);

/* ---- one Mamba block for one token of every stream in ONE launch (Block.forward + Mamba.step of the streaming path,
 * src/network/CleanUMamba.py:451-454): residual_out = hidden_in (+ residual_in); h = LayerNorm(residual_out);
 * xz = in_proj h; x = silu(conv_update(x)); (dt, B, C) = x_proj x; dt = softplus(dt_proj dt + dt_bias);
 * state = exp(dt A) state + dt B x; y = (C . state + D x) silu(z); hidden_out = out_proj y.  All tensors f32 and
 * contiguous: hidden / residual [streams][d_model], conv_state [streams][d_inner][d_conv] and ssm_state
 * [streams][d_inner][d_state] updated in place, A = -exp(A_log) [d_inner][d_state].  Optional (NULL): residual_in,
 * norm_b, in_proj_b, conv_b, dt_proj_b, D, out_proj_b.  For small (pruned) models: every stream's workgroup re-reads
 * the projection matrices from L2 -- cum_mamba_step_supported() tells whether the sizes qualify. */
int cum_mamba_step_supported(int32_t d_model, int32_t d_inner, int32_t d_state, int32_t dt_rank, int32_t d_conv);
int cum_mamba_step(int32_t streams, int32_t d_model, int32_t d_inner, int32_t d_state, int32_t dt_rank, int32_t d_conv,
                   float eps, const float *hidden_in, const float *residual_in, const float *norm_w,
                   const float *norm_b, const float *in_proj_w, const float *in_proj_b, float *conv_state,
                   const float *conv_w, const float *conv_b, const float *x_proj_w, const float *dt_proj_w,
                   const float *dt_proj_b, const float *A, const float *D, float *ssm_state, const float *out_proj_w,
                   const float *out_proj_b, float *hidden_out, float *residual_out, void *stream);

/* out[s][j] = bias[j] + sum_k W[j*cols + k] * x[s*x_stride + k], f32, one workgroup per row s: the 1x1 bottleneck
 * convolutions of a streaming hop (tsfm_conv1 / tsfm_conv2 on one-column inputs, src/network/CleanUMamba.py:277,310).
 * cols <= 1024; bias may be NULL. */
int cum_small_linear(int32_t streams, int32_t rows, int32_t cols, const float *x, int64_t x_stride, const float *W,
                     const float *bias, float *out, int64_t out_stride, void *stream);

/* ---- streaming decoder glue (CleanUMamba._denoise_frame, src/network/CleanUMamba.py:476-488): overlap-add of a frame's
 * transposed-conv output with the previous frame's tail, activation, skip add and tail update for S streams in
 * lock-step, channels-last rows of Cp (C real channels):
 *   out[s][t]  = act(y[s][t] + (t < 2 ? tail[s][t] : 0)) + skip[s][t]      t < L2
 *   tail[s][t] = y[s][L2 + t] - bias                                          t < 2
 * y, skip, out: stream s starts y_pitch / skip_pitch / out_pitch rows after stream s-1; tail: [S][2][Cp]. */
/* Streaming encoder window of one layer (per-layer caches of _denoise_frame, :425-447): for every stream drop the n_new
 * oldest of `rows` rows and append n_new rows of `fresh`: window row t >= rows - n_new takes fresh row t - fresh_row0
 * (fresh_row0 = 0: `fresh` is a whole recomputed window; fresh_row0 = rows - n_new: `fresh` holds only the new rows).
 * window / fresh: stream s starts `pitch` / `fresh_pitch` rows after stream s-1 (fresh must not alias window).  One
 * in-place launch when rows - n_new <= 2048 and rows are 16-byte aligned; other windows go through tmp (streams * rows * Cp elements, else
 * it may be NULL).  tail_dst (optional, in-place path only): also receives the n_new + 2 newest rows of the updated
 * window, stream s at row s * tail_pitch -- what cum_stream_tail_rows would copy for the next layer. */
int cum_stream_window_update(int32_t dtype, int32_t streams, int32_t rows, int32_t n_new, int32_t Cp, void *window,
                             const void *fresh, int64_t pitch, int64_t fresh_pitch, int32_t fresh_row0, void *tmp,
                             void *tail_dst, int64_t tail_pitch, void *stream);
/* Input of the next layer's incremental step: dst[s][t] = src[s][src_row0 + t] for t < rows (the newest rows of a
 * window: 2 carried rows + the hop's new rows); rows of dst beyond `rows` are not touched (they stay zero). */
int cum_stream_tail_rows(int32_t dtype, int32_t streams, int32_t rows, int32_t Cp, const void *src, int64_t src_pitch,
                         int32_t src_row0, void *dst, int64_t dst_pitch, void *stream);
int cum_stream_overlap_add(int32_t dtype, int32_t streams, int32_t L2, int32_t Cp, int32_t C, const void *y,
                           int64_t y_pitch, void *tail, const float *bias, const void *skip, int64_t skip_pitch,
                           void *out, int64_t out_pitch, int32_t relu, void *stream);

/* ---- the whole streaming hop in ONE launch (csrc/hop.hip): CleanUMamba.feed / _denoise_frame of
 * src/network/CleanUMamba.py:370-490 (running input std :399-401, encoder caches :425-447, Mamba.step :451-454, decoder
 * overlap-add :476-488, with the skip order fixed as SURVEY fact 9 describes) for `n_hops` consecutive hops of `streams`
 * concurrent streams; a workgroup owns one stream, activations stay in LDS, f32 throughout (exact-f32 matrix cores).
 *   plan     device int32[cum_stream_hop_plan_ints()]: sizes, LDS regions, offsets into `weights` and into a stream's
 *            state block, in the field order of csrc/hop.hip::HopPlan (built by cleanumamba_amd/network/hopplan.py):
 *            a 16-int header, the op list (24 ints per op), per op and wave the position and length of the wave's stage
 *            list, and the stage lists of the matrix products (4 ints per stage: blob offset, LDS operand offset, chunk
 *            count | first | last flags, destination) -- the kernel walks what the host compiled, it derives nothing
 *   weights  device f32 blob: every matrix zero-padded and in MFMA fragment order ([tile][16-deep k chunk][lane][4]),
 *            biases / LayerNorm parameters / -exp(A_log) / D padded to the pitches the plan names
 *   state    device f32 [streams][state_stride]: encoder rings, decoder tails, conv / SSM states, running std, ring phase
 *   in       stream s, hop h reads the frame in[s * in_stride + h * hop_len ...+ frame_len) (raw samples)
 *   out      stream s, hop h writes out[s * out_stride + h * hop_len ...+ hop_len)
 *   lds_bytes dynamic LDS the plan needs (<= cum_stream_hop_max_lds_bytes(), multiple of 16)
 * The first frame of a stream (whole windows, no history) is the per-layer path's; its state is converted once. */
int cum_stream_hop_plan_ints(void);
int cum_stream_hop_max_lds_bytes(void);
int cum_stream_hop(const void *plan, const float *weights, float *state, int64_t state_stride, int32_t streams,
                   const float *in, int64_t in_stride, float *out, int64_t out_stride, int32_t n_hops,
                   int32_t lds_bytes, void *stream);

/* ---- the stream pool (csrc/hop.hip; cleanumamba_amd/network/streampool.py): streams that join and leave on their own.
 * Replaces, for any subset of a fixed set of slots, what CleanUMamba.feed of src/network/CleanUMamba.py:370-418 does for
 * one stream (its pending buffer, running std and per-layer state), with the hops of all named slots in ONE launch.
 * cum_stream_hop_slots: the interpreter of cum_stream_hop over an ITEM TABLE instead of `streams` x `n_hops`: n_items
 * workgroups, record i = 8 int32 {slot, n_hops, in_row, in_col, out_row, out_col, 0, 0}: the workgroup runs n_hops
 * hops of the stream whose state is row `slot` of `state` (capacity rows), reading hop h's frame at
 * in[in_row * in_stride + in_col + h * hop_len ...+ frame_len) and writing out[out_row * out_stride + out_col + h * hop_len
 * ...+ hop_len).  `items` is the device table, `items_host` the same table in host memory: the entry point checks every
 * record (0 <= slot < capacity, n_hops >= 1, no negative row or column) before the launch.  A slot named twice in one
 * table is a race the caller excludes.  Plan, weights, LDS rules: as cum_stream_hop. */
int cum_stream_hop_slots(const void *plan, const float *weights, float *state, int64_t state_stride, int32_t capacity,
                         const int32_t *items_host, const int32_t *items, int32_t n_items, const float *in,
                         int64_t in_stride, float *out, int64_t out_stride, int32_t lds_bytes, void *stream);
/* Input rows of a pool call and the slots' unconsumed samples.  hist: [capacity][hist_stride] f32, slot s keeps its
 * pending samples at hist[s][0, pend).  Record r = 8 int32 {slot, pend, len, consumed, x_row, stage_row, 0, 0}:
 *   stage[stage_row][0, pend + len) = hist[slot][0, pend) ++ x[x_row][0, len)
 *   hist[slot][0, pend + len - consumed) = stage[stage_row][consumed, pend + len)
 * One launch for all records (recs: device table, recs_host: the same in host memory, checked: slot < capacity, the
 * rows fit hist_stride / stage_stride).  Slots not named are not touched. */
int cum_stream_pool_stage(float *hist, int64_t hist_stride, int32_t capacity, const int32_t *recs_host,
                          const int32_t *recs, int32_t n_recs, const float *x, int64_t x_stride, float *stage,
                          int64_t stage_stride, void *stream);
/* Slot-row mover of the per-layer pool (csrc/slotstate.hip; cleanumamba_amd/network/layerpool.py): the state that
 * CleanUMamba.feed / _denoise_frame of src/network/CleanUMamba.py:358-490 keep for ONE stream in Python attributes lives
 * per slot in one row of store [capacity][state_stride] f32; a dense batch of the per-layer hop holds stream j at
 * `dense + j * pitch`.  direction 0 gathers (store -> dense), 1 scatters (dense -> store); ONE launch moves every segment
 * of every named slot.  slots: n slot ids (stream j of the batch is slot slots[j]).  segs: n_segs records of 4 int64
 * {dense base pointer (row 1 of a row buffer), dense per-stream pitch in bytes, offset in the store row in bytes, length
 * in bytes}.  clears (gathers only): n_clears records of 4 int64 {base pointer of a dense row buffer, bytes to clear at
 * its start, byte offset of the second range, its bytes}: the leading row and the slack rows behind stream n - 1.
 * Every table is passed twice, as the device copy the kernel reads and as a host copy the entry point checks BEFORE the
 * launch: a slot outside [0, capacity), a slot named twice, a segment that overruns the store row, segments that overlap
 * in the store row, null pointers, and sizes that are not multiples of 4 bytes are refused (CUM_EINVAL).  Segments whose
 * base, pitch and offset are multiples of 16 (and a 16-byte aligned store and row) move as 16-byte vectors, the rest as
 * dwords; at most 256 segments.  Slots not named and store bytes outside every segment are not touched.  A gather with
 * n = 0 only clears. */
int cum_stream_slots_move(int32_t direction, float *store, int64_t state_stride, int32_t capacity,
                          const int32_t *slots_host, const int32_t *slots, int32_t n, const int64_t *segs_host,
                          const int64_t *segs, int32_t n_segs, const int64_t *clears_host, const int64_t *clears,
                          int32_t n_clears, void *stream);

/* ---- first encoder layer, fused (csrc/enc0.hip): Conv1d(1 -> 64, k 4, s 2) + ReLU + Conv1d(64 -> 128, 1x1) + GLU of
 * src/network/CleanUMamba.py:108-113 at channels_input = 1, channels_H = 64 (E6 / E8), 16-bit element types.  The ReLU
 * output of the one-input-channel conv is rebuilt from the four input samples wherever it is needed instead of being
 * stored: forward and backward each move the layer's output-sized tensors once.
 *   xin      the layer's input row buffer [1 + 2 M + >= 2][8] (column 0 = sample, as cum_frame_rows writes it)
 *   w1, b1   the conv's parameters as stored: (64, 1, 4) and (64) f32
 *   w2p, b2p the 1x1 conv in the forward GEMM's packed operand order: [128][64] element type / [128] f32, per 32 rows
 *            16 a-rows then the 16 b-rows of the same channels
 *   M rows = clips x pitch; rows with (m mod pitch) >= valid are the zero rows between clips
 * cum_enc0_fwd: out = row buffer [1 + M + slack][64] (row 0 and zero_tail elements behind row M are cleared), gate
 *   [M][64] = the GLU's gate pre-activations for the backward (NULL: not kept).
 * cum_enc0_bwd: dZ [M][128] (gradient wrt the 1x1 conv's output, packed column order) -> slot_w2 = dW2 [128][64] then
 *   db2 [128], slot_w1 = dW1 [64][32] (element (h, 8 k) = tap k, other columns 0) then db1 [64]: the layouts
 *   cum_gemm_tn writes for these two layers.  workspace: cum_enc0_bwd_workspace_elems(M) f32.  Deterministic (slabs
 *   per workgroup, fixed-order sum).  The layer has no input gradient. */
int cum_enc0_fwd(int32_t dtype, int64_t M, int32_t pitch, int32_t valid, const void *xin, const float *w1,
                 const float *b1, const void *w2p, const float *b2p, void *out, int64_t zero_tail, void *gate,
                 void *stream);
int32_t cum_enc0_bwd_workgroups(int64_t M);
int64_t cum_enc0_bwd_workspace_elems(int64_t M);
int cum_enc0_bwd(int32_t dtype, int64_t M, int32_t pitch, int32_t valid, const void *dZ, const void *xin,
                 const float *w1, const float *b1, const void *w2p, float *slot_w2, float *slot_w1, float *workspace,
                 void *stream);

/* An encoder layer of width 128, forward, fused:  Conv1d(64 -> 128, k 4, s 2) + ReLU + Conv1d(128 -> 256, 1x1) + GLU of
 * src/network/CleanUMamba.py:108-113 at channels_H = 64 (the second encoder layer of E6 / E8), 16-bit element types, one
 * launch instead of cum_gemm_nt (EPI_RELU) + cum_gemm_nt (EPI_GLU); it writes what those two write, so the backward is
 * theirs (csrc/ench.hip).
 *   xin      row 1 of the input row buffer [..][64]: output row m reads input rows 2 m .. 2 m + 3; x_rows = rows readable
 *            from xin (>= 2 M + 2)
 *   w1p/b1p  conv weight packed [128][256] (column tap * 64 + channel: lay_conv_fwd) and bias [128] f32
 *   w2p/b2p  1x1 weight packed [256][128] (rows 32 g + i: i < 16 value channel 16 g + i, else gate channel: lay_glu_fwd),
 *            bias [256] f32 in the same row order
 *   y1       row 1 of the hidden row buffer [..][128] (ReLU output; the 128 elements before it and y1_tail elements behind
 *            row M are cleared) or NULL (inference: not stored); bits: its sign nibbles, one byte per four channels,
 *            32 bytes per row (NULL: not kept)
 *   out      row 1 of the output row buffer [..][128] (framing cleared as for y1); gate: [M][128] gate pre-activations for
 *            the backward or NULL
 *   M rows = clips x pitch; rows with (m mod pitch) >= valid are zero rows of y1 / out. */
int cum_ench_fwd(int32_t dtype, int64_t M, int32_t pitch, int32_t valid, const void *xin, int64_t x_rows,
                 const void *w1p, const float *b1p, const void *w2p, const float *b2p, void *y1, int64_t y1_tail,
                 void *bits, void *out, int64_t out_tail, void *gate, void *stream);

/* A decoder layer of width 128, forward, fused:  Conv1d(128 -> 256, 1x1) + GLU + ConvTranspose1d(128 -> 64, k 4, s 2) +
 * ReLU (+ the next layer's skip connection) of src/network/CleanUMamba.py:121-130, 313-316 at channels_H = 64 (the
 * second-to-last decoder layer of E6 / E8), 16-bit element types, one launch instead of cum_gemm_nt (EPI_GLU) +
 * cum_gemm_nt (EPI_RELU with residual and sign nibbles); it writes what those two write (csrc/dech.hip).
 *   u        row 0 (the leading zero row) of the input row buffer [..][128]; u_rows = rows readable from it
 *   w1p/b1p  1x1 weight packed [256][128] (lay_glu_fwd) and bias [256] f32 in the same row order
 *   wtp/btp  transposed-conv weight packed [128 = (output-row parity, 64 channels)][256 = (row m - 1 | row m, 128
 *            channels)] (lay_convt_fwd) and bias [128] f32 (the 64 biases twice)
 *   skip     row 1 of the skip row buffer [..][64] (added after the ReLU) or NULL
 *   g        row 0 of the GLU-output row buffer [..][128] (row 0 and g_tail elements behind row M are cleared) with its gate
 *            pre-activations gate [M][128], or both NULL (inference: not stored)
 *   out      row 1 of the output row buffer [..][64] (GEMM row m = output rows 2 m, 2 m + 1; the 64 elements before it and
 *            out_tail elements behind output row 2 M are cleared); bits: sign nibbles of the ReLU, 32 bytes per GEMM row
 *            (NULL: not kept)
 *   M input rows = clips x pitch; data row d is real iff (d mod pitch) < valid. */
int cum_dech_fwd(int32_t dtype, int64_t M, int32_t pitch, int32_t valid, const void *u, int64_t u_rows,
                 const void *w1p, const float *b1p, const void *wtp, const float *btp, const void *skip, void *g,
                 int64_t g_tail, void *gate, void *out, int64_t out_tail, void *bits, void *stream);

/* The last decoder layer, fused:  Conv1d(64 -> 128, 1x1) + GLU + ConvTranspose1d(64 -> 1, k 4, s 2) of
 * src/network/CleanUMamba.py:121-130 at channels_output = 1, channels_H = 64 (E6 / E8), 16-bit element types.  The GLU
 * output is rebuilt from the layer input wherever it is needed instead of being stored.
 *   u        the layer's input row buffer [1 + M + slack][64]; M rows = clips x pitch, rows with (m mod pitch) >= valid
 *            are the zero rows between clips; pair row p <= valid of a clip produces output rows 2 p, 2 p + 1
 *   w1p, b1p the 1x1 conv in the forward GEMM's packed operand order ([128][64] element type / [128] f32, per 32 rows
 *            16 a-rows then the 16 b-rows of the same channels); wt (64, 1, 4), bt (1): the transposed conv as stored, f32
 * cum_dec7_fwd: out = output row buffer [1 + 2 M + slack][8] (channel 0 = the signal, channels 1-7 zero; row 0 and
 *   zero_tail elements behind row 2 M are cleared).
 * cum_dec7_bwd: dY = gradient of that buffer (channel 0 is read), mask = sign bits of the ReLU of the layer below as
 *   cum_gemm_nt writes them (16 bytes per row, data row 0 first) -> dU = gradient of u, dpre = dU where the bit is set
 *   (row buffers [1 + M + slack][64]; row 0 and zero_tail elements behind row M cleared), slot_w1 = dW1 [128][64] then
 *   db1 [128], slot_wt = dW [16][128] then db [16]: the layouts cum_gemm_tn writes for the 1x1 and for the transposed
 *   conv taken as a GEMM (N = output-row parity x 8 channels, K = (row m - 1 | row m) x 64 channels).
 *   workspace: cum_dec7_bwd_workspace_elems(M) f32.  Deterministic (slabs per workgroup, added in index order). */
int cum_dec7_fwd(int32_t dtype, int64_t M, int32_t pitch, int32_t valid, const void *u, const void *w1p, const float *b1p,
                 const float *wt, const float *bt, void *out, int64_t zero_tail, void *stream);
int32_t cum_dec7_bwd_workgroups(int64_t M);
int64_t cum_dec7_bwd_workspace_elems(int64_t M);
int cum_dec7_bwd(int32_t dtype, int64_t M, int32_t pitch, int32_t valid, const void *dY, const void *u, const void *mask,
                 const void *w1p, const float *b1p, const float *wt, void *dU, void *dpre, int64_t zero_tail,
                 float *slot_w1, float *slot_wt, float *workspace, void *stream);

/* ---- waveform ends of the train step (csrc/loss.hip).  All sums are per-workgroup partials in fixed order + one
 * finishing workgroup: deterministic, graph-capturable, nothing returns to the host.
 *
 * cum_lp_loss_fwd / _bwd: the time-domain term of loss_fn, F.l1_loss (p = 1) / F.mse_loss (p = 2) of (denoised, clean)
 * with reduction "mean" (src/util/util.py:262-268).  y, c, dy: n contiguous f32; partials: cum_lp_loss_parts(n) f32;
 * out: 1 f32; gout: 1 f32 in device memory (the incoming gradient of the scalar).  dy = gout * sign(y - c) / n (p = 1;
 * 0 where y == c, as torch) or gout * 2 (y - c) / n (p = 2). */
int32_t cum_lp_loss_parts(int64_t n);
int cum_lp_loss_fwd(int32_t p, const float *y, const float *c, int64_t n, float *partials, float *out, void *stream);
int cum_lp_loss_bwd(int32_t p, const float *y, const float *c, int64_t n, const float *gout, float *dy, void *stream);

/* cum_clip_std: out[r] = unbiased std of row r of x (rows x len f32, row stride `stride` elements) + eps -- the per-clip
 * input normalisation `noisy_audio.std(dim=2, keepdim=True) + 1e-3` (src/network/CleanUMamba.py:260-262).  One pass
 * (Welford per thread, Chan merges in fixed order).  partials: 3 * rows * cum_clip_std_parts(len) f32. */
int32_t cum_clip_std_parts(int64_t len);
int cum_clip_std(const float *x, int32_t rows, int64_t len, int64_t stride, float eps, float *partials, float *out,
                 void *stream);

/* cum_frame_rows: (batch, len) f32 signal -> the channels-last row buffer of a ONE-channel activation (8 columns per
 * row: column 0 the sample, 1-7 zero; row 0 zero; per clip T rows + 2 zero rows; total_rows rows written in all):
 * out = x / scale[b] (invert = 1: `noisy / std` + pad_signal, src/network/CleanUMamba.py:262-264) or x * scale[b]
 * (invert = 0: the backward of cum_unframe_rows); steps len .. T-1 are zero; scale may be NULL (= 1).
 * cum_unframe_rows: y[b][t] = rows[1 + b (T + 2) + t][0] * scale[b], t < len: `x[:, :, :L] * std`
 * (src/network/CleanUMamba.py:319) read straight from the last transposed conv's row buffer. */
int cum_frame_rows(int32_t dtype, const float *x, int32_t batch, int64_t len, int64_t stride, int64_t T,
                   int64_t total_rows, const float *scale, int32_t invert, void *out, void *stream);
int cum_unframe_rows(int32_t dtype, const void *rows, int32_t batch, int64_t len, int64_t T, const float *scale,
                     float *y, void *stream);

/* ---- optimizer section of the train step on flat buffers (src/training/train.py:303-310: scaler.unscale_,
 * clip_grad_norm_(clip_grad_norm_max), scaler.step(Adam), scaler.update; Adam built at :145-148 with betas / eps /
 * weight_decay of configs/config.json, GradScaler at :158-160).  p, g, m, v: f32 buffers of n elements, 16-byte
 * aligned (all parameters of the model back to back; training/flat_optim.py).  `state`: cum_optim_state_elems() f32 in
 * device memory, zero-initialised by the caller except [3] = initial loss scale and [8] = learning rate (written by
 * the caller before every step):
 *   [0] total gradient norm (unscaled)  [1] multiplier applied to g (clip coefficient / loss scale)  [2] found inf/nan
 *   [3] loss scale  [4] growth tracker  [5] Adam step count  [6] 1 - beta1^t  [7] sqrt(1 - beta2^t)  [8] learning rate
 *   [9] skipped steps  [10] the loss scale the gradients of the last step carried (written by cum_optim_prepare
 *   before it updates [3]: what a reader of those gradients divides by after the step)
 * Sequence per optimizer step: cum_optim_sumsq (partials: cum_optim_sumsq_parts(n) f32) -> cum_optim_prepare ->
 * cum_optim_adam.  Nothing returns to the host; with found inf/nan the Adam launch leaves p, m, v untouched and the
 * loss scale backs off (torch.amp.GradScaler semantics: growth x `growth` after `growth_interval` clean steps).
 * max_norm <= 0 disables clipping; use_scaler = 0: gradients are unscaled, state[3] is ignored. */
int32_t cum_optim_state_elems(void);
int32_t cum_optim_sumsq_parts(int64_t n);
int cum_optim_sumsq(const float *g, int64_t n, float *partials, void *stream);
int cum_optim_prepare(float *state, const float *partials, int32_t nparts, float max_norm, double beta1, double beta2,
                      int32_t use_scaler, float growth, float backoff, int32_t growth_interval, void *stream);
int cum_optim_adam(float *p, const float *g, float *m, float *v, int64_t n, const float *state, double beta1,
                   double beta2, float eps, float weight_decay, void *stream);   /* betas as double: 1 - beta must not
                                                                                    be formed in f32 (0.999f: 5e-5 off) */

/* cum_optim_adam_groups: the update of cum_optim_adam with torch's parameter groups, in the same one launch -- what the
 * reference's optimizer choice needs (src/training/train.py:126-154: "adam" = torch.optim.Adam, L2 decay on every
 * tensor; "adamw" = torch.optim.AdamW over two groups, decoupled decay on the dim() >= 2 tensors and none on the rest).
 * Takes the third place of the sequence above; state, betas and eps as there (shared by all groups).
 *   decoupled    0: g += weight_decay_k * p (torch.optim.Adam; one group gives the bits of cum_optim_adam)
 *                1: p *= 1 - lr_k * weight_decay_k before the update (torch.optim.AdamW)
 *   group_hyper  device, 16-byte aligned, 4 f32 per group: {lr, weight_decay, 1 - lr * weight_decay rounded once from
 *                double, unused}.  state[8] is not read.  ngroups in [1, cum_optim_max_groups()].
 *   membership   per float4 of the flat buffers (every parameter starts on a 4-element boundary), in tiles of
 *                cum_optim_group_tile_elems() elements, T = max(1, ceil(ceil(n / 4) / (tile / 4))) of them:
 *                tile_group[T] (device i32): >= 0: the whole tile belongs to that group; < 0: -(value) - 1 is the first
 *                entry of the segment list that reaches into the tile.  seg_end[nseg] / seg_group[nseg] (device i32):
 *                segments in ascending order, exclusive end in float4 units and group; the last ends at ceil(n / 4).
 * With found inf/nan the launch changes nothing, the decay included.  Zero padding (p = g = m = v = 0) stays zero.
 * Null or misaligned pointers, n < 0 and ngroups outside its range are rejected (CUM_EINVAL) before any launch. */
int32_t cum_optim_group_tile_elems(void);
int32_t cum_optim_max_groups(void);
int cum_optim_adam_groups(float *p, const float *g, float *m, float *v, int64_t n, const float *state, double beta1,
                          double beta2, float eps, int32_t decoupled, const float *group_hyper, int32_t ngroups,
                          const int32_t *tile_group, const int32_t *seg_end, const int32_t *seg_group, int32_t nseg,
                          void *stream);

/* ---- Mamba2 bottleneck (mamba_v2=True; csrc/ssd.hip).  ngroups 1, headdim and dstate in {16, 32, 64}, any len, any
 * batch.  Per head h: dt_t = softplus(dt_raw_t + dt_bias_h), A_h = -exp(A_log_h),
 *   state_t = exp(dt_t A_h) state_{t-1} + dt_t x_t B_t^T   (headdim x dstate),   y_t = state_t C_t + D_h x_t.
 * x, y: rows of nheads * headdim elements; dt: rows of nheads; B, C: rows of dstate; row (b, t) of each starts at
 * b * *_sb + t * *_sl elements (elements within a row contiguous).  io_dtype is the element type of x, dt, B, C, y and
 * of their gradients; dt_bias, A_log, D, the states and the parameter gradients are f32.
 * cum_ssd_fwd      <- mamba_ssm.ops.triton.ssd_combined.mamba_chunk_scan_combined (z = None, dt_softplus, dt_bias, D
 *                     per head, no dt limit).  states: f32, cum_ssd_states_elems() (opaque: the chunk-start states the
 *                     backward reads, chunks of cum_ssd_chunk() steps); final_state: NULL or (batch, nheads, headdim,
 *                     dstate) contiguous.
 * cum_ssd_bwd      <- its backward.  dy has y's strides, dx x's, ddt dt's (d dt_raw: the softplus is included); dB / dC
 *                     are summed over heads in a fixed order; dA_log, dD, ddt_bias (nheads each) are overwritten.
 *                     workspace: f32, cum_ssd_bwd_workspace_elems().  No atomics: bitwise reproducible. */
typedef struct {
  int32_t batch, len, nheads, headdim, dstate;
  int64_t x_sb, x_sl, dt_sb, dt_sl, B_sb, B_sl, C_sb, C_sl, y_sb, y_sl;
  int32_t io_dtype;
} cum_ssd_shape;
int cum_ssd_chunk(void);
int64_t cum_ssd_states_elems(int32_t batch, int32_t len, int32_t nheads, int32_t headdim, int32_t dstate);
int64_t cum_ssd_bwd_workspace_elems(int32_t batch, int32_t len, int32_t nheads, int32_t headdim, int32_t dstate);
int cum_ssd_fwd(const cum_ssd_shape *s, const void *x, const void *dt, const float *dt_bias, const float *A_log,
                const float *D, const void *B, const void *C, void *y, float *states, float *final_state, void *stream);
int cum_ssd_bwd(const cum_ssd_shape *s, const void *x, const void *dt, const float *dt_bias, const float *A_log,
                const float *D, const void *B, const void *C, const void *dy, const float *states, void *dx, void *ddt,
                void *dB, int64_t dB_sb, int64_t dB_sl, void *dC, int64_t dC_sb, int64_t dC_sl, float *dA_log,
                float *dD, float *ddt_bias, float *workspace, void *stream);
/* cum_gated_rmsnorm_fwd/bwd <- mamba_ssm.ops.triton.layernorm_gated.RMSNormGated (norm_before_gate=False, one group):
 * out = y * silu(z) * rsqrt(mean((y * silu(z))^2) + eps) * w over rows of `dim` elements (row pitches in elements,
 * dtype for y, z, out, dout, dy, dz; w, rstd, dw f32).  rstd: NULL or one f32 per row, saved for the backward.
 * dw is overwritten (per-workgroup slabs + fixed-order reduce); workspace: cum_gated_rmsnorm_bwd_workspace_elems(). */
int cum_gated_rmsnorm_fwd(int32_t dtype, int64_t rows, int32_t dim, const void *y, int64_t y_ld, const void *z,
                          int64_t z_ld, const float *w, float eps, void *out, int64_t out_ld, float *rstd, void *stream);
int64_t cum_gated_rmsnorm_bwd_workspace_elems(int32_t dim);
int cum_gated_rmsnorm_bwd(int32_t dtype, int64_t rows, int32_t dim, const void *y, int64_t y_ld, const void *z,
                          int64_t z_ld, const float *w, const float *rstd, const void *dout, int64_t d_ld, void *dy,
                          int64_t dy_ld, void *dz, int64_t dz_ld, float *dw, float *workspace, void *stream);
/* cum_ssd_step <- Mamba2.step of mamba-ssm 2.x (causal_conv1d_update over xBC with SiLU, selective_state_update with a
 * scalar decay per head, RMSNormGated): one token of every stream, f32, one launch.  zxbcdt: the in_proj output rows
 * [z (d_ssm) | xBC (d_ssm + 2 dstate) | dt (nheads)], pitch ld; conv_state (streams, d_ssm + 2 dstate, width) and
 * ssm_state (streams, nheads, d_ssm / nheads, dstate) contiguous, updated in place; out: (streams, d_ssm) rows, the
 * gated-norm output that goes to out_proj. */
int cum_ssd_step(int32_t streams, int32_t d_ssm, int32_t nheads, int32_t dstate, int32_t width, float eps,
                 const float *zxbcdt, int64_t ld, float *conv_state, const float *conv_w, const float *conv_b,
                 const float *dt_bias, const float *A_log, const float *D, const float *norm_w, float *ssm_state,
                 float *out, int64_t out_ld, void *stream);

/* ---- speech-quality metrics of a ragged batch of int16 clips (src/util/python_eval.py, pystoi.stoi) ----------------
 * clean / processed: flat int16 buffers of n_samples, 16-byte aligned; clip i is [offsets[i], offsets[i] + lengths[i])
 * of both.  offsets and lengths are HOST arrays: every entry checks them before any launch (a clip outside the buffer, a
 * clip shorter than one window, an unsupported rate, an empty batch -> CUM_EINVAL) and uploads the clip table to the
 * head of `workspace` on `stream`, waiting for that copy (one stream synchronise per call).  All sums run in a fixed order within a clip's own workgroups: bit-reproducible, and
 * a clip's result does not depend on the rest of its batch. */
/* frames per clip of the 16 kHz frame metrics: (len - 480) / 120, the reference's int(len / 120 - 480 / 120); -1 below 480 */
int64_t cum_metrics_frame_count(int64_t len);
/* frames kept by the trimmed mean: Python's round(0.95 * n_frames), half to even (python_eval.py:88, :93) */
int64_t cum_metrics_reduce_keep(int64_t n_frames);
/* workspace of cum_metrics_frames and cum_metrics_clip_reduce */
int64_t cum_metrics_workspace_bytes(int64_t n_clips, int64_t n_frames_total);
/* cum_metrics_frames <- python_eval.py:409 snr (segmental part), :336 llr + :380 lpcoeff, :139 wss at 16 kHz.
 * Frame f of clip i goes to index frame_off(i) + f of seg_snr / llr / wss (f64), frame_off the running sum of
 * cum_metrics_frame_count; n_frames_total is their sum.  Tables (device): window[480] = 0.5 (1 - cos(2 pi n / 481)),
 * n = 1..480; band_tab[25][3] = (first bin, bin count, offset into band_w) of each critical band's truncated Gaussian;
 * tw[513] = e^{-2 pi i m / 1024} as (re, im) f64. */
int cum_metrics_frames(const int16_t *clean, const int16_t *processed, int64_t n_samples, const int64_t *offsets,
                       const int64_t *lengths, int64_t n_clips, int32_t rate, const double *window,
                       const int32_t *band_tab, const double *band_w, const double *tw, void *workspace,
                       int64_t workspace_bytes, double *seg_snr, double *llr, double *wss, int64_t n_frames_total,
                       void *stream);
/* cum_metrics_clip_reduce <- eval_waveform's per-clip reduces (python_eval.py:86-104): out[i] over clip i's frame values
 * (laid out as cum_metrics_frames writes them).  mode 0: mean (segSNR); 1: mean of the round(0.95 n) lowest, NaN
 * sorting last (wss_dist); 2: as 1 with the NaNs of that slice dropped (llr_mean).  An empty selection gives NaN. */
int cum_metrics_clip_reduce(const double *values, const int64_t *lengths, int64_t n_clips, int32_t mode, void *workspace,
                            int64_t workspace_bytes, double *out, void *stream);
/* workspace of cum_metrics_stoi (bytes); -1 for bad arguments */
int64_t cum_metrics_stoi_workspace_bytes(const int64_t *lengths, int64_t n_clips, int32_t rate);
/* cum_metrics_stoi <- pystoi.stoi(x, y, rate, extended=False) as python_eval.py:123 calls it; rate 16000 or 10000.
 * taps[n_taps]: the 16 k -> 10 k polyphase filter of pystoi's resample_oct, normalised and scaled by up = 5 (ignored at
 * 10 kHz); window[256] = hanning(258)[1:-1]; tw[257] = e^{-2 pi i m / 512} (f64 re, im); bands[15][2] = [first, end) bin
 * of each one-third-octave band.  out[i]: STOI of clip i (1e-5 below 30 STFT frames, as pystoi). */
int cum_metrics_stoi(const int16_t *clean, const int16_t *processed, int64_t n_samples, const int64_t *offsets,
                     const int64_t *lengths, int64_t n_clips, int32_t rate, const double *taps, int32_t n_taps,
                     const double *window, const double *tw, const int32_t *bands, void *workspace,
                     int64_t workspace_bytes, double *out, void *stream);
/* The extended metrics below restate published definitions (tests/metrics_ext_ref.py holds them in f64 numpy); none has
 * been compared with pystoi, pysepm or torchmetrics.  Same conventions as the entries above.
 * cum_metrics_stoi_ex <- pystoi.stoi(x, y, rate, extended=...): which & 1 writes STOI to out (the bits of
 * cum_metrics_stoi), which & 2 writes eSTOI (Jensen & Taal, IEEE/ACM TASLP 24(11), 2016) to out_e; the front end up to
 * the one-third-octave magnitudes runs once.  Per 30-frame segment both 15 x 30 matrices get zero-mean unit-norm rows,
 * then zero-mean unit-norm columns (every norm + eps; pystoi adds eps-sized noise instead), the value is sum(Xn Yn) / 30,
 * the clip's the mean over segments; 1e-5 below 30 STFT frames.  Workspace: cum_metrics_stoi_workspace_bytes. */
int cum_metrics_stoi_ex(const int16_t *clean, const int16_t *processed, int64_t n_samples, const int64_t *offsets,
                        const int64_t *lengths, int64_t n_clips, int32_t rate, const double *taps, int32_t n_taps,
                        const double *window, const double *tw, const int32_t *bands, void *workspace,
                        int64_t workspace_bytes, int32_t which, double *out, double *out_e, void *stream);
/* cum_metrics_frames_ext <- the two remaining measures of Hu & Loizou 2008 on cum_metrics_frames' frames, window, tables,
 * workspace and layout (16 kHz).  cep: (10 / ln 10) sqrt(2 sum_k (c_k - c'_k)^2) of the order-16 LPC cepstra
 * (c_1 = -a_1, c_k = -a_k - (1/k) sum_{i<k} i c_i a_{k-i}), limited to [0, 10], NaN where either frame is all zeros.
 * fwseg: |FFT_1024| of the frame / 32768 * window over bins 0..511, each spectrum divided by (its sum + eps), critical
 * band sums ce_b / pe_b of these magnitudes, sum_b W_b 10 log10(ce_b^2 / max((ce_b - pe_b)^2, eps)) / sum_b W_b with
 * W_b = ce_b^0.2 over the bands with ce_b > 0, limited to [-10, 35]; NaN where the clean frame is silent. */
int cum_metrics_frames_ext(const int16_t *clean, const int16_t *processed, int64_t n_samples, const int64_t *offsets,
                           const int64_t *lengths, int64_t n_clips, int32_t rate, const double *window,
                           const int32_t *band_tab, const double *band_w, const double *tw, void *workspace,
                           int64_t workspace_bytes, double *cep, double *fwseg, int64_t n_frames_total, void *stream);
/* cum_metrics_clip_nanmean: out[i] = mean of clip i's frame values that are not NaN (fwsegSNR), NaN if it has none;
 * layout and workspace as cum_metrics_clip_reduce (whose mode 2 is the clip reduce of cep). */
int cum_metrics_clip_nanmean(const double *values, const int64_t *lengths, int64_t n_clips, void *workspace,
                             int64_t workspace_bytes, double *out, void *stream);
/* cum_metrics_sums: out[i][3] = exact int64 (sum x^2, sum y^2, sum x y) of clip i; any rate, clips of >= 1 sample.  The
 * overall SNR 10 log10(Sxx / (Sxx - 2 Sxy + Syy)) and SI-SDR 10 log10(Sxy^2 / (Sxx Syy - Sxy^2)) (Le Roux et al., ICASSP
 * 2019, no mean removal) follow from them in exact integer arithmetic on the host.  Workspace (bytes; -1 for bad
 * arguments): cum_metrics_sums_workspace_bytes. */
int64_t cum_metrics_sums_workspace_bytes(const int64_t *lengths, int64_t n_clips);
int cum_metrics_sums(const int16_t *clean, const int16_t *processed, int64_t n_samples, const int64_t *offsets,
                     const int64_t *lengths, int64_t n_clips, void *workspace, int64_t workspace_bytes, int64_t *out,
                     void *stream);

/* ---- structured channel pruning (cleanumamba_amd/pruning/; reference src/pruning/pruninggroup.py, util.py:328-349) --
 * Both entries take HOST descriptor tables, check every descriptor before any launch (CUM_EINVAL, nothing launched),
 * upload the tables to the head of `workspace` on `stream` and wait for that copy (one stream synchronise per call).
 *
 * cum_prune_importance <- PruningModule.channel_importances for every descriptor in one launch.  Channel c of
 * descriptor d covers the elements
 *   off + c ch_stride + h head_stride + i0 s0 + i1 s1,   h < heads, i0 < n0, i1 < n1
 * of w and g (both laid out alike, numel elements; g NULL: no gradient, its sums are 0).  out: n_out rows of 5 f32,
 * row d.out + c = [sum w^2, sum g'^2, sum |w g'|, sum (w g')^2, |sum w g'|] with g' = g / scale[0] (scale: NULL = 1, else
 * one f32 in device memory: the loss scale the gradients carry).  Sums in f64, one wave per channel
 * (lanes_on_channels = 0: lanes over the channel's elements) or per 64 channels (1: lane = channel) in a fixed order:
 * bitwise reproducible.  A non-finite gradient gives non-finite sums (the caller checks). */
typedef struct {
  const float *w, *g;
  int64_t numel;
  int64_t off, ch_stride, head_stride, s0, s1;
  int32_t channels, heads, n0, n1;
  int64_t out;
  int32_t lanes_on_channels, pad_;
} cum_prune_imp_desc;
int64_t cum_prune_importance_workspace_bytes(const cum_prune_imp_desc *descs, int32_t n_desc);
int cum_prune_importance(const cum_prune_imp_desc *descs, int32_t n_desc, const float *scale, float *out, int64_t n_out,
                         void *workspace, int64_t workspace_bytes, void *stream);
/* cum_prune_gather <- prune_parameter_and_grad on flat buffers: for every parameter d, the row-major (ndim <= 3) tensor
 * of old_dims at element d.src of the four old buffers (parameters, gradients, exp_avg, exp_avg_sq; src_numel each)
 * -> its kept part, new_dims, at element d.dst of the four new buffers (dst_numel each):
 *   new[i0][i1][i2] = old[K0(i0)][K1(i1)][K2(i2)],  Kk = keep[d.keep[k] ...] (strictly increasing), or the identity
 *   when d.keep[k] < 0 (new_dims[k] == old_dims[k]).
 * d.dst multiple of 4 (16-byte aligned starts), destinations in increasing order and disjoint; the alignment padding
 * after each new parameter (up to the next multiple of 4) is written as zeros.  n_new = product of new_dims.  The four
 * moment pointers (src_m, src_v, dst_m, dst_v) are all NULL when there are no Adam moments to move: then only parameters
 * and gradients are gathered.  Plain copies: bit-exact. */
typedef struct {
  int64_t src, dst, n_new;
  int32_t ndim;
  int32_t old_dims[3], new_dims[3];
  int32_t pad_;
  int64_t keep[3];
} cum_prune_gather_desc;
int64_t cum_prune_gather_workspace_bytes(int32_t n_desc, int64_t n_keep);
int cum_prune_gather(const cum_prune_gather_desc *descs, int32_t n_desc, const int32_t *keep, int64_t n_keep,
                     const float *src_p, const float *src_g, const float *src_m, const float *src_v, int64_t src_numel,
                     float *dst_p, float *dst_g, float *dst_m, float *dst_v, int64_t dst_numel, void *workspace,
                     int64_t workspace_bytes, void *stream);
/* cum_prune_mask <- the trial prune of layer-wise calibration (src/pruning/layerwise_calibration.py:120-135) in place.
 * Descriptor d covers, for every listed row r = idx[d.first + j] (j < n_rows, strictly increasing, r < rows), the
 * elements  r row_stride + i0 s0 + i1 s1  (i0 < n0, i1 < n1)  of w (numel elements).  Saved values sit in `save`
 * descriptor after descriptor, n_rows n0 n1 each (cum_prune_mask_save_elems in all); rows_fastest only orders them
 * (1: consecutive values on consecutive listed rows).  restore = 0: save every covered element, then zero it;
 * restore = 1: write the saved values back (plain copies: bit-exact).  The same descriptors and indices go to both
 * calls.  No element may belong to two descriptors (checked: the tensors' [w, w + numel) ranges must be disjoint). */
typedef struct {
  float *w;
  int64_t numel;
  int64_t row_stride, s0, s1;
  int32_t n0, n1;
  int32_t rows, n_rows;
  int64_t first;
  int32_t rows_fastest, pad_;
} cum_prune_mask_desc;
int64_t cum_prune_mask_save_elems(const cum_prune_mask_desc *descs, int32_t n_desc);
int64_t cum_prune_mask_workspace_bytes(int32_t n_desc, int64_t n_idx);
int cum_prune_mask(const cum_prune_mask_desc *descs, int32_t n_desc, const int32_t *idx, int64_t n_idx, float *save,
                   int64_t n_save, int32_t restore, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- input end of the train step (csrc/pcm.hip) --------------------------------------------------------------------
 * cum_pcm_batch_f32 <- the int16 -> float scaling and the short-clip tiling of CleanNoisyPairDataset.__getitem__
 * (src/util/dataset.py:108-150) and the two batch uploads of the train loop (src/training/train.py:259-260): the
 * loader stages int16 crops and uploads them once; this launch writes the float batch where the step reads it.
 * pcm: device buffer of 2 * batch rows, `pitch` int16 apart; row b is clean clip b, row batch + b noisy clip b, and
 * only the first min(src_len[b], len) samples of a row are meaningful.  src_len: device i32[batch].
 *   clean[b clean_sb + t] = pcm[b][t mod n_b] 2^-15,  noisy[b noisy_sb + t] = pcm[batch + b][t mod n_b] 2^-15,  t < len
 * with n_b = src_len[b] clamped into [1, len] inside the kernel (a bad table never indexes outside a row).  The
 * results are exact (an int16 times 2^-15 is a float).  Rows with n_b == len move 16 bytes per lane and access.
 * batch < 1, len < 1, pitch < len, pitch % 8 != 0, clean_sb < len, noisy_sb < len, a null pointer, or pcm / clean /
 * noisy off a 16-byte boundary: CUM_EINVAL before any launch. */
int cum_pcm_batch_f32(const int16_t *pcm, int64_t pitch, const int32_t *src_len, int32_t batch, int64_t len,
                      float *clean, int64_t clean_sb, float *noisy, int64_t noisy_sb, void *stream);

/* ---- ragged inference batches (csrc/ragged.hip, csrc/dech.hip, csrc/dec7.hip; network/ragged.py) --------------------
 * The reference denoises a folder one file per forward (src/examples/denoise.py:42-60, batch_size = 1).  Here clips of
 * different lengths share one forward, zero padded to the longest (lmax samples, T = valid_length(lmax) rows), and the
 * result of every clip equals its forward alone: each keeps its own std, its own framing and crop, and each decoder
 * layer's GLU output is cleared past the rows the clip would have alone.  len / valid / valid_rows are
 * device i32[batch] tables; the kernels clamp them, so a bad table never indexes outside a row.  x holds `batch` rows
 * `stride` elements apart: int16 PCM (src_i16 = 1, a sample is x 2^-15, exact) or f32 (src_i16 = 0).
 * Every entry returns CUM_EINVAL before any launch for batch < 1, lmax < 1 (T < 1 where there is no lmax), a null
 * pointer or a misaligned buffer (row buffers and packed operands 16 bytes; tables and f32 arrays 4; int16 rows 2).
 *
 * cum_clip_std_ragged <- `noisy_audio.std(dim=2, keepdim=True) + 1e-3` (src/network/CleanUMamba.py:260-262) of every
 *   file: out[b] = unbiased std of the first len[b] samples of row b + eps.  One launch for the batch, one workgroup
 *   per clip: Welford per thread over 8-sample chunks, Chan merges in a fixed order that depends on len[b] alone, so a
 *   clip's value does not depend on its batch mates, on stride or on alignment.  len[b] = 1 gives nan, as torch.std.
 * cum_frame_rows_ragged <- `noisy / std` + pad_signal (CleanUMamba.py:262-264) into the row buffer of Geo(batch, T, 1)
 *   in element type dtype: x / scale[b] for t < len[b] (a true division), zero for len[b] <= t < T, and the zero head
 *   row, the two pad rows per clip and the slack rows, as cum_frame_rows writes them (total_rows in all).  scale may be
 *   NULL (= 1).  16-byte loads where a row starts on a 16-byte boundary, 16-byte stores always.
 * cum_rows_zero_tail: on the row buffer of Geo(batch, T, C) (cp = C rounded up to 8 elements per row) clear rows
 *   [valid[b], T) of every clip and touch nothing else -- the rows `glu(conv1x1(x))` (CleanUMamba.py:121-130, decoder
 *   modules 0-1) does not have when clip b runs alone.  Work is proportional to the rows cleared.
 * cum_unframe_rows_ragged <- `x[:, :, :L] * std` (CleanUMamba.py:319) per clip: y[b][t] = rows[1 + b (T + 2) + t][0] *
 *   scale[b] for t < len[b], 0 for len[b] <= t < lmax; y is (batch, lmax) f32, contiguous.  scale may be NULL. */
int cum_clip_std_ragged(int32_t src_i16, const void *x, int32_t batch, int64_t lmax, int64_t stride, const int32_t *len,
                        float eps, float *out, void *stream);
int cum_frame_rows_ragged(int32_t dtype, int32_t src_i16, const void *x, int32_t batch, int64_t lmax, int64_t stride,
                          const int32_t *len, int64_t T, int64_t total_rows, const float *scale, void *out, void *stream);
int cum_rows_zero_tail(int32_t dtype, void *rows, int32_t batch, int64_t T, int32_t cp, const int32_t *valid,
                       void *stream);
int cum_unframe_rows_ragged(int32_t dtype, const void *rows, int32_t batch, int64_t lmax, int64_t T, const int32_t *len,
                            const float *scale, float *y, void *stream);

/* int16 PCM of a ragged batch in ONE flat buffer, the layout the metric kernels read (csrc/metrics.hip): clip b's
 * samples stand at out_i16[out_offset[b] .. out_offset[b] + len[b]), out_offset a device i64[batch] table of sample
 * offsets.  Clips are packed back to back, so a clip may start at any 2-byte position: stores are 16 bytes where the
 * destination is aligned, 2 bytes in front of the first boundary and behind the last.  Nothing outside a clip's range
 * is written (a negative offset skips the clip; ranges must not overlap).  No atomics: the same bits on every run.
 * mode 0 <- `(y * 32767).clamp(-32768, 32767).to(torch.int16)` (util/denoise_eval.py, the denoised signal):
 *   w = v * 32767.0f (f32, rounded once), clamped to [-32768, 32767], converted truncating toward zero.
 * mode 1 <- `(y * 32768).round().clamp(-32768, 32767)` (the converted clean signal): w = v * 32768.0f, rounded half to
 *   even, clamped.
 * NaN gives 0 in both modes; +inf gives 32767, -inf -32768.
 * cum_unframe_rows_ragged_pcm16: cum_unframe_rows_ragged with that store: v = (float)rows[1 + b (T + 2) + t][0] *
 *   scale[b] (one f32 product, as the f32 entry forms it; scale may be NULL) for t < len[b] clamped into [0, lmax].
 * cum_pcm16_from_f32_ragged: v = x[b stride + t] for t < len[b] clamped into [0, lmax] (rows of cum_resample_ragged).
 * batch < 1, lmax < 1, T < lmax / stride < lmax, a mode other than 0 or 1, a null pointer or a misaligned buffer (rows
 * 16 bytes, out_offset 8, len / scale / x 4, out_i16 2): CUM_EINVAL before any launch. */
int cum_unframe_rows_ragged_pcm16(int32_t dtype, const void *rows, int32_t batch, int64_t lmax, int64_t T,
                                  const int32_t *len, const float *scale, int32_t mode, int16_t *out_i16,
                                  const int64_t *out_offset, void *stream);
int cum_pcm16_from_f32_ragged(const float *x, int32_t batch, int64_t lmax, int64_t stride, const int32_t *len,
                              int32_t mode, int16_t *out_i16, const int64_t *out_offset, void *stream);

/* cum_dech_fwd_ragged / cum_dec7_fwd_ragged: cum_dech_fwd / cum_dec7_fwd (the decoder layers of
 * src/network/CleanUMamba.py:121-130 at widths 128 and 64, which never store their GLU output) for a ragged batch: the
 * GLU output of clip c = row / pitch is kept for its first min(valid_rows[c], valid) rows only; M must be batch x pitch.
 * The same kernel bodies, switched at compile time.  Inference only: no GLU output, gate or sign nibbles are stored. */
int cum_dech_fwd_ragged(int32_t dtype, int64_t M, int32_t pitch, int32_t valid, const int32_t *valid_rows, int32_t batch,
                        const void *u, int64_t u_rows, const void *w1p, const float *b1p, const void *wtp,
                        const float *btp, const void *skip, void *out, int64_t out_tail, void *stream);
int cum_dec7_fwd_ragged(int32_t dtype, int64_t M, int32_t pitch, int32_t valid, const int32_t *valid_rows, int32_t batch,
                        const void *u, const void *w1p, const float *b1p, const float *wt, const float *bt, void *out,
                        int64_t zero_tail, void *stream);

/* ---- sample-rate conversion of a ragged batch (csrc/resample.hip; util/resample.py) -------------------
 * The reference has no resampler: it drops the rate torchaudio.load returns (src/util/dataset.py:203).  For
 * rate_in -> rate_out with g = gcd, up = rate_out / g, down = rate_in / g and the n_taps = 2H + 1 taps h (odd count,
 * symmetric, sum up):   y[m] = sum_{j < K} x[n_hi - j] h[r + j up],  c = m down + H, r = c mod up, n_hi = c / up,
 * K = ceil(n_taps / up), samples outside the signal zero.  One f32 fma chain per output, j ascending: its order depends
 * on (m, up, down, H) alone.
 *
 * cum_resample_tile: outputs one workgroup produces.
 * cum_resample_ragged: one launch for `batch` rows of x (int16 PCM x 2^-15 with src_i16 = 1, or f32), in_pitch elements
 *   apart, row b holding len[b] samples (device i32[batch], clamped into [0, lmax] inside the kernel).  table: the taps
 *   as the polyphase table [up][table_pitch] f32 on the device, table[r][j] = h[r + j up], zero behind the taps;
 *   table_pitch >= K and a multiple of 4.  origin: device i64[batch][2] or NULL (zeros) -- the absolute input position
 *   of x_b[0] and the absolute output position of y_b[0], so that the same launch computes outputs [m0, m1) of a longer
 *   signal from a window of it.  Inputs before position 0 are zero.  With ends != 0 the signal of row b ends at
 *   origin + len[b] and the row gets outputs up to ceil((in0 + len) up / down); with ends == 0 only the outputs no
 *   later input can change, max(0, ceil(((in0 + len) up - H) / down)), are written.  Either count is taken from out0
 *   and capped at max_out.  y: f32 rows out_pitch apart; nothing is written behind a row's count, nothing is read
 *   behind len[b].  Needs no workspace.
 *   CUM_EINVAL before any launch: src_i16 not 0 / 1, batch outside [1, 65534], up or down outside [1, 1024], an even
 *   tap count, K up < n_taps, table_pitch < K or not a multiple of 4, a null table / len / y (x may be NULL with
 *   lmax = 0), a negative pitch or length, a pitch below its length, a misaligned pointer (table 16 bytes, origin 8,
 *   f32 and i32 4, int16 2), or a ratio whose tile span (tile down / up + K samples) exceeds 48 KB of LDS. */
int32_t cum_resample_tile(void);
int cum_resample_ragged(int32_t src_i16, const void *x, int32_t batch, int64_t lmax, int64_t in_pitch, const int32_t *len,
                        const int64_t *origin, int32_t ends, int32_t up, int32_t down, int32_t n_taps, int32_t K,
                        const float *table, int32_t table_pitch, float *y, int64_t out_pitch, int64_t max_out,
                        void *stream);
/* cum_resample_slots: the same chains (bit for bit) for streams of different rate pairs at different positions, in one
 *   launch over a record table -- what converts the stream pool's slots (network/streampool.py).
 *   hist: [capacity][2][hist_pitch] f32, the inputs a slot's unfinished outputs may still read, TWO rows per slot: a
 *   record reads row `parity` and writes the next history to row 1 - parity, so the workgroups of a record (one per
 *   cum_resample_tile outputs) never read what one of them writes.  The signal a record sees is
 *   hist[slot][parity][0, n_hist) ++ x[x_row][0, n_new), its first sample at absolute position in0.
 *   The two layouts below and the record of cum_pcm_batch_resample_f32 are described here alone; their fields are named
 *   in csrc/resample.hip (RsPlanField, RsSlotField, RsFeedField) and in util/resample.py (PLAN_INTS, REC_INTS, SLOT_*,
 *   FEED_*, REC_IN0 / REC_OUT0), whose PlanTable builds `plans_host`, `plans` and `tables`.
 *   Plan p = 8 int32 {up, down, n_taps, K, table_pitch, table_offset, 0, 0}: the pair's polyphase table (as for
 *     cum_resample_ragged) starts table_offset floats (a multiple of 4) into `tables` (table_floats long, 16-byte
 *     aligned).  up <= 3 takes the scalar-tap route, any other the per-lane row route, per record.
 *   Record r = 16 int32 {slot, plan, n_hist, x_row, n_new, n_out, y_row, ends, keep, parity, y_col, 0,
 *     in0 (int64 in ints 12-13), out0 (int64 in ints 14-15)}:
 *       y[y_row][y_col + o] = output out0 + o of the signal, o < n_out (inputs before position 0 and behind the
 *         samples held enter as zeros);
 *       hist[slot][1 - parity][0, keep) = the last `keep` samples of the signal.
 *     Nothing is read behind n_hist / n_new, nothing is written behind n_out / keep.  A record with n_out = 0 only
 *     moves the history.
 *   plans / recs: device tables; plans_host / recs_host: the same in host memory, checked before the launch.  x, y:
 *   f32 rows x_pitch / y_pitch apart, x_rows / y_rows of them (x may be NULL with x_rows = 0).  No workspace, no atomics.
 *   CUM_EINVAL before any launch: a null or misaligned pointer (tables 16 bytes, records 8, the rest 4), capacity or
 *   n_plans < 1, n_recs outside [0, 65535], a negative pitch or row count, plan fields outside the limits of
 *   cum_resample_ragged (the LDS span included) or a table outside the blob, a slot outside [0, capacity), a slot named
 *   twice, a plan id outside [0, n_plans), parity not 0 / 1, n_hist or keep above hist_pitch, keep above
 *   n_hist + n_new, a chunk or outputs that do not fit the rows of x / y, a negative position, out0 + n_out beyond the
 *   outputs the samples make final (ends = 0) or the signal has (ends != 0), or a history that starts behind the oldest
 *   sample the first output reads.  n_recs = 0 returns CUM_OK after the plan checks, without a launch. */
int cum_resample_slots(float *hist, int64_t hist_pitch, int32_t capacity, const int32_t *plans_host, const int32_t *plans,
                       int32_t n_plans, const float *tables, int64_t table_floats, const int32_t *recs_host,
                       const int32_t *recs, int32_t n_recs, const float *x, int32_t x_rows, int64_t x_pitch, float *y,
                       int32_t y_rows, int64_t y_pitch, void *stream);
/* cum_pcm_batch_resample_f32: cum_pcm_batch_f32 for pairs at any mix of sample rates (training/feeder.py with
 *   sample_rate): one launch from the int16 source windows of a batch to the model-rate float crops of
 *   both signals, with the chains of cum_resample_ragged bit for bit (the kernels inline one device function).
 *   pcm: 2 * batch rows `pitch` int16 apart, row b the clean clip, row batch + b the noisy clip of pair b.
 *   Plans and `tables`: as for cum_resample_slots (n_plans may be 0: plans and tables may then be NULL).
 *   Record b = 16 int32 {plan, n_src, M, N, 0 x 8, in0 (int64 in ints 12-13), out0 (int64 in ints 14-15)}, one per pair:
 *     both rows hold samples [in0, in0 + n_src) of a file of N samples, a sample being pcm x 2^-15; y is the conversion
 *     of the whole file under `plan` (what lies outside the file is zero), M = ceil(N up / down) outputs long; plan -1:
 *     the pair is at the model rate, y[m] = pcm[m - in0] 2^-15 (cum_pcm_batch_f32's arithmetic, exact) and M = N.
 *       clean[b clean_sb + t] = y_clean[(out0 + t) mod M],  noisy[b noisy_sb + t] = y_noisy[(out0 + t) mod M],  t < len
 *     with out0 + len <= M (a crop) or out0 = 0 (a file of M <= len outputs repeated to fill the crop).  Every output is
 *     computed once; the repeats are copies.  16-byte loads of whole aligned chunks inside the window, 16-byte stores
 *     from a row's first 16-byte boundary on.  Nothing is read behind n_src, nothing is written behind len.  The kernel
 *     clamps n_src into [0, pitch], M to >= 1 and the positions into [0, 2^51] (out0 below M), and skips a record whose
 *     plan id is outside the table, so a bad device table never indexes outside a row.
 *   recs / plans: device tables; recs_host / plans_host: the same in host memory, checked before the launch.  No
 *   workspace, no atomics; LDS 4 (span + cum_resample_tile) bytes, span the largest tile span of the plans.
 *   CUM_EINVAL before any launch: a null or misaligned pointer (pcm, clean, noisy, tables 16 bytes; records 8; plans 4),
 *   batch outside [1, 32767], len < 1, pitch not a multiple of 8 or below a record's n_src, clean_sb or noisy_sb below
 *   len, a plan id outside [-1, n_plans), plan fields outside the limits of cum_resample_ragged (the LDS span included)
 *   or a table outside the blob, M < 1 or not ceil(N up / down), out0 + len > M with out0 != 0, a negative position, a
 *   window that runs past its file, that starts behind the oldest sample its first output reads (unless it starts the
 *   file) or ends before the newest sample its last output reads (unless it ends the file). */
int cum_pcm_batch_resample_f32(const int16_t *pcm, int64_t pitch, const int32_t *recs_host, const int32_t *recs,
                               int32_t batch, const int32_t *plans_host, const int32_t *plans, int32_t n_plans,
                               const float *tables, int64_t table_floats, int64_t len, float *clean, int64_t clean_sb,
                               float *noisy, int64_t noisy_sb, void *stream);

/* ---- training augmentation (csrc/augment.hip; training/augment.py) -----------------------------------
 * cum_augment_pairs <- the hook of the train loop, src/training/train.py:262-265
 *   (`noise = noisy_audio - clean_audio; noise, clean_audio = augment((noise, clean_audio)); noisy_audio = noise +
 *   clean_audio`): exchange the noises within the batch, shift noise against speech, add a synthetic room, re-draw the
 *   SNR and the level, from the assembled crops straight into the step's inputs.
 *   clean_src / noisy_src: f32 rows of src_len samples, clean_src_sb / noisy_src_sb apart (C and Y below).
 *   recs: device table, 8 int32 per row {perm, off_clean, off_noise, n_taps, snr_db (f32), gain (f32), kappa (f32), 0}.
 *   tap_delay (i32) / tap_gain (f32): device tables of k_max entries per row, the first n_taps of them used.
 *   For row b, p = perm[b], t < len, the sums over k < n_taps in ascending k as one fma chain, terms with
 *   t < delay[b][k] dropped:
 *     c0[t] = C[b][t + off_clean],  n0[t] = Y[p][t + off_noise] - C[p][t + off_noise]
 *     rc[t] = sum_k tap_gain[b][k] c0[t - delay[b][k]],  rn[t] = sum_k tap_gain[b][k] n0[t - delay[b][k]]
 *     c1 = c0 + kappa rc,  n1 = n0 + rn + (1 - kappa) rc
 *     Ec = sum_t c1[t]^2, En = sum_t n1[t]^2 in f64, one fixed order
 *     a = sqrt(Ec / (En 10^(snr_db / 10))) if snr_db is finite and Ec > 0 and En > 0, else 1
 *     clean[b clean_sb + t] = gain c1[t],  noisy[b noisy_sb + t] = gain (c1[t] + a n1[t])
 *   workspace: cum_augment_workspace_elems(batch, len) floats, 8-byte aligned; or NULL: no row has a finite snr_db (a
 *   = 1 everywhere, snr_db is not read) and one launch does it all.  With a workspace there are two launches.  No
 *   atomics: two runs give the same bits.  The kernel clamps perm into [0, batch), the offsets into [0, src_len - len]
 *   and n_taps into [0, k_max], and drops a tap whose delay is below 1, so a bad table never indexes outside its rows.
 *   The outputs must not overlap the sources (the caller's check).  Nothing is allocated, read on the host or waited for.
 *   CUM_EINVAL before any launch: batch outside [1, 32767], len < 1, src_len < len (src_len is len plus the largest
 *   offset), k_max outside [0, 512], a source stride below src_len, clean_sb or noisy_sb below len, a null pointer
 *   (tap_delay / tap_gain may be NULL with k_max = 0), clean or noisy off a 16-byte boundary, workspace off an 8-byte
 *   one, any other pointer off a 4-byte one. */
int64_t cum_augment_workspace_elems(int32_t batch, int64_t len);
int cum_augment_pairs(const float *clean_src, int64_t clean_src_sb, const float *noisy_src, int64_t noisy_src_sb,
                      int32_t batch, int64_t len, int64_t src_len, const int32_t *recs, const int32_t *tap_delay,
                      const float *tap_gain, int32_t k_max, float *workspace, float *clean, int64_t clean_sb,
                      float *noisy, int64_t noisy_sb, void *stream);

/* ---- BandMask (csrc/bandmask.hip; training/augment.py) ----------------------------------------------
 * cum_band_mask_pairs <- the same hook of the train loop, src/training/train.py:262-265 (`noise, clean_audio =
 *   augment((noise, clean_audio))`): the BandMask of the denoiser lineage, a band-stop between two mel edges applied
 *   to speech and noisy alike, as the stage in front of cum_augment_pairs.
 *   clean_src / noisy_src: f32 rows of n samples, clean_src_sb / noisy_src_sb apart (C and Y below, zero outside [0, n)).
 *   recs: device table, 4 int32 per row {W, c_lo (f32), c_hi (f32), 0}: the half-width and the two cutoffs in cycles
 *   per sample.  For a row with W > 0, k = -W..W, everything in f64 and h then rounded to f32:
 *     w[k]    = 0.54 - 0.46 cos(pi (k + W) / W)
 *     lp_c[k] = 2 c sinc(2 c k) w[k],  sinc(x) = sin(pi x) / (pi x), sinc(0) = 1
 *     h[k]    = [k == 0] + lp_lo[k] - lp_hi[k]
 *     clean[b clean_sb + t] = sum_k h[k] C[b][t - k],  noisy[b noisy_sb + t] = sum_k h[k] Y[b][t - k],  t in [0, n)
 *   by overlap-save on an in-LDS FFT of cum_band_mask_block() points (z = C + i Y: one transform pair filters both).
 *   A row with W = 0 is copied bit for bit.  The kernel clamps W into [0, 1600] and takes a row whose cutoffs are not
 *   finite or not 0 <= c_lo <= c_hi <= 0.5 as W = 0, so a bad table never indexes anywhere.
 *   workspace: cum_band_mask_workspace_elems(batch) floats, 8-byte aligned (the twiddle table and one spectrum per
 *   row; written by the first of the two launches, read by the second).  No atomics: two runs give the same bits, and a
 *   row's result does not depend on the rest of the batch.  Nothing outside [row, row + n) is read or written.
 *   The outputs must not overlap the sources (the caller's check).  Nothing is allocated, read on the host or waited for.
 *   CUM_EINVAL before any launch: batch outside [1, 32767], n < 1, a stride below n, a null pointer, clean or noisy off
 *   a 16-byte boundary, workspace off an 8-byte one, any other pointer off a 4-byte one.
 * cum_band_mask_block: N, the FFT length; a row with half-width W is cut into blocks of V = N - 2 W outputs. */
int32_t cum_band_mask_block(void);
int64_t cum_band_mask_workspace_elems(int32_t batch);
int cum_band_mask_pairs(const float *clean_src, int64_t clean_src_sb, const float *noisy_src, int64_t noisy_src_sb,
                        int32_t batch, int64_t n, const int32_t *recs, float *workspace, float *clean, int64_t clean_sb,
                        float *noisy, int64_t noisy_sb, void *stream);

/* ---- room impulse responses (csrc/reverb.hip; training/augment.py) -----------------------------------
 * cum_reverb_pairs <- the same hook of the train loop, src/training/train.py:262-265 (`noise, clean_audio =
 *   augment((noise, clean_audio))`): the speech of a row convolved with a measured or simulated room response, as the
 *   DNS synthesiser does before it adds the noise; the stage in front of cum_band_mask_pairs and cum_augment_pairs.
 *   clean_src / noisy_src: f32 rows of n samples, clean_src_sb / noisy_src_sb apart (C and Y below, zero outside [0, n)).
 *   recs: device table, 4 int32 per row {rir, 0, 0, 0}: the id of the row's response.
 *   bank: device blob of bank_floats f32, every response starting on a 16-byte boundary, h[0] the direct path.
 *   rirs: device table of n_rirs records of 4 int32 {offset into the bank in floats (int64 in ints 0-1), taps, 0};
 *   rirs_host: the same in host memory, checked before the launch.
 *   A row with rir outside [0, n_rirs) is copied bit for bit.  Otherwise, h = bank[rir] of T taps, t in [0, n):
 *     Cr[t] = sum_{k = 0 .. min(t, T - 1)} h[k] C[b][t - k]
 *     clean[b clean_sb + t] = Cr[t]
 *     noisy[b noisy_sb + t] = (Y[b][t] - C[b][t]) + Cr[t]          (f32: one subtraction, then one addition)
 *   by uniformly partitioned overlap-save on an in-LDS FFT of N = cum_reverb_block() points: partitions of the response
 *   and output blocks are N / 2 long, the spectra of block m - k and partition k are multiplied and added in ascending k
 *   as one fma chain, one inverse transform per block.  The target is the reverberant speech and the noise Y - C stays
 *   free of speech.  The kernel reads the device table again and does not trust it: an offset outside the bank makes
 *   the row a copy, taps are clamped into [1, cum_reverb_max_taps()] and to what the bank holds behind the offset, so a
 *   bad device table never indexes outside the bank.
 *   workspace: cum_reverb_workspace_elems(batch, n) floats, 8-byte aligned (the twiddle table, the spectra of every
 *   row's partitions and input blocks; written by the first two of the three launches, read by the last two).  No
 *   atomics: two runs give the same bits, and a row's result depends on its own record and samples only.  Nothing
 *   outside [row, row + n) is read or written.  The outputs must not overlap the sources (the caller's check).  Nothing
 *   is allocated, read back or waited for.
 *   CUM_EINVAL before any launch: batch outside [1, 32767], n < 1, a stride below n, a null pointer, clean or noisy off
 *   a 16-byte boundary, workspace off an 8-byte one, any other pointer off a 4-byte one, n_rirs or bank_floats below 1,
 *   a response in rirs_host with taps outside [1, cum_reverb_max_taps()], with an offset that is negative or not a
 *   multiple of 4 floats, or whose span leaves the bank.
 * cum_reverb_block: N, the FFT length; partitions and output blocks are N / 2 long.
 * cum_reverb_max_taps: T_MAX = 16384: 1.02 s at 16 kHz, 8 partitions at N = 4096. */
int32_t cum_reverb_block(void);
int32_t cum_reverb_max_taps(void);
int64_t cum_reverb_workspace_elems(int32_t batch, int64_t n);
int cum_reverb_pairs(const float *clean_src, int64_t clean_src_sb, const float *noisy_src, int64_t noisy_src_sb,
                     int32_t batch, int64_t n, const int32_t *recs, const float *bank, int64_t bank_floats,
                     const int32_t *rirs_host, const int32_t *rirs, int32_t n_rirs, float *workspace, float *clean,
                     int64_t clean_sb, float *noisy, int64_t noisy_sb, void *stream);

/* ---- speech and noise mixed on the device (csrc/mix.hip; training/mix.py) -----------------------------
 * cum_mix_pairs: the mixer of the DNS challenge's synthesiser in place of cum_pcm_batch_f32, for a feeder over two
 *   unpaired corpora (the reference trains from pre-mixed pairs only, src/util/dataset.py:108-150): the noise scaled to
 *   an SNR measured on the ACTIVE frames of both signals, the mixture brought to a level in dBFS, a guard against
 *   clipping.  The scheme follows the synthesiser's; it has not been compared with its output.
 *   pcm: 2 * batch rows, `pitch` int16 apart; row b is speech, row batch + b noise (cum_pcm_batch_f32's layout).
 *   recs: device table, 12 int32 per row {n_speech, frame, thr (int64 in ints 2-3), q (f64 in ints 4-5), l (f64 in ints
 *   6-7), clip (f32), 0, 0, 0}: q = 10^(snr_db / 10), l = 10^(level_db / 10) or NaN (keep the level), thr = floor(2^30
 *   10^(activity_db / 10)), all formed on the host in double: the device evaluates no transcendental.
 *   For row b, t < len:  S[t] = pcm[b][t mod n_s], n_s = n_speech clamped into [1, len];  N[t] = pcm[batch + b][t].
 *     frames [k frame, min((k + 1) frame, len)), frame clamped into [1, len], thr into [0, 2^30]; per frame of m samples
 *       es_k = sum S^2, en_k = sum N^2; over the row Ss = sum S^2, Snn = sum N^2, Ssn = sum S N: exact, in int64;
 *       a frame is active iff e_k > thr m (integers)
 *     Ps = (sum es_k over active frames) / (sum m over active frames), or Ss / len if no frame is active; Pn likewise (f64)
 *     a = sqrt(Ps / (Pn q)) if Ps > 0, Pn > 0 and q is finite and positive, else 1;  a32 = (float) a
 *     Em = (A Snn + 2 Ssn) A + Ss,  A = (double) a32  (f64, no fused operation)
 *     g = sqrt(l len 2^30 / Em) if l is finite and Em > 0, else 1;  g32 = (float) g
 *     m[t] = fmaf(a32, N[t] 2^-15, S[t] 2^-15),  peak = max_t |m[t]|  (f32)
 *     if g32 peak > clip: g32 = clip / peak  (one f32 division)
 *     clean[b clean_sb + t] = g32 (S[t] 2^-15),  noisy[b noisy_sb + t] = g32 m[t]
 *   stats: NULL, or batch rows of 8 f32 {a32, g32 (as applied), Ps 2^-30, Pn 2^-30, peak, (sum m over active speech
 *   frames) / len, the same of noise, 1.0 if the guard acted else 0.0}.
 *   workspace: cum_mix_workspace_elems(batch, len) floats, 8-byte aligned (the workgroups' integer totals and the tiles'
 *   peaks; written by the first two of the three launches, read by the last two).  No atomics, and every sum is an exact
 *   integer: two runs give the same bits, and a row's result depends on its own record and samples only.  Nothing is
 *   read behind len in a row of pcm, nothing written behind len in an output row.  Nothing is allocated, read on the
 *   host or waited for.
 *   CUM_EINVAL before any launch: batch outside [1, 32767], len < 1, pitch < len, pitch % 8 != 0, clean_sb or noisy_sb
 *   below len, a null pointer (stats may be NULL), pcm / clean / noisy off a 16-byte boundary, workspace or recs off an
 *   8-byte one, stats off a 4-byte one. */
int64_t cum_mix_workspace_elems(int32_t batch, int64_t len);
int cum_mix_pairs(const int16_t *pcm, int64_t pitch, const int32_t *recs, int32_t batch, int64_t len, void *workspace,
                  float *clean, int64_t clean_sb, float *noisy, int64_t noisy_sb, float *stats, void *stream);

/* ---- teacher / student feature distillation loss (csrc/distill.hip; training/distill.py) ---------------
 * The teacher branch of the reference's loss_fn (src/util/util.py:259-290, after arXiv:2303.11098): per layer the
 * embedded student feature e and the teacher feature t go through BatchNorm1d(affine=False) in training mode
 * (ad["bn_s"], ad["bn_t"], :276-279), d = s^ - t^, D = sum d^4, L = kd_p log D (:281-284).  The ~15 elementwise and
 * reduction passes of that chain, and the four full-size tensors its autograd keeps, become three streaming passes over
 * e and t for ALL layers at once, each one launch over work items (layer, chunk of CUM_DISTILL_ROWS rows) plus one small
 * launch that merges the chunks' partial results in a fixed order (no atomics: two runs give the same bits):
 *   stats  per chunk and channel (mean, M2) of e and t (Welford per lane, Chan's merge through LDS and over the chunks,
 *          the latter in f64; every value relative to its chunk's first row, so features far from zero keep their digits)
 *          -> cst[ch] = {mean_e hi, lo, rstd_e, 0, mean_t hi, lo, rstd_t, 0}, rstd = 1 / sqrt(M2 / n + eps), n = B T; and
 *          the modules' training-mode side effects: running_mean = (1 - momentum) running_mean + momentum mean,
 *          running_var likewise with M2 / (n - 1), num_batches_tracked += 1 (pointers may be NULL: no update).
 *   loss   s^ = ((e - hi) - lo) rstd_e, t^ likewise, d = s^ - t^: per chunk sum d^4 and per channel sum d^3, sum d^3 s^
 *          -> csum[ch] = {sum d^3, sum d^3 s^} (f64), D[layer] (f64), L[layer] = kd_p log D[layer].
 *   bwd    de = rstd_e a (d^3 - csum[0] / n - s^ csum[1] / n), a = (float)(4 kd_p / D) G[layer] formed in f32, written in
 *          e's element type to de (C rounded up to 8 columns per row, the columns past C and, where de_sb > T de_st, the
 *          rows between clips written as zeros).  G: device f32, the upstream gradient of every L[layer].  Nothing flows
 *          to t.
 * A layer's e and t are (B, T, C) with element strides (sb, st, 1): views of the conv stack's row buffers (st = C rounded
 * up to 8, sb = (T + 2) st) or contiguous tensors.  Elements past column C of a row and rows past T of a clip are never
 * added into a sum.  16-byte loads are used where a side's base is 16-byte aligned and st, sb are multiples of 8 elements
 * with st >= C rounded up to 8; other layouts are read element by element.  e_dtype, t_dtype: CUM_F32 / CUM_BF16 /
 * CUM_F16; de has e's.  All arithmetic is f32 or f64.
 * cum_distill_sizes: sizes[0] = f32 elements of `part`, sizes[1] = channels over all layers (cst holds 8 f32, csum 2 f64
 *   per channel), sizes[2] = chunks over all layers (s4 holds one f32 per chunk).  D and L hold one value per layer.
 * cum_distill_fwd: passes & 1 runs stats, passes & 2 runs loss (which reads what stats left in cst).
 * CUM_EINVAL before any launch: n_layers outside [1, CUM_DISTILL_MAX_LAYERS], a layer with B, T or C < 1, B T < 2 or
 * B T >= 2^31, a stride below what (T, C) need, an unknown dtype, a null e / t (de for cum_distill_bwd) or workspace. */
#define CUM_DISTILL_MAX_LAYERS 16
#define CUM_DISTILL_ROWS 256
typedef struct {
  const void *e, *t;
  void *de;
  float *rm_s, *rv_s, *rm_t, *rv_t;       /* running_mean / running_var of bn_s and bn_t, or NULL */
  int64_t *nbt_s, *nbt_t;                 /* num_batches_tracked of bn_s and bn_t, or NULL */
  int64_t e_sb, e_st, t_sb, t_st, de_sb, de_st;
  int32_t B, T, C;
  int32_t e_dtype, t_dtype;
  float momentum, eps;
  int32_t pad_;
} cum_distill_layer;
int cum_distill_sizes(const cum_distill_layer *layers, int32_t n_layers, int64_t *sizes);
int cum_distill_fwd(const cum_distill_layer *layers, int32_t n_layers, float kd_p, int32_t passes, float *part, float *cst,
                    double *csum, float *s4, double *D, float *L, void *stream);
int cum_distill_bwd(const cum_distill_layer *layers, int32_t n_layers, float kd_p, const float *cst, const double *csum,
                    const double *D, const float *G, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CLEANUMAMBA_HIP_H */
