// Waveform ends and row masks of the ragged inference forward for gfx950: one batch of clips of DIFFERENT lengths, zero
// padded to the longest, goes through the fused conv stack once (network/ragged.py).  Every clip keeps its own std, its
// own framing and its own crop, and no value computed over padding leaves:
//
//   cum_clip_std_ragged      <- noisy_audio.std(dim=2, keepdim=True) + 1e-3 of every clip over ITS samples
//                               (src/network/CleanUMamba.py:260-262, called per file by src/examples/denoise.py:54-60)
//   cum_frame_rows_ragged    <- noisy / std + pad_signal into the first conv's row buffer (CleanUMamba.py:262-264)
//   cum_rows_zero_tail       <- the rows a clip does not have when it runs alone: the GLU output of a decoder layer
//                               (CleanUMamba.py:121-130) past the clip's own row count is cleared
//   cum_unframe_rows_ragged  <- x[:, :, :L] * std of every clip (CleanUMamba.py:319), zeros behind L
//   cum_unframe_rows_ragged_pcm16  the same crop, quantised to int16 into one flat buffer (the layout of the metric
//                               kernels, csrc/metrics.hip): validate's `(y * 32767).clamp(..).to(int16)` on the device
//   cum_pcm16_from_f32_ragged   the same quantisers on f32 rows (the output of cum_resample_ragged)
//
// Rows arrive as the files hold them (int16 PCM, scaled by 2^-15: exact in f32) or as f32.  `len` / `valid` are device
// i32 tables, clamped inside the kernels: a bad table never indexes outside a row.  All four move bytes and do nothing
// else, so every global access is 16 bytes per lane wherever the row's alignment allows it.
#include "common.h"

namespace cum {

constexpr int RT = 256;             // threads per workgroup of the framing kernels
constexpr int RS = 1024;            // threads of the std workgroup (one per clip)
constexpr float kRagPcm = 1.f / 32768.f;

typedef short rg_short8 __attribute__((ext_vector_type(8)));
typedef float rg_float4 __attribute__((ext_vector_type(4)));

// Eight consecutive samples [8 c, 8 c + 8) of one row as f32.  wide: the row starts on a 16-byte boundary and the chunk
// is whole -- the values and their order are the same on both routes, only the loads differ.
template <typename S>
__device__ __forceinline__ void rg_load8(const S *__restrict__ row, int64_t c, int64_t n, bool wide, float v[8]) {
  const int64_t t0 = 8 * c;
  if (wide && t0 + 8 <= n) {
    if constexpr (sizeof(S) == 2) {
      const rg_short8 s = *reinterpret_cast<const rg_short8 *>(row + t0);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (float)s[j] * kRagPcm;
    } else {
      const rg_float4 a = *reinterpret_cast<const rg_float4 *>(row + t0);
      const rg_float4 b = *reinterpret_cast<const rg_float4 *>(row + t0 + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = a[j];
        v[4 + j] = b[j];
      }
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float x = 0.f;
    if (t0 + j < n) x = sizeof(S) == 2 ? (float)row[t0 + j] * kRagPcm : (float)row[t0 + j];
    v[j] = x;
  }
}

// ---------------------------------------------------------------- unbiased std of the first len[b] samples of row b
// One workgroup per clip, one launch per batch.  Thread i takes the 8-sample chunks i, i + 1024, ... in order (Welford),
// then Chan's merges: across the wave by xor distance 1, 2, ... 32 with (lower lane, upper lane) operands, the 16 waves
// as a fixed tree.  The order depends on the clip's own length only -- not on the batch, the pitch or the alignment.
struct RgWf {
  float n, mean, m2;
};
__device__ __forceinline__ RgWf rg_merge(RgWf a, RgWf b) {
  const float n = a.n + b.n;
  if (n == 0.f) return a;
  const float d = b.mean - a.mean, f = b.n / n;
  RgWf r;
  r.n = n;
  r.mean = a.mean + d * f;
  r.m2 = a.m2 + b.m2 + d * d * a.n * f;
  return r;
}

template <typename S>
__global__ __launch_bounds__(RS) void std_ragged_kernel(const S *__restrict__ x, int64_t stride, int64_t Lmax,
                                                       const int32_t *__restrict__ len, float eps,
                                                       float *__restrict__ out) {
  __shared__ RgWf sw[RS / 64];
  const int b = blockIdx.x;
  const S *__restrict__ row = x + (int64_t)b * stride;
  int64_t n = len[b];
  n = n < 0 ? 0 : (n > Lmax ? Lmax : n);
  const bool wide = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
  RgWf a{0.f, 0.f, 0.f};
  const int64_t chunks = (n + 7) / 8;
  for (int64_t c = threadIdx.x; c < chunks; c += RS) {
    float v[8];
    rg_load8(row, c, n, wide, v);
    const int m = n - 8 * c < 8 ? (int)(n - 8 * c) : 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j < m) {
        a.n += 1.f;
        const float d = v[j] - a.mean;
        a.mean += d / a.n;
        a.m2 += d * (v[j] - a.mean);
      }
    }
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    RgWf p;
    p.n = __shfl_xor(a.n, o, 64);
    p.mean = __shfl_xor(a.mean, o, 64);
    p.m2 = __shfl_xor(a.m2, o, 64);
    a = (threadIdx.x & o) ? rg_merge(p, a) : rg_merge(a, p);      // both partners form the same value
  }
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    RgWf t[RS / 64];
#pragma unroll
    for (int i = 0; i < RS / 64; ++i) t[i] = sw[i];
#pragma unroll
    for (int w = RS / 128; w >= 1; w >>= 1)
#pragma unroll
      for (int i = 0; i < w; ++i) t[i] = rg_merge(t[2 * i], t[2 * i + 1]);
    out[b] = sqrtf(t[0].m2 / (t[0].n - 1.f)) + eps;               // one sample: nan, as torch.std
  }
}

// ---------------------------------------------------------------- (B, Lmax) rows -> row buffer of Geo(B, T, 1)
// grid (workgroups along the clip, B + 1): blockIdx.y < B writes the T + 2 rows of clip y, eight rows (one 16-byte load,
// eight row stores) per lane; blockIdx.y == B writes the leading zero row and the slack rows.
template <typename T, typename S>
__global__ __launch_bounds__(RT) void frame_rows_ragged_kernel(const S *__restrict__ x, int64_t stride, int64_t Lmax,
                                                              int B, const int32_t *__restrict__ len, int64_t Tn, int64_t R,
                                                              const float *__restrict__ s, T *__restrict__ out) {
  typedef T V __attribute__((ext_vector_type(8)));
  const V zero = {(T)0.f, (T)0.f, (T)0.f, (T)0.f, (T)0.f, (T)0.f, (T)0.f, (T)0.f};
  const int64_t P = Tn + 2;
  const int64_t tid = (int64_t)blockIdx.x * RT + threadIdx.x, nthreads = (int64_t)gridDim.x * RT;
  const int b = blockIdx.y;
  if (b == B) {
    const int64_t first = 1 + (int64_t)B * P, extra = 1 + (R - first);
    for (int64_t i = tid; i < extra; i += nthreads) {
      const int64_t r = i == 0 ? 0 : first + i - 1;
      *reinterpret_cast<V *>(out + r * 8) = zero;
    }
    return;
  }
  const S *__restrict__ row = x + (int64_t)b * stride;
  int64_t n = len[b];
  n = n < 0 ? 0 : (n > Lmax ? Lmax : n);
  const float sc = s ? s[b] : 1.f;
  const bool wide = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
  T *__restrict__ dst = out + (1 + (int64_t)b * P) * 8;
  const int64_t chunks = (P + 7) / 8;
  for (int64_t c = tid; c < chunks; c += nthreads) {
    float v[8];
    rg_load8(row, c, n, wide, v);                // zeros from sample n on
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int64_t t = 8 * c + j;
      if (t < P) {
        V o = zero;
        if (t < n) o[0] = (T)(v[j] / sc);        // a true division where the reference divides (noisy / std)
        *reinterpret_cast<V *>(dst + t * 8) = o;
      }
    }
  }
}

// ---------------------------------------------------------------- zero rows [valid[b], T) of every clip of a row buffer
// grid (workgroups along the tail, B).  A clip's tail is one contiguous run of 16-byte chunks; workgroups past it leave.
__global__ __launch_bounds__(RT) void rows_zero_tail_kernel(uint4 *__restrict__ rows1, int64_t T, int64_t row_chunks,
                                                           const int32_t *__restrict__ valid) {
  const int b = blockIdx.y;
  int64_t v = valid[b];
  v = v < 0 ? 0 : (v > T ? T : v);
  const int64_t n = (T - v) * row_chunks;
  uint4 *__restrict__ dst = rows1 + ((int64_t)b * (T + 2) + v) * row_chunks;
  for (int64_t i = (int64_t)blockIdx.x * RT + threadIdx.x; i < n; i += (int64_t)gridDim.x * RT)
    dst[i] = make_uint4(0u, 0u, 0u, 0u);
}

// ---------------------------------------------------------------- row buffer of Geo(B, T, 1) -> (B, Lmax) f32
// Four samples per lane: one 16-byte store where the output row is aligned.
template <typename T>
__global__ __launch_bounds__(RT) void unframe_rows_ragged_kernel(const T *__restrict__ rows, int64_t Lmax, int64_t Tn,
                                                                const int32_t *__restrict__ len,
                                                                const float *__restrict__ s, float *__restrict__ y) {
  const int b = blockIdx.y;
  int64_t n = len[b];
  n = n < 0 ? 0 : (n > Lmax ? Lmax : n);
  n = n > Tn ? Tn : n;
  const float sc = s ? s[b] : 1.f;
  const T *__restrict__ src = rows + (1 + (int64_t)b * (Tn + 2)) * 8;
  float *__restrict__ dst = y + (int64_t)b * Lmax;
  const bool wide = (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  const int64_t chunks = (Lmax + 3) / 4;
  for (int64_t c = (int64_t)blockIdx.x * RT + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * RT) {
    const int64_t t0 = 4 * c;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = t0 + j < n ? (float)src[(t0 + j) * 8] * sc : 0.f;
    if (wide && t0 + 4 <= Lmax) {
      *reinterpret_cast<rg_float4 *>(dst + t0) = rg_float4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (t0 + j < Lmax) dst[t0 + j] = v[j];
    }
  }
}

// ---------------------------------------------------------------- f32 values -> int16 PCM in ONE flat buffer
// The two quantisers of util/denoise_eval.py, each one f32 product rounded once and then a conversion:
//   mode 0  (y * 32767).clamp(-32768, 32767).to(int16): truncation toward zero (validate's denoised signal)
//   mode 1  (y * 32768).round().clamp(-32768, 32767):   round half to even (validate's converted clean signal)
// NaN gives 0 in both modes; +-inf clamps to 32767 / -32768.
__device__ __forceinline__ int16_t rg_quant(float v, int mode) {
  float w = mode == 0 ? v * 32767.f : rintf(v * 32768.f);
  if (!(w == w)) return 0;
  w = fminf(fmaxf(w, -32768.f), 32767.f);
  return (int16_t)(int)w;                        // w is finite here; mode 0 truncates, mode 1 is already an integer
}

// Clip b's n samples go to dst = out + off[b], which may start at any 2-byte position.  Chunk 0 is the head: the
// `head` samples in front of the first 16-byte boundary of dst; chunk c >= 1 is the 8 samples [head + 8 (c - 1), ...)
// behind it -- one 16-byte store where it is whole, 2-byte stores for the head and the tail.  `get(t)` is sample t as
// f32.  Nothing outside [dst, dst + n) is written.
template <typename Get>
__device__ __forceinline__ void rg_store_pcm16(int16_t *__restrict__ dst, int64_t n, int mode, Get get) {
  int64_t head = (int64_t)((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15) / 2;
  head = head > n ? n : head;
  const int64_t chunks = 1 + (n - head + 7) / 8;
  for (int64_t c = (int64_t)blockIdx.x * RT + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * RT) {
    const int64_t t0 = c == 0 ? 0 : head + 8 * (c - 1);
    const int64_t t1 = c == 0 ? head : (t0 + 8 < n ? t0 + 8 : n);
    if (c > 0 && t1 - t0 == 8) {
      rg_short8 q;
#pragma unroll
      for (int j = 0; j < 8; ++j) q[j] = rg_quant(get(t0 + j), mode);
      *reinterpret_cast<rg_short8 *>(dst + t0) = q;
    } else {
      for (int64_t t = t0; t < t1; ++t) dst[t] = rg_quant(get(t), mode);
    }
  }
}

// grid (workgroups along the clip, B): cum_unframe_rows_ragged with the quantising store.
template <typename T>
__global__ __launch_bounds__(RT) void unframe_rows_ragged_pcm16_kernel(const T *__restrict__ rows, int64_t Lmax, int64_t Tn,
                                                                      const int32_t *__restrict__ len,
                                                                      const float *__restrict__ s, int mode,
                                                                      int16_t *__restrict__ out,
                                                                      const int64_t *__restrict__ off) {
  const int b = blockIdx.y;
  int64_t n = len[b];
  n = n < 0 ? 0 : (n > Lmax ? Lmax : n);
  n = n > Tn ? Tn : n;
  const int64_t o = off[b];
  if (o < 0) return;
  const float sc = s ? s[b] : 1.f;
  const T *__restrict__ src = rows + (1 + (int64_t)b * (Tn + 2)) * 8;
  rg_store_pcm16(out + o, n, mode, [&](int64_t t) { return (float)src[t * 8] * sc; });
}

// grid (workgroups along the clip, B): f32 rows `stride` apart (the output of cum_resample_ragged) -> the flat buffer.
__global__ __launch_bounds__(RT) void pcm16_from_f32_ragged_kernel(const float *__restrict__ x, int64_t Lmax, int64_t stride,
                                                                  const int32_t *__restrict__ len, int mode,
                                                                  int16_t *__restrict__ out,
                                                                  const int64_t *__restrict__ off) {
  const int b = blockIdx.y;
  int64_t n = len[b];
  n = n < 0 ? 0 : (n > Lmax ? Lmax : n);
  const int64_t o = off[b];
  if (o < 0) return;
  const float *__restrict__ row = x + (int64_t)b * stride;
  rg_store_pcm16(out + o, n, mode, [&](int64_t t) { return row[t]; });
}

static unsigned rg_grid(int64_t items) {
  int64_t g = (items + RT - 1) / RT;
  return (unsigned)(g < 1 ? 1 : (g > 256 ? 256 : g));
}

}  // namespace cum

using namespace cum;

#define RG_BATCH_OK(batch) ((batch) >= 1 && (batch) <= 65534)

extern "C" int cum_clip_std_ragged(int32_t src_i16, const void *x, int32_t batch, int64_t lmax, int64_t stride,
                                   const int32_t *len, float eps, float *out, void *stream) {
  CUM_REQUIRE(src_i16 == 0 || src_i16 == 1, "clip_std_ragged: src_i16 must be 0 (f32 rows) or 1 (int16 rows)");
  CUM_REQUIRE(RG_BATCH_OK(batch), "clip_std_ragged: batch must be in [1, 65534]");
  CUM_REQUIRE(lmax >= 1, "clip_std_ragged: lmax must be at least 1");
  CUM_REQUIRE(stride >= lmax, "clip_std_ragged: stride must be at least lmax");
  CUM_REQUIRE(x && len && out, "clip_std_ragged: null pointer");
  CUM_REQUIRE((reinterpret_cast<uintptr_t>(x) & (src_i16 ? 1 : 3)) == 0 && (reinterpret_cast<uintptr_t>(len) & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(out) & 3) == 0, "clip_std_ragged: x, len or out is misaligned");
  hipStream_t st = (hipStream_t)stream;
  if (src_i16)
    hipLaunchKernelGGL(std_ragged_kernel<int16_t>, dim3(batch), dim3(RS), 0, st, (const int16_t *)x, stride, lmax, len, eps, out);
  else
    hipLaunchKernelGGL(std_ragged_kernel<float>, dim3(batch), dim3(RS), 0, st, (const float *)x, stride, lmax, len, eps, out);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}

template <typename S>
static void rg_launch_frame(int32_t dtype, const S *x, int32_t batch, int64_t lmax, int64_t stride, const int32_t *len,
                            int64_t T, int64_t R, const float *scale, void *out, hipStream_t st) {
  const int64_t slack = R - (int64_t)batch * (T + 2);
  const int64_t per = (T + 2 + 7) / 8;
  const dim3 g(rg_grid(per > slack ? per : slack), (unsigned)batch + 1), b(RT);
  if (dtype == CUM_F32)
    hipLaunchKernelGGL((frame_rows_ragged_kernel<float, S>), g, b, 0, st, x, stride, lmax, batch, len, T, R, scale, (float *)out);
  else if (dtype == CUM_BF16)
    hipLaunchKernelGGL((frame_rows_ragged_kernel<__bf16, S>), g, b, 0, st, x, stride, lmax, batch, len, T, R, scale, (__bf16 *)out);
  else
    hipLaunchKernelGGL((frame_rows_ragged_kernel<f16, S>), g, b, 0, st, x, stride, lmax, batch, len, T, R, scale, (f16 *)out);
}

extern "C" int cum_frame_rows_ragged(int32_t dtype, int32_t src_i16, const void *x, int32_t batch, int64_t lmax,
                                     int64_t stride, const int32_t *len, int64_t T, int64_t total_rows,
                                     const float *scale, void *out, void *stream) {
  CUM_REQUIRE(dtype_ok(dtype), "frame_rows_ragged: bad dtype");
  CUM_REQUIRE(src_i16 == 0 || src_i16 == 1, "frame_rows_ragged: src_i16 must be 0 (f32 rows) or 1 (int16 rows)");
  CUM_REQUIRE(RG_BATCH_OK(batch), "frame_rows_ragged: batch must be in [1, 65534]");
  CUM_REQUIRE(lmax >= 1, "frame_rows_ragged: lmax must be at least 1");
  CUM_REQUIRE(T >= lmax && stride >= lmax, "frame_rows_ragged: T and stride must be at least lmax");
  CUM_REQUIRE(total_rows >= 1 + (int64_t)batch * (T + 2), "frame_rows_ragged: row buffer too small");
  CUM_REQUIRE(x && len && out, "frame_rows_ragged: null pointer");
  CUM_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "frame_rows_ragged: out must be 16-byte aligned");
  CUM_REQUIRE((reinterpret_cast<uintptr_t>(x) & (src_i16 ? 1 : 3)) == 0 && (reinterpret_cast<uintptr_t>(len) & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(scale) & 3) == 0, "frame_rows_ragged: x, len or scale is misaligned");
  hipStream_t st = (hipStream_t)stream;
  if (src_i16)
    rg_launch_frame(dtype, (const int16_t *)x, batch, lmax, stride, len, T, total_rows, scale, out, st);
  else
    rg_launch_frame(dtype, (const float *)x, batch, lmax, stride, len, T, total_rows, scale, out, st);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}

extern "C" int cum_rows_zero_tail(int32_t dtype, void *rows, int32_t batch, int64_t T, int32_t cp, const int32_t *valid,
                                  void *stream) {
  CUM_REQUIRE(dtype_ok(dtype), "rows_zero_tail: bad dtype");
  CUM_REQUIRE(RG_BATCH_OK(batch), "rows_zero_tail: batch must be in [1, 65534]");
  CUM_REQUIRE(T >= 1, "rows_zero_tail: T must be at least 1");
  CUM_REQUIRE(cp >= 8 && cp % 8 == 0, "rows_zero_tail: the row width must be a positive multiple of 8 elements");
  CUM_REQUIRE(rows && valid, "rows_zero_tail: null pointer");
  CUM_REQUIRE((reinterpret_cast<uintptr_t>(rows) & 15) == 0 && (reinterpret_cast<uintptr_t>(valid) & 3) == 0,
              "rows_zero_tail: rows must be 16-byte aligned, valid 4-byte aligned");
  const int64_t row_chunks = (int64_t)cp * (dtype == CUM_F32 ? 4 : 2) / 16;
  uint4 *rows1 = static_cast<uint4 *>(rows) + row_chunks;          // row 1: the first clip's first row
  // at most 64 workgroups per clip: those whose share of the clip's tail is empty return at once
  int64_t gx = (T * row_chunks + RT - 1) / RT;
  gx = gx > 64 ? 64 : gx;
  hipLaunchKernelGGL(rows_zero_tail_kernel, dim3((unsigned)gx, (unsigned)batch), dim3(RT), 0, (hipStream_t)stream, rows1, T,
                     row_chunks, valid);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}

extern "C" int cum_unframe_rows_ragged(int32_t dtype, const void *rows, int32_t batch, int64_t lmax, int64_t T,
                                       const int32_t *len, const float *scale, float *y, void *stream) {
  CUM_REQUIRE(dtype_ok(dtype), "unframe_rows_ragged: bad dtype");
  CUM_REQUIRE(RG_BATCH_OK(batch), "unframe_rows_ragged: batch must be in [1, 65534]");
  CUM_REQUIRE(lmax >= 1, "unframe_rows_ragged: lmax must be at least 1");
  CUM_REQUIRE(T >= lmax, "unframe_rows_ragged: T must be at least lmax");
  CUM_REQUIRE(rows && len && y, "unframe_rows_ragged: null pointer");
  CUM_REQUIRE((reinterpret_cast<uintptr_t>(rows) & 15) == 0, "unframe_rows_ragged: rows must be 16-byte aligned");
  CUM_REQUIRE((reinterpret_cast<uintptr_t>(y) & 3) == 0 && (reinterpret_cast<uintptr_t>(len) & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(scale) & 3) == 0, "unframe_rows_ragged: y, len or scale is misaligned");
  hipStream_t st = (hipStream_t)stream;
  const dim3 g(rg_grid((lmax + 3) / 4), (unsigned)batch), b(RT);
  if (dtype == CUM_F32)
    hipLaunchKernelGGL(unframe_rows_ragged_kernel<float>, g, b, 0, st, (const float *)rows, lmax, T, len, scale, y);
  else if (dtype == CUM_BF16)
    hipLaunchKernelGGL(unframe_rows_ragged_kernel<__bf16>, g, b, 0, st, (const __bf16 *)rows, lmax, T, len, scale, y);
  else
    hipLaunchKernelGGL(unframe_rows_ragged_kernel<f16>, g, b, 0, st, (const f16 *)rows, lmax, T, len, scale, y);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}

#define RG_PCM16_TABLES_OK(len, out, off)                                                            \
  ((reinterpret_cast<uintptr_t>(len) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 1) == 0 &&     \
   (reinterpret_cast<uintptr_t>(off) & 7) == 0)

extern "C" int cum_unframe_rows_ragged_pcm16(int32_t dtype, const void *rows, int32_t batch, int64_t lmax, int64_t T,
                                             const int32_t *len, const float *scale, int32_t mode, int16_t *out_i16,
                                             const int64_t *out_offset, void *stream) {
  CUM_REQUIRE(dtype_ok(dtype), "unframe_rows_ragged_pcm16: bad dtype");
  CUM_REQUIRE(RG_BATCH_OK(batch), "unframe_rows_ragged_pcm16: batch must be in [1, 65534]");
  CUM_REQUIRE(lmax >= 1, "unframe_rows_ragged_pcm16: lmax must be at least 1");
  CUM_REQUIRE(T >= lmax, "unframe_rows_ragged_pcm16: T must be at least lmax");
  CUM_REQUIRE(mode == 0 || mode == 1, "unframe_rows_ragged_pcm16: mode must be 0 (x 32767, truncate) or 1 (x 32768, round)");
  CUM_REQUIRE(rows && len && out_i16 && out_offset, "unframe_rows_ragged_pcm16: null pointer");
  CUM_REQUIRE((reinterpret_cast<uintptr_t>(rows) & 15) == 0, "unframe_rows_ragged_pcm16: rows must be 16-byte aligned");
  CUM_REQUIRE(RG_PCM16_TABLES_OK(len, out_i16, out_offset) && (reinterpret_cast<uintptr_t>(scale) & 3) == 0,
              "unframe_rows_ragged_pcm16: len, scale, out_i16 or out_offset is misaligned");
  hipStream_t st = (hipStream_t)stream;
  const dim3 g(rg_grid((lmax + 7) / 8 + 1), (unsigned)batch), b(RT);
  if (dtype == CUM_F32)
    hipLaunchKernelGGL(unframe_rows_ragged_pcm16_kernel<float>, g, b, 0, st, (const float *)rows, lmax, T, len, scale, mode,
                       out_i16, out_offset);
  else if (dtype == CUM_BF16)
    hipLaunchKernelGGL(unframe_rows_ragged_pcm16_kernel<__bf16>, g, b, 0, st, (const __bf16 *)rows, lmax, T, len, scale,
                       mode, out_i16, out_offset);
  else
    hipLaunchKernelGGL(unframe_rows_ragged_pcm16_kernel<f16>, g, b, 0, st, (const f16 *)rows, lmax, T, len, scale, mode,
                       out_i16, out_offset);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}

extern "C" int cum_pcm16_from_f32_ragged(const float *x, int32_t batch, int64_t lmax, int64_t stride, const int32_t *len,
                                         int32_t mode, int16_t *out_i16, const int64_t *out_offset, void *stream) {
  CUM_REQUIRE(RG_BATCH_OK(batch), "pcm16_from_f32_ragged: batch must be in [1, 65534]");
  CUM_REQUIRE(lmax >= 1, "pcm16_from_f32_ragged: lmax must be at least 1");
  CUM_REQUIRE(stride >= lmax, "pcm16_from_f32_ragged: stride must be at least lmax");
  CUM_REQUIRE(mode == 0 || mode == 1, "pcm16_from_f32_ragged: mode must be 0 (x 32767, truncate) or 1 (x 32768, round)");
  CUM_REQUIRE(x && len && out_i16 && out_offset, "pcm16_from_f32_ragged: null pointer");
  CUM_REQUIRE(RG_PCM16_TABLES_OK(len, out_i16, out_offset) && (reinterpret_cast<uintptr_t>(x) & 3) == 0,
              "pcm16_from_f32_ragged: x, len, out_i16 or out_offset is misaligned");
  const dim3 g(rg_grid((lmax + 7) / 8 + 1), (unsigned)batch), b(RT);
  hipLaunchKernelGGL(pcm16_from_f32_ragged_kernel, g, b, 0, (hipStream_t)stream, x, lmax, stride, len, mode, out_i16,
                     out_offset);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}
