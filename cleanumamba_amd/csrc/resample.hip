// Polyphase sample-rate conversion of a ragged batch for gfx950 (util/resample.py): what stands between a
// recording at 8 / 22.05 / 32 / 44.1 / 48 kHz and the 16 kHz model, in both directions.  The reference has none (it drops
// the rate torchaudio.load returns, src/util/dataset.py:203).
//
//   rate_in -> rate_out, g = gcd, up = rate_out / g, down = rate_in / g, taps h[0 .. 2H] (odd, symmetric, sum up)
//   y[m] = sum_n x[n] h[m down - n up + H]        over the n with 0 <= m down - n up + H <= 2H
//        = sum_{j < K} x[n_hi - j] h[r + j up],   c = m down + H, r = c mod up, n_hi = c / up, K = ceil((2H + 1) / up)
//
// The taps arrive as the polyphase table tab[r][j] = h[r + j up] (zero behind 2H), rows `table_pitch` floats apart, so
// that the K taps of one output are one contiguous row.  The sum of output m is ONE f32 fma chain over j = 0 .. K - 1 in
// that order: it depends on (m, up, down, H) and on nothing else -- not on the tile, the clip's place in the batch, its
// mates, or where a stream was cut (a sample outside the signal enters as 0 x h, which leaves the bits alone).
//
// A workgroup owns RS_TILE consecutive outputs of one clip.  It stages the input span they read (RS_TILE down / up + K
// samples) once in LDS as f32 -- 16-byte global loads, int16 scaled by 2^-15 there -- and each lane then walks its
// outputs' phase rows against the span.  Two routes, the same chains:
//   up <= 3 (48 k, 32 k, 8 k <-> 16 k): the tile's outputs are taken one phase class at a time (o = up v + k, k fixed), so
//     a whole wave reads ONE table row: the taps come through the scalar cache into SGPRs and cost neither LDS nor
//     vector-memory issue; a lane carries up to three outputs of the class, so a tap is fetched once for three fmas;
//   up > 3 (the 160/441-type ratios, tables of tens of KB): neighbouring outputs use different rows; every lane reads
//     its own row in place through L2, 16 bytes per load.
// Results are gathered in LDS and leave as whole coalesced rows.
#include "common.h"

namespace cum {

constexpr int RS_THREADS = 256;
constexpr int RS_TILE = 768;                 // outputs of one workgroup: 3 per thread, and a multiple of up = 1, 2, 3
constexpr int RS_UNIFORM_MAX_UP = 3;         // up to here a phase class fills whole waves (the scalar-tap route)
constexpr int RS_LDS_SPAN_FLOATS = 12288;    // 48 KB: the longest input span a tile may need
constexpr float kRsPcm = 1.f / 32768.f;

typedef short rs_short8 __attribute__((ext_vector_type(8)));
typedef float rs_float4 __attribute__((ext_vector_type(4)));

struct RsArgs {
  int64_t lmax, in_pitch, out_pitch, max_out;
  int32_t up, down, H, K, kp, ends, span_cap;
};

// floats of LDS the input span of one tile can need: K taps back from the last output's n_hi, plus the two chunks of
// slack that aligning the span's start to the row's 16-byte chunks costs
static inline int64_t rs_span_cap(int64_t up, int64_t down, int64_t K) {
  const int64_t dq = ((up - 1) + (int64_t)(RS_TILE - 1) * down) / up;
  return (K + dq + 16 + 7) / 8 * 8;
}

// x: rows of S; origin: [batch][2] = absolute input position of x_b[0], absolute output position of y_b[0] (or null);
// UP: the up factor on the scalar-tap route (1, 2, 3), 0 for any other.
template <typename S, int UP>
__global__ __launch_bounds__(RS_THREADS) void resample_ragged_kernel(const S *__restrict__ x, const int32_t *__restrict__ len,
                                                                    const int64_t *__restrict__ origin,
                                                                    const float *__restrict__ table, float *__restrict__ y,
                                                                    const RsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  constexpr int E = sizeof(S) == 2 ? 8 : 4;                 // samples of one 16-byte chunk
  const int b = blockIdx.y;
  int64_t n = len[b];
  n = n < 0 ? 0 : (n > a.lmax ? a.lmax : n);
  const int64_t in0 = origin ? origin[2 * b] : 0, out0 = origin ? origin[2 * b + 1] : 0;
  // outputs this clip has: all of the signal's when it ends here, else those no later sample can change
  const int64_t total = in0 + n;
  const int64_t all = (total * a.up + a.down - 1) / a.down;
  int64_t fin = total * a.up - a.H;
  fin = fin <= 0 ? 0 : (fin + a.down - 1) / a.down;
  int64_t n_out = (a.ends ? all : (fin < all ? fin : all)) - out0;
  n_out = n_out < 0 ? 0 : (n_out > a.max_out ? a.max_out : n_out);
  const int64_t t0 = (int64_t)blockIdx.x * RS_TILE;
  if (t0 >= n_out) return;
  const int nt = n_out - t0 < RS_TILE ? (int)(n_out - t0) : RS_TILE;

  const int64_t c0 = (out0 + t0) * a.down + a.H;            // >= 0
  const int64_t q0 = c0 / a.up;
  const int r0 = (int)(c0 - q0 * a.up);
  const int64_t rel_first = q0 - (a.K - 1) - in0;           // row index of the oldest sample the first output reads
  const int64_t rel_base = (rel_first >= 0 ? rel_first / E : -((-rel_first + E - 1) / E)) * E;   // floor to a chunk
  const int off = (int)(rel_first - rel_base);              // in [0, E)
  const int dq_last = (r0 + (nt - 1) * a.down) / a.up;
  int need = a.K + dq_last + off;                           // LDS floats the tile reads: [0, need)
  need = need > a.span_cap ? a.span_cap : need;             // (never: span_cap is sized for it)

  float *__restrict__ xs = rs_lds;
  float *__restrict__ ys = rs_lds + a.span_cap;             // the tile's RS_TILE results
  const S *__restrict__ row = x + (int64_t)b * a.in_pitch;
  const bool wide = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
  for (int c = threadIdx.x; c * E < need; c += RS_THREADS) {
    const int64_t s0 = rel_base + (int64_t)c * E;           // a multiple of E: the chunk is 16-byte aligned when the row is
    float v[E];
    if (wide && s0 >= 0 && s0 + E <= n) {
      if constexpr (sizeof(S) == 2) {
        const rs_short8 s = *reinterpret_cast<const rs_short8 *>(row + s0);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (float)s[j] * kRsPcm;
      } else {
        const rs_float4 s = *reinterpret_cast<const rs_float4 *>(row + s0);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = s[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < E; ++j) {
        float s = 0.f;                                      // before the signal, behind the clip's length: zero
        if (s0 + j >= 0 && s0 + j < n) s = sizeof(S) == 2 ? (float)row[s0 + j] * kRsPcm : (float)row[s0 + j];
        v[j] = s;
      }
    }
#pragma unroll
    for (int j = 0; j < E; j += 4)
      *reinterpret_cast<rs_float4 *>(xs + c * E + j) = rs_float4{v[j], v[j + 1], v[j + 2], v[j + 3]};
  }
  __syncthreads();
  const float *__restrict__ x0 = xs + (a.K - 1) + off;      // x[n_hi] of the tile's first output; output o: x0[dq(o)]
  if constexpr (UP > 0) {
    constexpr int PER = RS_TILE / UP;                       // outputs of one phase class
    constexpr int V = (PER + RS_THREADS - 1) / RS_THREADS;  // ... a lane carries of them
#pragma unroll 1
    for (int k = 0; k < UP; ++k) {
      // outputs o = UP v + k: c = c0 + o down, so r = (r0 + k down) mod UP for all of them and n_hi = q0 + v down + dk
      const int ck = r0 + k * a.down, dk = ck / UP, rk = ck - dk * UP;
      const float *__restrict__ hrow = table + rk * a.kp;   // wave-uniform: scalar loads
      const float *xp[V];
      float acc[V];
#pragma unroll
      for (int q = 0; q < V; ++q) {
        int v = (int)threadIdx.x + q * RS_THREADS;
        v = v < PER ? v : PER - 1;                          // (a lane without a q-th output recomputes the class's last)
        xp[q] = x0 + dk + v * a.down;
        acc[q] = 0.f;
      }
      int j = 0;
      for (; j + 8 <= a.K; j += 8) {
        float h[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) h[u] = hrow[j + u];
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
          for (int q = 0; q < V; ++q) acc[q] = __builtin_fmaf(xp[q][-j - u], h[u], acc[q]);
      }
      for (; j < a.K; ++j) {
        const float h = hrow[j];
#pragma unroll
        for (int q = 0; q < V; ++q) acc[q] = __builtin_fmaf(xp[q][-j], h, acc[q]);
      }
#pragma unroll
      for (int q = 0; q < V; ++q) {
        const int v = (int)threadIdx.x + q * RS_THREADS;
        if (v < PER) ys[UP * v + k] = acc[q];               // (slots at or behind nt are filled and never stored)
      }
    }
  } else {
    for (int o = threadIdx.x; o < nt; o += RS_THREADS) {
      const int cc = r0 + o * a.down;
      const int dq = cc / a.up;
      const int r = cc - dq * a.up;
      const float *__restrict__ hrow = table + r * a.kp;
      const float *__restrict__ xp = x0 + dq;
      float acc = 0.f;
      int j = 0;
      for (; j + 4 <= a.K; j += 4) {
        const rs_float4 h = *reinterpret_cast<const rs_float4 *>(hrow + j);
        acc = __builtin_fmaf(xp[-j], h[0], acc);
        acc = __builtin_fmaf(xp[-j - 1], h[1], acc);
        acc = __builtin_fmaf(xp[-j - 2], h[2], acc);
        acc = __builtin_fmaf(xp[-j - 3], h[3], acc);
      }
      for (; j < a.K; ++j) acc = __builtin_fmaf(xp[-j], hrow[j], acc);
      ys[o] = acc;
    }
  }
  __syncthreads();
  float *__restrict__ dst = y + (int64_t)b * a.out_pitch + t0;
  for (int o = threadIdx.x; o < nt; o += RS_THREADS) dst[o] = ys[o];
}

template <typename S>
static void rs_launch(const void *x, const int32_t *len, const int64_t *origin, const float *table, float *y,
                      const RsArgs &a, dim3 g, size_t lds, hipStream_t st) {
  const S *xr = static_cast<const S *>(x);
  const dim3 t(RS_THREADS);
  if (a.up == 1)
    hipLaunchKernelGGL((resample_ragged_kernel<S, 1>), g, t, lds, st, xr, len, origin, table, y, a);
  else if (a.up == 2)
    hipLaunchKernelGGL((resample_ragged_kernel<S, 2>), g, t, lds, st, xr, len, origin, table, y, a);
  else if (a.up == 3)
    hipLaunchKernelGGL((resample_ragged_kernel<S, 3>), g, t, lds, st, xr, len, origin, table, y, a);
  else
    hipLaunchKernelGGL((resample_ragged_kernel<S, 0>), g, t, lds, st, xr, len, origin, table, y, a);
}

}  // namespace cum

using namespace cum;

extern "C" int32_t cum_resample_tile(void) { return RS_TILE; }

extern "C" int cum_resample_ragged(int32_t src_i16, const void *x, int32_t batch, int64_t lmax, int64_t in_pitch,
                                   const int32_t *len, const int64_t *origin, int32_t ends, int32_t up, int32_t down,
                                   int32_t n_taps, int32_t K, const float *table, int32_t table_pitch, float *y,
                                   int64_t out_pitch, int64_t max_out, void *stream) {
  CUM_REQUIRE(src_i16 == 0 || src_i16 == 1, "resample_ragged: src_i16 must be 0 (f32 rows) or 1 (int16 rows)");
  CUM_REQUIRE(batch >= 1 && batch <= 65534, "resample_ragged: batch must be in [1, 65534]");
  CUM_REQUIRE(up >= 1 && down >= 1, "resample_ragged: up and down must be at least 1");
  CUM_REQUIRE(up <= 1024 && down <= 1024, "resample_ragged: up and down must be at most 1024 (reduce the ratio)");
  CUM_REQUIRE(n_taps >= 1 && (n_taps & 1) == 1, "resample_ragged: the tap count must be odd (taps h[0 .. 2H])");
  CUM_REQUIRE(K >= 1 && (int64_t)K * up >= n_taps, "resample_ragged: K * up is smaller than the tap count");
  CUM_REQUIRE(table_pitch >= K && table_pitch % 4 == 0,
              "resample_ragged: table_pitch must be a multiple of 4 floats and at least K");
  CUM_REQUIRE(table != nullptr, "resample_ragged: null table");
  CUM_REQUIRE(lmax >= 0 && in_pitch >= 0 && out_pitch >= 0 && max_out >= 0,
              "resample_ragged: negative pitch or length");
  CUM_REQUIRE(in_pitch >= lmax && out_pitch >= max_out, "resample_ragged: a pitch is smaller than its row's length");
  CUM_REQUIRE(len != nullptr && y != nullptr && (x != nullptr || lmax == 0), "resample_ragged: null pointer");
  CUM_REQUIRE((reinterpret_cast<uintptr_t>(table) & 15) == 0, "resample_ragged: table must be 16-byte aligned");
  CUM_REQUIRE((reinterpret_cast<uintptr_t>(x) & (src_i16 ? 1 : 3)) == 0 && (reinterpret_cast<uintptr_t>(len) & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(y) & 3) == 0 && (reinterpret_cast<uintptr_t>(origin) & 7) == 0,
              "resample_ragged: x, len, origin or y is misaligned");
  const int64_t span = rs_span_cap(up, down, K);
  CUM_REQUIRE(span <= RS_LDS_SPAN_FLOATS,
              "resample_ragged: the input span of one tile (tile * down / up + K samples) does not fit in LDS");
  if (max_out == 0) return CUM_OK;
  RsArgs a;
  a.lmax = lmax, a.in_pitch = in_pitch, a.out_pitch = out_pitch, a.max_out = max_out;
  a.up = up, a.down = down, a.H = (n_taps - 1) / 2, a.K = K, a.kp = table_pitch, a.ends = ends != 0, a.span_cap = (int32_t)span;
  static_assert(RS_UNIFORM_MAX_UP == 3 && RS_TILE % 6 == 0, "the scalar-tap route is instantiated for up = 1, 2, 3");
  const dim3 g((unsigned)cdiv64(max_out, RS_TILE), (unsigned)batch);
  const size_t lds = sizeof(float) * (size_t)(span + RS_TILE);
  if (src_i16)
    rs_launch<int16_t>(x, len, origin, table, y, a, g, lds, (hipStream_t)stream);
  else
    rs_launch<float>(x, len, origin, table, y, a, g, lds, (hipStream_t)stream);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}
