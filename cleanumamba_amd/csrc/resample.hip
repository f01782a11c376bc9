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
#include <stdio.h>

#include <vector>

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

// The int32 fields of a plan row and of the slots and feeder records, as include/cleanumamba_hip.h describes them
enum RsPlanField { kPlUp, kPlDown, kPlTaps, kPlK, kPlPitch, kPlOffset, kRsPlanInts = 8 };
enum RsSlotField { kSlSlot, kSlPlan, kSlNHist, kSlXRow, kSlNNew, kSlNOut, kSlYRow, kSlEnds, kSlKeep, kSlParity, kSlYCol };
enum RsFeedField { kFdPlan, kFdNSrc, kFdM, kFdN };
enum { kRsRecIn0 = 12, kRsRecOut0 = 14, kRsRecInts = 16 };   // both records: the int64 positions, the size
constexpr int64_t kRsPosMax = INT64_MAX >> 12;               // 2^51: the largest position a record may carry

// an int64 position of a record (records are 8-byte aligned, on the host as on the device)
__host__ __device__ __forceinline__ int64_t rs_pos(const int32_t *rec, const int field) {
  int64_t v;
  __builtin_memcpy(&v, __builtin_assume_aligned(rec + field, 8), sizeof v);
  return v;
}

// outputs of `total` samples: all at the signal's end, else the final ones (early returns: the ragged kernels' SGPRs)
__host__ __device__ inline int64_t rs_final_outputs(int64_t total, int64_t up, int64_t down, int64_t H, bool ends) {
  const int64_t all = (total * up + down - 1) / down;
  if (ends) return all;
  const int64_t part = total * up - H;
  if (part <= 0) return 0;
  const int64_t fin = (part + down - 1) / down;
  return fin < all ? fin : all;
}

// position of the oldest sample output out0 reads: its n_hi less the K - 1 taps behind it
__host__ __device__ inline int64_t rs_first_tap(int64_t out0, int64_t up, int64_t down, int64_t H, int64_t K) {
  return (out0 * down + H) / up - (K - 1);
}

// The input span of one tile: outputs m0 .. m0 + nt - 1 of a signal whose staged row starts at absolute position in0.
//   r0: c mod up of the first output;  rel_base: row index of the first staged sample, the oldest sample the first output
//   reads floored to a chunk of E samples;  off: what the flooring added, in [0, E);  need: LDS floats the tile reads.
struct RsTile { int r0, off, need; int64_t rel_base; };
template <int E>
__device__ __forceinline__ RsTile rs_tile_geometry(const int64_t m0, const int nt, const int64_t in0, const int up,
                                                   const int down, const int H, const int K, const int span_cap) {
  RsTile t;
  const int64_t c0 = m0 * down + H;                         // >= 0
  t.r0 = (int)(c0 - c0 / up * up);
  const int64_t rel_first = rs_first_tap(m0, up, down, H, K) - in0;
  t.rel_base = (rel_first >= 0 ? rel_first / E : -((-rel_first + E - 1) / E)) * E;   // floor to a chunk
  t.off = (int)(rel_first - t.rel_base);
  const int need = K + (t.r0 + (nt - 1) * down) / up + t.off;
  t.need = need > span_cap ? span_cap : need;               // (never: span_cap is sized for it)
  return t;
}

// Stage row[rel_base, rel_base + need) as f32 in xs, 16 bytes per load where the chunk lies inside [0, n) and the row is
// 16-byte aligned (`wide`); before the signal and behind its n samples: zero.  int16 is scaled by 2^-15.
template <typename S>
__device__ __forceinline__ void rs_stage_span(float *__restrict__ xs, const S *__restrict__ row, const int64_t n,
                                              const int64_t rel_base, const int need, const bool wide) {
  constexpr int E = sizeof(S) == 2 ? 8 : 4;                 // samples of one 16-byte chunk
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
        float s = 0.f;
        if (s0 + j >= 0 && s0 + j < n) s = sizeof(S) == 2 ? (float)row[s0 + j] * kRsPcm : (float)row[s0 + j];
        v[j] = s;
      }
    }
#pragma unroll
    for (int j = 0; j < E; j += 4)
      *reinterpret_cast<rs_float4 *>(xs + c * E + j) = rs_float4{v[j], v[j + 1], v[j + 2], v[j + 3]};
  }
}

// The chains of one tile: outputs o = 0 .. nt - 1, output o = sum_{j < K} x0[dq(o) - j] table[r(o)][j] with
// c = r0 + o down, dq = c / up, r = c mod up, into ys[o].  x0: LDS, x[n_hi] of the tile's first output.  UP: the up factor
// on the scalar-tap route (1, 2, 3), 0 for any other.  Both entries' kernels run these, hence the same bits.
template <int UP>
__device__ __forceinline__ void rs_tile_chains(const float *__restrict__ x0, const float *__restrict__ table,
                                               float *__restrict__ ys, const int r0, const int nt, const int up,
                                               const int down, const int K, const int kp) {
  if constexpr (UP > 0) {
    constexpr int PER = RS_TILE / UP;                       // outputs of one phase class
    constexpr int V = (PER + RS_THREADS - 1) / RS_THREADS;  // ... a lane carries of them
#pragma unroll 1
    for (int k = 0; k < UP; ++k) {
      // outputs o = UP v + k: c = c0 + o down, so r = (r0 + k down) mod UP for all of them and n_hi = q0 + v down + dk
      const int ck = r0 + k * down, dk = ck / UP, rk = ck - dk * UP;
      const float *__restrict__ hrow = table + rk * kp;   // wave-uniform: scalar loads
      const float *xp[V];
      float acc[V];
#pragma unroll
      for (int q = 0; q < V; ++q) {
        int v = (int)threadIdx.x + q * RS_THREADS;
        v = v < PER ? v : PER - 1;                          // (a lane without a q-th output recomputes the class's last)
        xp[q] = x0 + dk + v * down;
        acc[q] = 0.f;
      }
      int j = 0;
      for (; j + 8 <= K; j += 8) {
        float h[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) h[u] = hrow[j + u];
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
          for (int q = 0; q < V; ++q) acc[q] = __builtin_fmaf(xp[q][-j - u], h[u], acc[q]);
      }
      for (; j < K; ++j) {
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
      const int cc = r0 + o * down;
      const int dq = cc / up;
      const int r = cc - dq * up;
      const float *__restrict__ hrow = table + r * kp;
      const float *__restrict__ xp = x0 + dq;
      float acc = 0.f;
      int j = 0;
      for (; j + 4 <= K; j += 4) {
        const rs_float4 h = *reinterpret_cast<const rs_float4 *>(hrow + j);
        acc = __builtin_fmaf(xp[-j], h[0], acc);
        acc = __builtin_fmaf(xp[-j - 1], h[1], acc);
        acc = __builtin_fmaf(xp[-j - 2], h[2], acc);
        acc = __builtin_fmaf(xp[-j - 3], h[3], acc);
      }
      for (; j < K; ++j) acc = __builtin_fmaf(xp[-j], hrow[j], acc);
      ys[o] = acc;
    }
  }
}

// ... with the route taken from `up` on the device (workgroup-uniform): for kernels whose workgroups differ in their pair
__device__ __forceinline__ void rs_tile_chains_any(const float *__restrict__ x0, const float *__restrict__ table,
                                                   float *__restrict__ ys, const int r0, const int nt, const int up,
                                                   const int down, const int K, const int kp) {
  if (up == 1)
    rs_tile_chains<1>(x0, table, ys, r0, nt, up, down, K, kp);
  else if (up == 2)
    rs_tile_chains<2>(x0, table, ys, r0, nt, up, down, K, kp);
  else if (up == 3)
    rs_tile_chains<3>(x0, table, ys, r0, nt, up, down, K, kp);
  else
    rs_tile_chains<0>(x0, table, ys, r0, nt, up, down, K, kp);
}

// x: rows of S; origin: [batch][2] = absolute input position of x_b[0], absolute output position of y_b[0] (or null);
// UP: the up factor on the scalar-tap route (1, 2, 3), 0 for any other.
template <typename S, int UP>
__global__ __launch_bounds__(RS_THREADS) void resample_ragged_kernel(const S *__restrict__ x, const int32_t *__restrict__ len,
                                                                    const int64_t *__restrict__ origin,
                                                                    const float *__restrict__ table, float *__restrict__ y,
                                                                    const RsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  const int b = blockIdx.y;
  int64_t n = len[b];
  n = n < 0 ? 0 : (n > a.lmax ? a.lmax : n);
  const int64_t in0 = origin ? origin[2 * b] : 0, out0 = origin ? origin[2 * b + 1] : 0;
  int64_t n_out = rs_final_outputs(in0 + n, a.up, a.down, a.H, a.ends) - out0;
  n_out = n_out < 0 ? 0 : (n_out > a.max_out ? a.max_out : n_out);
  const int64_t t0 = (int64_t)blockIdx.x * RS_TILE;
  if (t0 >= n_out) return;
  const int nt = n_out - t0 < RS_TILE ? (int)(n_out - t0) : RS_TILE;
  const RsTile t = rs_tile_geometry<sizeof(S) == 2 ? 8 : 4>(out0 + t0, nt, in0, a.up, a.down, a.H, a.K, a.span_cap);
  float *__restrict__ xs = rs_lds;
  float *__restrict__ ys = rs_lds + a.span_cap;             // the tile's RS_TILE results
  const S *__restrict__ row = x + (int64_t)b * a.in_pitch;
  rs_stage_span(xs, row, n, t.rel_base, t.need, (reinterpret_cast<uintptr_t>(row) & 15) == 0);
  __syncthreads();
  const float *__restrict__ x0 = xs + (a.K - 1) + t.off;    // x[n_hi] of the tile's first output; output o: x0[dq(o)]
  rs_tile_chains<UP>(x0, table, ys, t.r0, nt, a.up, a.down, a.K, a.kp);
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

// ---- slots: streams of different rates at different positions in one launch (cum_resample_slots) --------------------
// What the stream pool converts with (network/streampool.py): every slot keeps, per direction, the last
// inputs an unfinished output may still read.  hist: [capacity][2][hist_pitch] f32 -- TWO rows per slot; a record reads
// row `parity` and writes the next history to row `1 - parity`, so the workgroups of a record (one per tile of its
// outputs) never read what one of them writes, in whatever order they run.  The signal a record sees is
// hist[slot][parity][0, n_hist) ++ x[x_row][0, n_new), its first sample at absolute position in0.  Plan rows
// (RsPlanField) and records (RsSlotField): include/cleanumamba_hip.h, cum_resample_slots.
__global__ __launch_bounds__(RS_THREADS) void resample_slots_kernel(const int32_t *__restrict__ recs,
                                                                   const int32_t *__restrict__ plans,
                                                                   const float *__restrict__ tables, float *hist,
                                                                   const int64_t hist_pitch, const float *__restrict__ x,
                                                                   const int64_t x_pitch, float *__restrict__ y,
                                                                   const int64_t y_pitch, const int span_cap) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  const int32_t *__restrict__ rec = recs + (int64_t)blockIdx.y * kRsRecInts;      // workgroup-uniform, as all below
  const int slot = rec[kSlSlot], n_hist = rec[kSlNHist], n_new = rec[kSlNNew], n_out = rec[kSlNOut];
  const int keep = rec[kSlKeep], parity = rec[kSlParity];
  const int tiles = (n_out + RS_TILE - 1) / RS_TILE;
  const int tile = blockIdx.x, last = tiles > 0 ? tiles - 1 : 0;
  if (tile > last) return;
  const int32_t *__restrict__ pl = plans + (int64_t)rec[kSlPlan] * kRsPlanInts;
  const int up = pl[kPlUp], down = pl[kPlDown], H = (pl[kPlTaps] - 1) / 2, K = pl[kPlK], kp = pl[kPlPitch];
  const float *__restrict__ table = tables + pl[kPlOffset];
  const int64_t in0 = rs_pos(rec, kRsRecIn0), out0 = rs_pos(rec, kRsRecOut0);
  const float *hold = hist + ((int64_t)slot * 2 + parity) * hist_pitch;
  float *hnew = hist + ((int64_t)slot * 2 + (parity ^ 1)) * hist_pitch;
  const float *__restrict__ xr = x + (int64_t)rec[kSlXRow] * x_pitch;
  const int n = n_hist + n_new;                              // samples of the signal this record holds

  if (tile < tiles) {
    const int t0 = tile * RS_TILE;
    const int nt = n_out - t0 < RS_TILE ? n_out - t0 : RS_TILE;
    const RsTile t = rs_tile_geometry<1>(out0 + t0, nt, in0, up, down, H, K, span_cap);   // no chunks: off = 0
    float *__restrict__ xs = rs_lds;
    float *__restrict__ ys = rs_lds + span_cap;              // the tile's RS_TILE results
    for (int i = threadIdx.x; i < t.need; i += RS_THREADS) {
      const int64_t s = t.rel_base + i;
      float v = 0.f;                                         // before the signal, behind what has arrived: zero
      if (s >= 0 && s < n) v = s < n_hist ? hold[s] : xr[s - n_hist];
      xs[i] = v;
    }
    __syncthreads();
    rs_tile_chains_any(xs + (K - 1), table, ys, t.r0, nt, up, down, K, kp);   // xs[K - 1]: x[n_hi] of the first output
    __syncthreads();
    float *__restrict__ dst = y + (int64_t)rec[kSlYRow] * y_pitch + rec[kSlYCol] + t0;
    for (int o = threadIdx.x; o < nt; o += RS_THREADS) dst[o] = ys[o];
  }
  if (tile == last) {
    for (int t = threadIdx.x; t < keep; t += RS_THREADS) {
      const int s = n - keep + t;
      hnew[t] = s < n_hist ? hold[s] : xr[s - n_hist];
    }
  }
}

// ---- feeder: the train step's float batch from int16 windows at any mix of rates (cum_pcm_batch_resample_f32) --------
// What training/feeder.py assembles a rated batch with: cum_pcm_batch_f32's layout -- row b the clean
// clip, row batch + b the noisy clip, `pitch` int16 apart -- but a row holds the window of its file, at the file's rate,
// that the crop reads, and leaves as the model-rate crop in the step's input buffers.
//
// One record per PAIR (RsFeedField; include/cleanumamba_hip.h, cum_pcm_batch_resample_f32): plan -1 = the pair is at the
// model rate (up = down = K = 1, H = 0, the tap 1: y[m] = x[m]);  out[t] = y[(out0 + t) mod M], t < len.
// A workgroup owns RS_TILE outputs m = out0 + t0 + o of one row, computes each ONCE and stores it to every t = t0 + o + k M
// below len, so a tiled clip repeats bit for bit.
constexpr int RS_COPY_SPAN = RS_TILE + 8;    // LDS floats a tile of a model-rate row stages (its outputs + chunk slack)

// ys[0, n) -> dst[0, n) by the whole workgroup: 16-byte stores from dst's first 16-byte boundary on, elements around them
__device__ __forceinline__ void rs_store_run(float *__restrict__ dst, const float *__restrict__ ys, const int n) {
  int head = (int)((4 - ((reinterpret_cast<uintptr_t>(dst) >> 2) & 3)) & 3);
  head = head < n ? head : n;
  if ((int)threadIdx.x < head) dst[threadIdx.x] = ys[threadIdx.x];
  const int nv = (n - head) >> 2;
  for (int v = threadIdx.x; v < nv; v += RS_THREADS) {
    const int o = head + 4 * v;
    *reinterpret_cast<rs_float4 *>(dst + o) = rs_float4{ys[o], ys[o + 1], ys[o + 2], ys[o + 3]};
  }
  for (int o = head + 4 * nv + (int)threadIdx.x; o < n; o += RS_THREADS) dst[o] = ys[o];
}

// grid: (tiles of len, 2 * batch rows)
__global__ __launch_bounds__(RS_THREADS) void pcm_batch_resample_kernel(
    const int16_t *__restrict__ pcm, const int64_t pitch, const int32_t *__restrict__ recs,
    const int32_t *__restrict__ plans, const int n_plans, const float *__restrict__ tables, const int batch,
    const int64_t len, float *__restrict__ clean, const int64_t clean_sb, float *__restrict__ noisy,
    const int64_t noisy_sb, const int span_cap) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  const int r = blockIdx.y;
  const int b = r < batch ? r : r - batch;
  const int32_t *__restrict__ rec = recs + (int64_t)b * kRsRecInts;              // workgroup-uniform, as all below
  const int plan = rec[kFdPlan];
  if (plan < -1 || plan >= n_plans) return;
  // a bad table can never index outside a row: n in [0, pitch], M >= 1, positions in [0, 2^51], out0 < M
  int64_t n = rec[kFdNSrc], M = rec[kFdM];
  n = n < 0 ? 0 : (n > pitch ? pitch : n);
  M = M < 1 ? 1 : M;
  int64_t in0 = rs_pos(rec, kRsRecIn0), out0 = rs_pos(rec, kRsRecOut0);
  in0 = in0 < 0 ? 0 : (in0 > kRsPosMax ? kRsPosMax : in0);
  out0 = out0 < 0 ? 0 : (out0 > M - 1 ? M - 1 : out0);
  const int64_t cnt = M - out0 < len ? M - out0 : len;       // distinct outputs the row needs: y[out0, out0 + cnt)
  const int64_t t0 = (int64_t)blockIdx.x * RS_TILE;
  if (t0 >= cnt) return;
  int nt = cnt - t0 < RS_TILE ? (int)(cnt - t0) : RS_TILE;

  int up = 1, down = 1, H = 0, K = 1, kp = 4;
  const float *__restrict__ table = tables;
  if (plan >= 0) {
    const int32_t *__restrict__ pl = plans + (int64_t)plan * kRsPlanInts;
    up = pl[kPlUp], down = pl[kPlDown], H = (pl[kPlTaps] - 1) / 2, K = pl[kPlK], kp = pl[kPlPitch];
    table = tables + pl[kPlOffset];
  }
  const RsTile t = rs_tile_geometry<8>(out0 + t0, nt, in0, up, down, H, K, span_cap);

  float *__restrict__ xs = rs_lds;
  float *ys = rs_lds + span_cap;                             // the tile's RS_TILE results
  rs_stage_span(xs, pcm + (int64_t)r * pitch, n, t.rel_base, t.need, true);      // 16-byte aligned: pitch % 8 == 0
  __syncthreads();
  if (plan < 0) {
    ys = xs + t.off;                                         // the model rate: output o IS staged sample o (exact)
  } else {
    rs_tile_chains_any(xs + (K - 1) + t.off, table, ys, t.r0, nt, up, down, K, kp);
    __syncthreads();
  }
  // a file that fits the tile and is repeated: lay whole periods side by side first, so the replicas leave in runs of
  // up to RS_TILE, not of M (copies: the bits of a period are those of the first)
  int64_t period = M;
  if (cnt < len && nt == M && 2 * nt <= RS_TILE) {
    const int wide = RS_TILE / nt * nt;
    for (int o = nt + threadIdx.x; o < wide; o += RS_THREADS) ys[o] = ys[o % nt];
    __syncthreads();
    nt = wide, period = wide;
  }
  float *__restrict__ dst = r < batch ? clean + (int64_t)b * clean_sb : noisy + (int64_t)b * noisy_sb;
  for (int64_t tb = t0; tb < len; tb += period)
    rs_store_run(dst + tb, ys, len - tb < nt ? (int)(len - tb) : nt);
}

// ---- host checks shared by the three entries: CUM_EINVAL with "<who>: <what>" as the error ----------------------------
static int rs_fail(const char *who, const char *what) {
  char msg[256];
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  cum_set_error(msg);
  return CUM_EINVAL;
}
#define RS_REQUIRE(cond, what)              /* in a function with a `who` */ \
  do {                                      \
    if (!(cond)) return rs_fail(who, what); \
  } while (0)

// the factors, tap count, K and table pitch of one pair; *span: the LDS floats its tile span needs, which must fit
static int rs_check_plan(const char *who, int64_t up, int64_t down, int64_t taps, int64_t K, int64_t kp, int64_t *span) {
  RS_REQUIRE(up >= 1 && down >= 1, "up and down must be at least 1");
  RS_REQUIRE(up <= 1024 && down <= 1024, "up and down must be at most 1024 (reduce the ratio)");
  RS_REQUIRE(taps >= 1 && (taps & 1) == 1, "the tap count must be odd (taps h[0 .. 2H])");
  RS_REQUIRE(K >= 1 && K * up >= taps, "K * up is smaller than the tap count");
  RS_REQUIRE(kp >= K && kp % 4 == 0, "table_pitch must be a multiple of 4 floats and at least K");
  *span = rs_span_cap(up, down, K);
  RS_REQUIRE(*span <= RS_LDS_SPAN_FLOATS, "the input span of one tile (tile * down / up + K samples) does not fit in LDS");
  return CUM_OK;
}

// every row of a plan table, and its table inside the blob; *span grows to the largest tile span of the plans
static int rs_check_plan_table(const char *who, const int32_t *plans_host, int32_t n_plans, int64_t table_floats,
                               int64_t *span) {
  for (int32_t i = 0; i < n_plans; ++i) {
    const int32_t *p = plans_host + (int64_t)i * kRsPlanInts;
    int64_t s;
    if (rs_check_plan(who, p[kPlUp], p[kPlDown], p[kPlTaps], p[kPlK], p[kPlPitch], &s)) return CUM_EINVAL;
    RS_REQUIRE(p[kPlOffset] >= 0 && p[kPlOffset] % 4 == 0 &&
                   p[kPlOffset] + (int64_t)p[kPlUp] * p[kPlPitch] <= table_floats,
               "a plan's table does not lie in the blob at a multiple of 4 floats");
    *span = s > *span ? s : *span;
  }
  return CUM_OK;
}

static int rs_check_positions(const char *who, int64_t in0, int64_t out0) {
  RS_REQUIRE(in0 >= 0 && out0 >= 0 && in0 <= kRsPosMax && out0 <= kRsPosMax, "a position is negative or beyond 2^51");
  return CUM_OK;
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
  int64_t span;
  if (rs_check_plan("resample_ragged", up, down, n_taps, K, table_pitch, &span)) return CUM_EINVAL;
  CUM_REQUIRE(table != nullptr, "resample_ragged: null table");
  CUM_REQUIRE(lmax >= 0 && in_pitch >= 0 && out_pitch >= 0 && max_out >= 0,
              "resample_ragged: negative pitch or length");
  CUM_REQUIRE(in_pitch >= lmax && out_pitch >= max_out, "resample_ragged: a pitch is smaller than its row's length");
  CUM_REQUIRE(len != nullptr && y != nullptr && (x != nullptr || lmax == 0), "resample_ragged: null pointer");
  CUM_REQUIRE((reinterpret_cast<uintptr_t>(table) & 15) == 0, "resample_ragged: table must be 16-byte aligned");
  CUM_REQUIRE((reinterpret_cast<uintptr_t>(x) & (src_i16 ? 1 : 3)) == 0 && (reinterpret_cast<uintptr_t>(len) & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(y) & 3) == 0 && (reinterpret_cast<uintptr_t>(origin) & 7) == 0,
              "resample_ragged: x, len, origin or y is misaligned");
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

extern "C" int cum_resample_slots(float *hist, int64_t hist_pitch, int32_t capacity, const int32_t *plans_host,
                                  const int32_t *plans, int32_t n_plans, const float *tables, int64_t table_floats,
                                  const int32_t *recs_host, const int32_t *recs, int32_t n_recs, const float *x,
                                  int32_t x_rows, int64_t x_pitch, float *y, int32_t y_rows, int64_t y_pitch,
                                  void *stream) {
  CUM_REQUIRE(capacity >= 1 && n_plans >= 1 && n_recs >= 0 && n_recs <= 65535,
              "resample_slots: capacity and n_plans must be at least 1, n_recs in [0, 65535]");
  CUM_REQUIRE(hist_pitch >= 0 && table_floats >= 0 && x_rows >= 0 && x_pitch >= 0 && y_rows >= 0 && y_pitch >= 0,
              "resample_slots: negative pitch or row count");
  CUM_REQUIRE(hist != nullptr && plans_host != nullptr && plans != nullptr && tables != nullptr &&
                  recs_host != nullptr && recs != nullptr && y != nullptr && (x != nullptr || x_rows == 0),
              "resample_slots: null pointer");
  CUM_REQUIRE((reinterpret_cast<uintptr_t>(tables) & 15) == 0, "resample_slots: tables must be 16-byte aligned");
  CUM_REQUIRE((reinterpret_cast<uintptr_t>(recs) & 7) == 0 && (reinterpret_cast<uintptr_t>(recs_host) & 7) == 0 &&
                  (reinterpret_cast<uintptr_t>(plans) & 3) == 0 && (reinterpret_cast<uintptr_t>(plans_host) & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(hist) & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(y) & 3) == 0,
              "resample_slots: hist, plans, recs, x or y is misaligned (records 8 bytes, the rest 4)");
  int64_t span = 0;
  if (rs_check_plan_table("resample_slots", plans_host, n_plans, table_floats, &span)) return CUM_EINVAL;
  if (n_recs == 0) return CUM_OK;
  std::vector<uint8_t> named((size_t)capacity, 0);
  int32_t tiles = 1;
  for (int32_t i = 0; i < n_recs; ++i) {
    const int32_t *r = recs_host + (int64_t)i * kRsRecInts;
    const int32_t slot = r[kSlSlot], plan = r[kSlPlan], n_hist = r[kSlNHist], x_row = r[kSlXRow], n_new = r[kSlNNew];
    const int32_t n_out = r[kSlNOut], y_row = r[kSlYRow], ends = r[kSlEnds], keep = r[kSlKeep], parity = r[kSlParity];
    const int32_t y_col = r[kSlYCol];
    const int64_t in0 = rs_pos(r, kRsRecIn0), out0 = rs_pos(r, kRsRecOut0);
    CUM_REQUIRE(slot >= 0 && slot < capacity, "resample_slots: a record names a slot outside the pool (slot < capacity)");
    CUM_REQUIRE(!named[slot], "resample_slots: a slot is named twice");
    named[slot] = 1;
    CUM_REQUIRE(plan >= 0 && plan < n_plans, "resample_slots: a record names a plan outside the table");
    CUM_REQUIRE(parity == 0 || parity == 1, "resample_slots: parity must be 0 or 1");
    CUM_REQUIRE(n_hist >= 0 && n_hist <= hist_pitch, "resample_slots: a history count does not fit the history row");
    CUM_REQUIRE(n_new >= 0 && n_new <= x_pitch && (n_new == 0 || (x_row >= 0 && x_row < x_rows)),
                "resample_slots: a chunk does not fit the rows of x");
    CUM_REQUIRE(keep >= 0 && keep <= hist_pitch && keep <= (int64_t)n_hist + n_new,
                "resample_slots: the history to keep does not fit the history row or exceeds the samples held");
    CUM_REQUIRE(n_out >= 0 && y_col >= 0 && (int64_t)y_col + n_out <= y_pitch &&
                    (n_out == 0 || (y_row >= 0 && y_row < y_rows)),
                "resample_slots: the outputs do not fit the rows of y");
    if (rs_check_positions("resample_slots", in0, out0)) return CUM_EINVAL;
    // the outputs asked for must exist: all of the signal's when it ends here, else those no later sample can change
    const int32_t *p = plans_host + (int64_t)plan * kRsPlanInts;
    const int64_t up = p[kPlUp], down = p[kPlDown], H = (p[kPlTaps] - 1) / 2, K = p[kPlK];
    CUM_REQUIRE(out0 + n_out <= rs_final_outputs(in0 + n_hist + n_new, up, down, H, ends != 0),
                "resample_slots: more outputs than the samples received make final");
    // ... and the history must reach back to the oldest sample the first of them reads
    CUM_REQUIRE(n_out == 0 || in0 == 0 || rs_first_tap(out0, up, down, H, K) >= in0,
                "resample_slots: the history starts behind the oldest sample the first output reads");
    const int32_t t = (n_out + RS_TILE - 1) / RS_TILE;
    tiles = t > tiles ? t : tiles;
  }
  const dim3 g((unsigned)tiles, (unsigned)n_recs);
  const size_t lds = sizeof(float) * (size_t)(span + RS_TILE);
  hipLaunchKernelGGL(resample_slots_kernel, g, dim3(RS_THREADS), lds, (hipStream_t)stream, recs, plans, tables, hist,
                     hist_pitch, x, x_pitch, y, y_pitch, (int)span);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}

extern "C" int cum_pcm_batch_resample_f32(const int16_t *pcm, int64_t pitch, const int32_t *recs_host, const int32_t *recs,
                                          int32_t batch, const int32_t *plans_host, const int32_t *plans, int32_t n_plans,
                                          const float *tables, int64_t table_floats, int64_t len, float *clean,
                                          int64_t clean_sb, float *noisy, int64_t noisy_sb, void *stream) {
  CUM_REQUIRE(batch >= 1, "pcm_batch_resample: batch must be at least 1");
  CUM_REQUIRE(batch <= 32767, "pcm_batch_resample: batch must be at most 32767 (2 * batch rows on the grid's y axis)");
  CUM_REQUIRE(len >= 1 && len <= (int64_t)RS_TILE * INT32_MAX, "pcm_batch_resample: len must be in [1, tile * 2^31)");
  CUM_REQUIRE(pitch >= 0 && pitch % 8 == 0, "pcm_batch_resample: pitch must be a multiple of 8 samples (16-byte rows)");
  CUM_REQUIRE(clean_sb >= len && noisy_sb >= len, "pcm_batch_resample: clean_sb and noisy_sb must be at least len");
  CUM_REQUIRE(n_plans >= 0 && table_floats >= 0, "pcm_batch_resample: negative plan count or table size");
  CUM_REQUIRE(pcm && recs_host && recs && clean && noisy, "pcm_batch_resample: null pointer");
  CUM_REQUIRE(n_plans == 0 || (plans_host && plans && tables), "pcm_batch_resample: null plan table or tap tables");
  CUM_REQUIRE(((reinterpret_cast<uintptr_t>(pcm) | reinterpret_cast<uintptr_t>(clean) | reinterpret_cast<uintptr_t>(noisy) |
                reinterpret_cast<uintptr_t>(tables)) & 15) == 0,
              "pcm_batch_resample: pcm, clean, noisy and tables must be 16-byte aligned");
  CUM_REQUIRE((reinterpret_cast<uintptr_t>(recs) & 7) == 0 && (reinterpret_cast<uintptr_t>(recs_host) & 7) == 0 &&
                  (reinterpret_cast<uintptr_t>(plans) & 3) == 0 && (reinterpret_cast<uintptr_t>(plans_host) & 3) == 0,
              "pcm_batch_resample: recs or plans is misaligned (records 8 bytes, plans 4)");
  int64_t span = RS_COPY_SPAN;
  if (rs_check_plan_table("pcm_batch_resample", plans_host, n_plans, table_floats, &span)) return CUM_EINVAL;
  for (int32_t i = 0; i < batch; ++i) {
    const int32_t *r = recs_host + (int64_t)i * kRsRecInts;
    const int32_t plan = r[kFdPlan];
    const int64_t n_src = r[kFdNSrc], M = r[kFdM], N = r[kFdN];
    const int64_t in0 = rs_pos(r, kRsRecIn0), out0 = rs_pos(r, kRsRecOut0);
    CUM_REQUIRE(plan >= -1 && plan < n_plans, "pcm_batch_resample: a record names a plan outside the table");
    CUM_REQUIRE(n_src >= 0 && n_src <= pitch, "pcm_batch_resample: pitch is smaller than a record's n_src");
    if (rs_check_positions("pcm_batch_resample", in0, out0)) return CUM_EINVAL;
    int64_t up = 1, down = 1, H = 0, K = 1;
    if (plan >= 0) {
      const int32_t *p = plans_host + (int64_t)plan * kRsPlanInts;
      up = p[kPlUp], down = p[kPlDown], H = (p[kPlTaps] - 1) / 2, K = p[kPlK];
    }
    CUM_REQUIRE(M >= 1 && N >= 1 && M == (N * up + down - 1) / down,
                "pcm_batch_resample: M must be at least 1 and the output count of the file's N samples");
    CUM_REQUIRE(out0 == 0 || out0 + len <= M, "pcm_batch_resample: out0 + len exceeds M for a crop that does not start at 0");
    CUM_REQUIRE(in0 + n_src <= N, "pcm_batch_resample: a window runs past the end of its file");
    // the window must hold every sample the distinct outputs y[out0, out0 + cnt) read (what lies outside the file is zero)
    const int64_t cnt = M - out0 < len ? M - out0 : len;
    const int64_t first = rs_first_tap(out0, up, down, H, K);
    int64_t last = ((out0 + cnt - 1) * down + H) / up;
    last = last < N - 1 ? last : N - 1;
    CUM_REQUIRE(in0 == 0 || in0 <= first,
                "pcm_batch_resample: a window starts behind the oldest sample its first output reads");
    CUM_REQUIRE(in0 + n_src - 1 >= last, "pcm_batch_resample: a window ends before the newest sample its last output reads");
  }
  const dim3 g((unsigned)cdiv64(len, RS_TILE), (unsigned)(2 * batch));
  const size_t lds = sizeof(float) * (size_t)(span + RS_TILE);
  hipLaunchKernelGGL(pcm_batch_resample_kernel, g, dim3(RS_THREADS), lds, (hipStream_t)stream, pcm, pitch, recs, plans,
                     (int)n_plans, tables, (int)batch, len, clean, clean_sb, noisy, noisy_sb, (int)span);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}
