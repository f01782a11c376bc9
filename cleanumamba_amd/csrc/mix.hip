// Mixing stage for gfx950: speech and noise from two unpaired corpora become the train step's (clean, noisy) pair on the
// device, from the int16 rows the feeder uploads (training/mix.py).
//
//   cum_mix_pairs   the mixer of the DNS challenge's synthesiser: the noise is scaled to an SNR measured on the ACTIVE
//                   frames of speech and noise, the mixture is brought to a level in dBFS, and a guard keeps it from
//                   clipping.  The reference trains from pre-mixed pairs only (src/util/dataset.py:108-150).
//
// Three launches, all over (tiles along the row, batch rows); the int16 rows are read three times, the floats written once:
//   sums    a workgroup takes a whole number of frames (a multiple of 4, at least 4096 samples), one frame per wave at a
//           time: eight samples per lane and 16-byte load, sum S^2, sum N^2, sum S N per lane in int64, a butterfly over
//           the wave per frame, the frame's activity decided in integers, and the workgroup's seven totals through LDS to
//           the workspace.  Every sum is an exact integer, so no order matters.
//   peak    every workgroup adds its row's totals (wave 0, a handful of loads), forms a in f64 and takes
//           max |fmaf(a, N 2^-15, S 2^-15)| over its tile of 2048 samples.
//   write   every workgroup forms a again, the level gain g from the totals and the row's peak, applies the guard and
//           writes its tile of both outputs with 16-byte stores; workgroup 0 of a row writes the row's stats.
// No atomics, nothing on the host, no transcendental: 10^(x / 10) of every setting arrives in the record.
#include "common.h"

namespace cum {

constexpr int MT = 256;                  // threads per workgroup
constexpr int MV = 8;                    // samples per lane and 16-byte load
constexpr int MTILE = MT * MV;           // samples per workgroup of the peak and write launches
constexpr int MSPAN = 4096;              // fewest samples per workgroup of the sums launch
constexpr int MWAVES = MT / CUM_WAVE;
constexpr int MPART = 8;                 // int64 per workgroup of the sums launch: the seven totals below, then 0
constexpr float kMixScale = 1.f / 32768.f;

// one record of 12 int32 per row (training/mix.py: REC_*)
enum MixField { MIX_N_SPEECH, MIX_FRAME, MIX_THR, MIX_Q = 4, MIX_L = 6, MIX_CLIP = 8, MIX_REC_INTS = 12 };
enum MixTotal { MIX_SS, MIX_SNN, MIX_SSN, MIX_ACT_ES, MIX_ACT_MS, MIX_ACT_EN, MIX_ACT_MN };

typedef short short8m __attribute__((ext_vector_type(8)));
typedef float float4m __attribute__((ext_vector_type(4)));

struct MixRow {
  const int16_t *speech, *noise;
  int64_t n_s, frame, thr;               // clamped: a bad table can never index outside a row
  double q, l;
  float clip;
};

__device__ __forceinline__ MixRow mix_row(const int16_t *__restrict__ pcm, int64_t pitch, const int32_t *__restrict__ recs,
                                          int batch, int b, int64_t len) {
  const int32_t *rec = recs + (int64_t)b * MIX_REC_INTS;
  MixRow r;
  r.speech = pcm + (int64_t)b * pitch;
  r.noise = pcm + (int64_t)(batch + b) * pitch;
  int64_t n = rec[MIX_N_SPEECH], f = rec[MIX_FRAME];
  r.n_s = n < 1 ? 1 : (n > len ? len : n);
  r.frame = f < 1 ? 1 : (f > len ? len : f);
  const int64_t thr = *reinterpret_cast<const int64_t *>(rec + MIX_THR);
  r.thr = thr < 0 ? 0 : (thr > (1 << 30) ? (1 << 30) : thr);       // (a frame's mean square is at most 2^30)
  r.q = *reinterpret_cast<const double *>(rec + MIX_Q);
  r.l = *reinterpret_cast<const double *>(rec + MIX_L);
  r.clip = __builtin_bit_cast(float, rec[MIX_CLIP]);
  return r;
}

// S[t0 .. t0 + 8) and N[t0 .. t0 + 8), t0 a multiple of 8 with t0 + 8 <= len: the noise and an untiled speech row by one
// 16-byte load each, a tiled speech row sample by sample (one division per eight samples)
__device__ __forceinline__ void mix_load8(const MixRow &r, int64_t len, int64_t t0, short8m &s, short8m &n) {
  n = *reinterpret_cast<const short8m *>(r.noise + t0);
  if (r.n_s == len) {                                              // wave-uniform: the whole row takes one path
    s = *reinterpret_cast<const short8m *>(r.speech + t0);
  } else {
    int64_t idx = t0 % r.n_s;
#pragma unroll
    for (int i = 0; i < MV; ++i) {
      s[i] = r.speech[idx];
      idx = idx + 1 == r.n_s ? 0 : idx + 1;
    }
  }
}

__device__ __forceinline__ int64_t wave_allsum(int64_t v) {
#pragma unroll
  for (int m = 1; m < CUM_WAVE; m <<= 1) v += __shfl_xor((long long)v, m);
  return v;
}

__device__ __forceinline__ float wave_allmax(float v) {
#pragma unroll
  for (int m = 1; m < CUM_WAVE; m <<= 1) v = fmaxf(v, __shfl_xor(v, m));
  return v;
}

// how the sums launch cuts a row: frames per workgroup (a multiple of the waves) and the samples they span
__device__ __forceinline__ int64_t mix_span(int64_t frame) {
  return (int64_t)MWAVES * ((MSPAN + MWAVES * frame - 1) / (MWAVES * frame)) * frame;
}

__global__ __launch_bounds__(MT) void mix_sums_kernel(const int16_t *__restrict__ pcm, int64_t pitch,
                                                     const int32_t *__restrict__ recs, int batch, int64_t len,
                                                     int64_t *__restrict__ parts) {
  __shared__ int64_t red[MWAVES][MPART];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & (CUM_WAVE - 1), wave = tid / CUM_WAVE;
  const MixRow r = mix_row(pcm, pitch, recs, batch, b, len);
  const int64_t span = mix_span(r.frame);
  const int64_t w0 = (int64_t)blockIdx.x * span;
  if (w0 >= len) return;                                           // (uniform) the grid is sized for the shortest span
  const int64_t w1 = w0 + span < len ? w0 + span : len;
  int64_t ssn = 0;                                                 // per lane over all frames of this wave
  int64_t tot[MPART] = {0, 0, 0, 0, 0, 0, 0, 0};                   // wave-uniform
  for (int64_t f0 = w0 + wave * r.frame; f0 < w1; f0 += MWAVES * r.frame) {
    const int64_t f1 = f0 + r.frame < len ? f0 + r.frame : len;
    int64_t es = 0, en = 0;
    for (int64_t c = (f0 >> 3) + lane; c <= ((f1 - 1) >> 3); c += CUM_WAVE) {
      const int64_t t0 = c * MV;
      if (t0 >= f0 && t0 + MV <= f1) {
        short8m s, n;
        mix_load8(r, len, t0, s, n);
#pragma unroll
        for (int i = 0; i < MV; ++i) {
          const int si = s[i], ni = n[i];
          es += (int64_t)(si * si), en += (int64_t)(ni * ni), ssn += (int64_t)(si * ni);
        }
      } else {                                                     // the ragged ends of a frame
        const int64_t ta = t0 > f0 ? t0 : f0, tb = t0 + MV < f1 ? t0 + MV : f1;
        int64_t idx = ta % r.n_s;
        for (int64_t t = ta; t < tb; ++t) {
          const int si = r.speech[idx], ni = r.noise[t];
          idx = idx + 1 == r.n_s ? 0 : idx + 1;
          es += (int64_t)(si * si), en += (int64_t)(ni * ni), ssn += (int64_t)(si * ni);
        }
      }
    }
    es = wave_allsum(es), en = wave_allsum(en);
    const int64_t m = f1 - f0;
    tot[MIX_SS] += es, tot[MIX_SNN] += en;
    if (es > r.thr * m) tot[MIX_ACT_ES] += es, tot[MIX_ACT_MS] += m;
    if (en > r.thr * m) tot[MIX_ACT_EN] += en, tot[MIX_ACT_MN] += m;
  }
  tot[MIX_SSN] = wave_allsum(ssn);
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < MPART; ++q) red[wave][q] = tot[q];
  }
  __syncthreads();
  if (tid < MPART) {
    int64_t v = 0;
#pragma unroll
    for (int w = 0; w < MWAVES; ++w) v += red[w][tid];
    parts[((int64_t)b * gridDim.x + blockIdx.x) * MPART + tid] = v;
  }
}

struct MixScalars {
  float a32, ps, pn, share_s, share_n;
  double em;
};

// The row's totals and what follows from them, by one whole wave (every lane returns the same values).  `parts`: the
// row's workgroup totals of the sums launch.
__device__ __forceinline__ MixScalars mix_scalars(const MixRow &r, int64_t len, const int64_t *__restrict__ parts,
                                                  int lane) {
#pragma clang fp contract(off)
  const int64_t nwg = (len + mix_span(r.frame) - 1) / mix_span(r.frame);
  const int q = lane & (MPART - 1);
  int64_t acc = 0;
  for (int64_t i = lane / MPART; i < nwg; i += CUM_WAVE / MPART) acc += parts[i * MPART + q];
#pragma unroll
  for (int m = MPART; m < CUM_WAVE; m <<= 1) acc += __shfl_xor((long long)acc, m);
  double tot[MPART - 1];
#pragma unroll
  for (int j = 0; j < MPART - 1; ++j) tot[j] = (double)(int64_t)__shfl((long long)acc, j);
  const double n = (double)len;
  const double ps = tot[MIX_ACT_MS] > 0.0 ? tot[MIX_ACT_ES] / tot[MIX_ACT_MS] : tot[MIX_SS] / n;
  const double pn = tot[MIX_ACT_MN] > 0.0 ? tot[MIX_ACT_EN] / tot[MIX_ACT_MN] : tot[MIX_SNN] / n;
  double a = 1.0;
  if (ps > 0.0 && pn > 0.0 && __builtin_isfinite(r.q) && r.q > 0.0) a = sqrt(ps / (pn * r.q));
  MixScalars s;
  s.a32 = (float)a;
  const double A = (double)s.a32;
  s.em = (A * tot[MIX_SNN] + 2.0 * tot[MIX_SSN]) * A + tot[MIX_SS];
  s.ps = (float)(ps * (1.0 / 1073741824.0));
  s.pn = (float)(pn * (1.0 / 1073741824.0));
  s.share_s = (float)(tot[MIX_ACT_MS] / n);
  s.share_n = (float)(tot[MIX_ACT_MN] / n);
  return s;
}

__global__ __launch_bounds__(MT) void mix_peak_kernel(const int16_t *__restrict__ pcm, int64_t pitch,
                                                     const int32_t *__restrict__ recs, int batch, int64_t len,
                                                     const int64_t *__restrict__ parts, int64_t parts_row,
                                                     float *__restrict__ peaks) {
  __shared__ float sh_a;
  __shared__ float red[MWAVES];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & (CUM_WAVE - 1), wave = tid / CUM_WAVE;
  const MixRow r = mix_row(pcm, pitch, recs, batch, b, len);
  if (wave == 0) {
    const MixScalars s = mix_scalars(r, len, parts + (int64_t)b * parts_row, lane);
    if (lane == 0) sh_a = s.a32;
  }
  __syncthreads();
  const float a = sh_a;
  const int64_t t0 = (int64_t)blockIdx.x * MTILE + (int64_t)tid * MV;
  float pk = 0.f;
  if (t0 + MV <= len) {
    short8m s, n;
    mix_load8(r, len, t0, s, n);
#pragma unroll
    for (int i = 0; i < MV; ++i) pk = fmaxf(pk, fabsf(fmaf(a, (float)n[i] * kMixScale, (float)s[i] * kMixScale)));
  } else if (t0 < len) {
    int64_t idx = t0 % r.n_s;
    for (int64_t t = t0; t < len; ++t) {
      pk = fmaxf(pk, fabsf(fmaf(a, (float)r.noise[t] * kMixScale, (float)r.speech[idx] * kMixScale)));
      idx = idx + 1 == r.n_s ? 0 : idx + 1;
    }
  }
  pk = wave_allmax(pk);
  if (lane == 0) red[wave] = pk;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < MWAVES; ++w) pk = fmaxf(pk, red[w]);
    peaks[(int64_t)b * gridDim.x + blockIdx.x] = pk;
  }
}

__global__ __launch_bounds__(MT) void mix_write_kernel(const int16_t *__restrict__ pcm, int64_t pitch,
                                                      const int32_t *__restrict__ recs, int batch, int64_t len,
                                                      const int64_t *__restrict__ parts, int64_t parts_row,
                                                      const float *__restrict__ peaks, float *__restrict__ clean,
                                                      int64_t clean_sb, float *__restrict__ noisy, int64_t noisy_sb,
                                                      float *__restrict__ stats) {
  __shared__ float sh_a, sh_g;
  __shared__ float red[MWAVES];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & (CUM_WAVE - 1), wave = tid / CUM_WAVE;
  const MixRow r = mix_row(pcm, pitch, recs, batch, b, len);
  float pk = 0.f;                                                  // the row's peak: the tiles' peaks, any order
  for (unsigned i = tid; i < gridDim.x; i += MT) pk = fmaxf(pk, peaks[(int64_t)b * gridDim.x + i]);
  pk = wave_allmax(pk);
  if (lane == 0) red[wave] = pk;
  __syncthreads();
  if (wave == 0) {
#pragma clang fp contract(off)
    const MixScalars s = mix_scalars(r, len, parts + (int64_t)b * parts_row, lane);
#pragma unroll
    for (int w = 0; w < MWAVES; ++w) pk = fmaxf(pk, red[w]);
    double g = 1.0;
    if (__builtin_isfinite(r.l) && s.em > 0.0) g = sqrt(r.l * (double)len * 1073741824.0 / s.em);
    float g32 = (float)g;
    const bool guard = g32 * pk > r.clip;
    if (guard) g32 = r.clip / pk;
    if (lane == 0) {
      sh_a = s.a32, sh_g = g32;
      if (stats != nullptr && blockIdx.x == 0) {
        float *o = stats + (int64_t)b * 8;
        o[0] = s.a32, o[1] = g32, o[2] = s.ps, o[3] = s.pn, o[4] = pk, o[5] = s.share_s, o[6] = s.share_n;
        o[7] = guard ? 1.f : 0.f;
      }
    }
  }
  __syncthreads();
  const float a = sh_a, g = sh_g;
  float *__restrict__ dc = clean + (int64_t)b * clean_sb;
  float *__restrict__ dn = noisy + (int64_t)b * noisy_sb;
  const int64_t t0 = (int64_t)blockIdx.x * MTILE + (int64_t)tid * MV;
  if (t0 + MV <= len) {
    short8m s, n;
    mix_load8(r, len, t0, s, n);
    float c[MV], y[MV];
#pragma unroll
    for (int i = 0; i < MV; ++i) {
      const float sf = (float)s[i] * kMixScale;
      c[i] = g * sf;
      y[i] = g * fmaf(a, (float)n[i] * kMixScale, sf);
    }
    if (((reinterpret_cast<uintptr_t>(dc) | reinterpret_cast<uintptr_t>(dn)) & 15) == 0) {       // wave-uniform
      const float4m c0 = {c[0], c[1], c[2], c[3]}, c1 = {c[4], c[5], c[6], c[7]};
      const float4m y0 = {y[0], y[1], y[2], y[3]}, y1 = {y[4], y[5], y[6], y[7]};
      reinterpret_cast<float4m *>(dc + t0)[0] = c0;
      reinterpret_cast<float4m *>(dc + t0)[1] = c1;
      reinterpret_cast<float4m *>(dn + t0)[0] = y0;
      reinterpret_cast<float4m *>(dn + t0)[1] = y1;
    } else {
#pragma unroll
      for (int i = 0; i < MV; ++i) dc[t0 + i] = c[i], dn[t0 + i] = y[i];
    }
  } else if (t0 < len) {
    int64_t idx = t0 % r.n_s;
    for (int64_t t = t0; t < len; ++t) {
      const float sf = (float)r.speech[idx] * kMixScale;
      idx = idx + 1 == r.n_s ? 0 : idx + 1;
      dc[t] = g * sf;
      dn[t] = g * fmaf(a, (float)r.noise[t] * kMixScale, sf);
    }
  }
}

}  // namespace cum

using namespace cum;

extern "C" int64_t cum_mix_workspace_elems(int32_t batch, int64_t len) {
  if (batch < 1 || len < 1) return 0;
  // per row: MPART int64 per workgroup of the sums launch, one float per tile of the peak launch; counted in floats, even
  const int64_t n = (int64_t)batch * (2 * MPART * cdiv64(len, MSPAN) + cdiv64(len, MTILE));
  return n + (n & 1);
}

extern "C" int cum_mix_pairs(const int16_t *pcm, int64_t pitch, const int32_t *recs, int32_t batch, int64_t len,
                             void *workspace, float *clean, int64_t clean_sb, float *noisy, int64_t noisy_sb,
                             float *stats, void *stream) {
  CUM_REQUIRE(batch >= 1, "mix_pairs: batch must be at least 1");
  CUM_REQUIRE(batch <= 32767, "mix_pairs: batch must be at most 32767 (rows on the grid's y axis)");
  CUM_REQUIRE(len >= 1, "mix_pairs: len must be at least 1");
  CUM_REQUIRE(pitch >= len, "mix_pairs: pitch must be at least len");
  CUM_REQUIRE(pitch % 8 == 0, "mix_pairs: pitch must be a multiple of 8 samples (16-byte rows)");
  CUM_REQUIRE(clean_sb >= len && noisy_sb >= len, "mix_pairs: clean_sb and noisy_sb must be at least len");
  CUM_REQUIRE(pcm && recs && workspace && clean && noisy, "mix_pairs: null pointer");
  CUM_REQUIRE(((reinterpret_cast<uintptr_t>(pcm) | reinterpret_cast<uintptr_t>(clean) |
                reinterpret_cast<uintptr_t>(noisy)) & 15) == 0,
              "mix_pairs: pcm, clean and noisy must be 16-byte aligned");
  CUM_REQUIRE(((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(recs)) & 7) == 0,
              "mix_pairs: workspace and recs must be 8-byte aligned");
  CUM_REQUIRE((reinterpret_cast<uintptr_t>(stats) & 3) == 0, "mix_pairs: stats must be 4-byte aligned");
  const int64_t g1 = cdiv64(len, MSPAN), g2 = cdiv64(len, MTILE);
  CUM_REQUIRE(g2 <= 0x7fffffff, "mix_pairs: len is beyond the grid's x axis");
  int64_t *parts = reinterpret_cast<int64_t *>(workspace);
  float *peaks = reinterpret_cast<float *>(parts + (int64_t)batch * g1 * MPART);
  const dim3 block(MT);
  hipLaunchKernelGGL(mix_sums_kernel, dim3((unsigned)g1, (unsigned)batch), block, 0, (hipStream_t)stream, pcm, pitch, recs,
                     (int)batch, len, parts);
  CUM_CHECK_LAUNCH();
  hipLaunchKernelGGL(mix_peak_kernel, dim3((unsigned)g2, (unsigned)batch), block, 0, (hipStream_t)stream, pcm, pitch, recs,
                     (int)batch, len, parts, g1 * MPART, peaks);
  CUM_CHECK_LAUNCH();
  hipLaunchKernelGGL(mix_write_kernel, dim3((unsigned)g2, (unsigned)batch), block, 0, (hipStream_t)stream, pcm, pitch, recs,
                     (int)batch, len, parts, g1 * MPART, peaks, clean, clean_sb, noisy, noisy_sb, stats);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}
