// Training augmentation for gfx950, between the assembled float crops and the train step's inputs.
//
//   cum_augment_pairs   <- the hook `noise, clean_audio = augment((noise, clean_audio))` of the train loop
//                          (src/training/train.py:262-265): exchange the noises within the batch, shift noise against
//                          speech, add a synthetic room, re-draw the SNR and the level
//
// Two launches over a grid of (tiles of 2048 samples, batch rows):
//   mix     c1 = c0 + kappa rc into `clean`, n1 = n0 + rn + (1 - kappa) rc into `noisy`, and the tile's sums of c1^2 and
//           n1^2 in f64 to the workspace.  A row without taps moves eight samples per lane: the reads at t + offset take
//           16-, 8- or 4-byte loads as the address allows (wave-uniform), the stores are 16 bytes wherever the output row
//           starts on a 16-byte boundary.  A row with taps puts consecutive t on consecutive lanes, so that each tap is a
//           gather of one contiguous run per wave; the delays reach seconds, so the runs come from L2, not from LDS.
//   scale   every workgroup adds its row's tile sums in one fixed order, a = sqrt(Ec / (En 10^(snr/10))), and finishes
//           both buffers in place.
// With workspace == NULL (no row re-draws its SNR) the mix launch finishes the buffers itself.
// No atomics anywhere: every sum has one order, fixed by (len, the row's tap count) alone.
#include "common.h"

namespace cum {

constexpr int AT = 256;                  // threads per workgroup
constexpr int AV = 8;                    // samples per lane
constexpr int ATILE = AT * AV;           // samples per workgroup
constexpr int kAugMaxTaps = 512;

// one record of 8 int32 per row (training/augment.py: REC_*)
enum AugField { AUG_PERM, AUG_OFF_CLEAN, AUG_OFF_NOISE, AUG_N_TAPS, AUG_SNR_DB, AUG_GAIN, AUG_KAPPA, AUG_REC_INTS = 8 };

typedef float float4a __attribute__((ext_vector_type(4)));
typedef float float2a __attribute__((ext_vector_type(2)));

// eight consecutive floats from an address that is only 4-byte aligned by construction; the alignment is the same for
// every lane of the launch's row (the lanes are 32 bytes apart), so the branch is wave-uniform
__device__ __forceinline__ void load8(const float *__restrict__ p, float (&v)[AV]) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if ((a & 15) == 0) {
    const float4a lo = *reinterpret_cast<const float4a *>(p), hi = *reinterpret_cast<const float4a *>(p + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = lo[i], v[4 + i] = hi[i];
  } else if ((a & 7) == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float2a x = *reinterpret_cast<const float2a *>(p + 2 * i);
      v[2 * i] = x[0], v[2 * i + 1] = x[1];
    }
  } else {
#pragma unroll
    for (int i = 0; i < AV; ++i) v[i] = p[i];
  }
}

__device__ __forceinline__ void store8(float *__restrict__ p, const float (&v)[AV], bool wide) {
  if (wide) {
    float4a lo = {v[0], v[1], v[2], v[3]}, hi = {v[4], v[5], v[6], v[7]};
    reinterpret_cast<float4a *>(p)[0] = lo;
    reinterpret_cast<float4a *>(p)[1] = hi;
  } else {
#pragma unroll
    for (int i = 0; i < AV; ++i) p[i] = v[i];
  }
}

// sums of a and b over the workgroup in a fixed tree; every thread returns with the totals
__device__ __forceinline__ void block_sum2(double &a, double &b, double (*red)[AT]) {
  const int tid = threadIdx.x;
  red[0][tid] = a;
  red[1][tid] = b;
  __syncthreads();
  for (int s = AT / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red[0][tid] += red[0][tid + s];
      red[1][tid] += red[1][tid + s];
    }
    __syncthreads();
  }
  a = red[0][0];
  b = red[1][0];
}

__device__ __forceinline__ float rec_f32(const int32_t *rec, int field) { return __builtin_bit_cast(float, rec[field]); }

// FINAL: no row re-draws its SNR (a = 1): write clean' and noisy' at once, no sums
template <bool FINAL>
__global__ __launch_bounds__(AT) void augment_mix_kernel(const float *__restrict__ csrc, int64_t csrc_sb,
                                                        const float *__restrict__ ysrc, int64_t ysrc_sb, int batch,
                                                        int64_t len, int64_t src_len, const int32_t *__restrict__ recs,
                                                        const int32_t *__restrict__ tap_delay,
                                                        const float *__restrict__ tap_gain, int k_max,
                                                        double *__restrict__ parts, float *__restrict__ clean,
                                                        int64_t clean_sb, float *__restrict__ noisy, int64_t noisy_sb) {
  __shared__ double red[2][AT];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int32_t *rec = recs + (int64_t)b * AUG_REC_INTS;
  // a bad table can never index outside its rows: every index is clamped (src_len >= len was checked on the host)
  const int64_t room = src_len - len;
  int p = rec[AUG_PERM];
  p = p < 0 ? 0 : (p >= batch ? batch - 1 : p);
  int64_t oc = rec[AUG_OFF_CLEAN], on = rec[AUG_OFF_NOISE];
  oc = oc < 0 ? 0 : (oc > room ? room : oc);
  on = on < 0 ? 0 : (on > room ? room : on);
  int nt = rec[AUG_N_TAPS];
  nt = nt < 0 ? 0 : (nt > k_max ? k_max : nt);
  const float gain = rec_f32(rec, AUG_GAIN), kappa = rec_f32(rec, AUG_KAPPA);
  const float *__restrict__ cb = csrc + (int64_t)b * csrc_sb + oc;       // c0[t] = cb[t]
  const float *__restrict__ cp = csrc + (int64_t)p * csrc_sb + on;       // n0[t] = yp[t] - cp[t]
  const float *__restrict__ yp = ysrc + (int64_t)p * ysrc_sb + on;
  float *__restrict__ dc = clean + (int64_t)b * clean_sb;
  float *__restrict__ dn = noisy + (int64_t)b * noisy_sb;
  const int64_t tile0 = (int64_t)blockIdx.x * ATILE;
  double ec = 0.0, en = 0.0;

  if (nt == 0) {                                           // rc = rn = 0: c1 = c0, n1 = n0, eight samples per lane
    const int64_t t0 = tile0 + (int64_t)tid * AV;
    if (t0 + AV <= len) {
      float c[AV], y[AV], x[AV], oc1[AV], on1[AV];
      load8(cb + t0, c);
      load8(yp + t0, y);
      load8(cp + t0, x);
#pragma unroll
      for (int i = 0; i < AV; ++i) {
        const float c1 = c[i], n1 = y[i] - x[i];
        if (FINAL) {
          oc1[i] = gain * c1;
          on1[i] = gain * fmaf(1.f, n1, c1);
        } else {
          oc1[i] = c1, on1[i] = n1;
          ec += (double)c1 * (double)c1;
          en += (double)n1 * (double)n1;
        }
      }
      store8(dc + t0, oc1, (reinterpret_cast<uintptr_t>(dc) & 15) == 0);
      store8(dn + t0, on1, (reinterpret_cast<uintptr_t>(dn) & 15) == 0);
    } else {
      for (int64_t t = t0; t < len; ++t) {
        const float c1 = cb[t], n1 = yp[t] - cp[t];
        if (FINAL) {
          dc[t] = gain * c1;
          dn[t] = gain * fmaf(1.f, n1, c1);
        } else {
          dc[t] = c1, dn[t] = n1;
          ec += (double)c1 * (double)c1;
          en += (double)n1 * (double)n1;
        }
      }
    }
  } else {                                                 // the echo: consecutive t on consecutive lanes
    const int64_t tend = tile0 + ATILE < len ? tile0 + ATILE : len;      // this tile is [tile0, tend)
    const int32_t *__restrict__ dl = tap_delay + (int64_t)b * k_max;
    const float *__restrict__ gl = tap_gain + (int64_t)b * k_max;
    float c0[AV], n0[AV], rc[AV], rn[AV];
#pragma unroll
    for (int j = 0; j < AV; ++j) {
      const int64_t t = tile0 + j * AT + tid;
      rc[j] = rn[j] = c0[j] = n0[j] = 0.f;
      if (t < tend) c0[j] = cb[t], n0[j] = yp[t] - cp[t];
    }
    for (int k = 0; k < nt; ++k) {                         // k ascending: one fixed-order fma chain per sample
      const int64_t d = dl[k];
      const float g = gl[k];
      if (d < 1 || d >= tend) continue;                    // (uniform) no sample of this tile reaches back that far
      // no branch around the loads: a lane whose term is dropped reads sample 0 of its rows and keeps its sums, so the
      // 24 gathers of a tap are in flight together instead of eight dependent groups of three
      float xc[AV], xy[AV], xp[AV];
#pragma unroll
      for (int j = 0; j < AV; ++j) {
        const int64_t t = tile0 + j * AT + tid;
        const int64_t i = t < tend && t >= d ? t - d : 0;
        xc[j] = cb[i], xy[j] = yp[i], xp[j] = cp[i];
      }
#pragma unroll
      for (int j = 0; j < AV; ++j) {
        const int64_t t = tile0 + j * AT + tid;
        const bool on_row = t < tend && t >= d;
        rc[j] = on_row ? fmaf(g, xc[j], rc[j]) : rc[j];
        rn[j] = on_row ? fmaf(g, xy[j] - xp[j], rn[j]) : rn[j];
      }
    }
    const float one_minus_kappa = 1.f - kappa;
#pragma unroll
    for (int j = 0; j < AV; ++j) {
      const int64_t t = tile0 + j * AT + tid;
      if (t < tend) {
        const float c1 = fmaf(kappa, rc[j], c0[j]);
        const float n1 = fmaf(one_minus_kappa, rc[j], n0[j] + rn[j]);
        if (FINAL) {
          dc[t] = gain * c1;
          dn[t] = gain * fmaf(1.f, n1, c1);
        } else {
          dc[t] = c1, dn[t] = n1;
          ec += (double)c1 * (double)c1;
          en += (double)n1 * (double)n1;
        }
      }
    }
  }
  if (!FINAL) {
    block_sum2(ec, en, red);
    if (tid == 0) {
      double *o = parts + ((int64_t)b * gridDim.x + blockIdx.x) * 2;
      o[0] = ec, o[1] = en;
    }
  }
}

// clean' = gain c1, noisy' = gain (c1 + a n1) in place; a from the row's tile sums, added in one fixed order
__global__ __launch_bounds__(AT) void augment_scale_kernel(int64_t len, const int32_t *__restrict__ recs,
                                                          const double *__restrict__ parts, float *__restrict__ clean,
                                                          int64_t clean_sb, float *__restrict__ noisy, int64_t noisy_sb) {
  __shared__ double red[2][AT];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int32_t *rec = recs + (int64_t)b * AUG_REC_INTS;
  const float gain = rec_f32(rec, AUG_GAIN), snr_db = rec_f32(rec, AUG_SNR_DB);
  const double *row = parts + (int64_t)b * gridDim.x * 2;
  double ec = 0.0, en = 0.0;
  for (unsigned i = tid; i < gridDim.x; i += AT) ec += row[2 * (int64_t)i], en += row[2 * (int64_t)i + 1];
  block_sum2(ec, en, red);
  float a = 1.f;
  if (__builtin_isfinite(snr_db) && ec > 0.0 && en > 0.0) a = (float)sqrt(ec / (en * pow(10.0, (double)snr_db / 10.0)));

  float *__restrict__ dc = clean + (int64_t)b * clean_sb;
  float *__restrict__ dn = noisy + (int64_t)b * noisy_sb;
  const int64_t t0 = (int64_t)blockIdx.x * ATILE + (int64_t)tid * AV;
  const bool wide = ((reinterpret_cast<uintptr_t>(dc) | reinterpret_cast<uintptr_t>(dn)) & 15) == 0;
  if (t0 + AV <= len && wide) {
    float c[AV], n[AV];
    load8(dc + t0, c);
    load8(dn + t0, n);
#pragma unroll
    for (int i = 0; i < AV; ++i) {
      n[i] = gain * fmaf(a, n[i], c[i]);
      c[i] = gain * c[i];
    }
    store8(dc + t0, c, true);
    store8(dn + t0, n, true);
  } else {
    const int64_t t1 = t0 + AV < len ? t0 + AV : len;
    for (int64_t t = t0; t < t1; ++t) {
      const float c1 = dc[t], n1 = dn[t];
      dc[t] = gain * c1;
      dn[t] = gain * fmaf(a, n1, c1);
    }
  }
}

}  // namespace cum

using namespace cum;

extern "C" int64_t cum_augment_workspace_elems(int32_t batch, int64_t len) {
  if (batch < 1 || len < 1) return 0;
  return 4 * (int64_t)batch * cdiv64(len, ATILE);          // two f64 sums per tile and row, counted in floats
}

extern "C" int cum_augment_pairs(const float *clean_src, int64_t clean_src_sb, const float *noisy_src,
                                 int64_t noisy_src_sb, int32_t batch, int64_t len, int64_t src_len, const int32_t *recs,
                                 const int32_t *tap_delay, const float *tap_gain, int32_t k_max, float *workspace,
                                 float *clean, int64_t clean_sb, float *noisy, int64_t noisy_sb, void *stream) {
  CUM_REQUIRE(batch >= 1, "augment_pairs: batch must be at least 1");
  CUM_REQUIRE(batch <= 32767, "augment_pairs: batch must be at most 32767 (rows on the grid's y axis)");
  CUM_REQUIRE(len >= 1, "augment_pairs: len must be at least 1");
  CUM_REQUIRE(src_len >= len, "augment_pairs: src_len must be at least len (len plus the largest offset)");
  CUM_REQUIRE(k_max >= 0 && k_max <= kAugMaxTaps, "augment_pairs: k_max must be in [0, 512]");
  CUM_REQUIRE(clean_src_sb >= src_len && noisy_src_sb >= src_len,
              "augment_pairs: clean_src_sb and noisy_src_sb must be at least src_len");
  CUM_REQUIRE(clean_sb >= len && noisy_sb >= len, "augment_pairs: clean_sb and noisy_sb must be at least len");
  CUM_REQUIRE(clean_src && noisy_src && recs && clean && noisy, "augment_pairs: null pointer");
  CUM_REQUIRE(k_max == 0 || (tap_delay && tap_gain), "augment_pairs: null pointer (tap_delay, tap_gain with k_max > 0)");
  CUM_REQUIRE(((reinterpret_cast<uintptr_t>(clean) | reinterpret_cast<uintptr_t>(noisy)) & 15) == 0,
              "augment_pairs: clean and noisy must be 16-byte aligned");
  CUM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "augment_pairs: workspace must be 8-byte aligned");
  CUM_REQUIRE(((reinterpret_cast<uintptr_t>(clean_src) | reinterpret_cast<uintptr_t>(noisy_src) |
                reinterpret_cast<uintptr_t>(recs) | reinterpret_cast<uintptr_t>(tap_delay) |
                reinterpret_cast<uintptr_t>(tap_gain)) & 3) == 0,
              "augment_pairs: clean_src, noisy_src, recs, tap_delay and tap_gain must be 4-byte aligned");
  const int64_t gx = cdiv64(len, ATILE);
  CUM_REQUIRE(gx <= 0x7fffffff, "augment_pairs: len is beyond the grid's x axis");
  const dim3 grid((unsigned)gx, (unsigned)batch), block(AT);
  double *parts = reinterpret_cast<double *>(workspace);
  if (parts == nullptr) {
    hipLaunchKernelGGL(augment_mix_kernel<true>, grid, block, 0, (hipStream_t)stream, clean_src, clean_src_sb, noisy_src,
                       noisy_src_sb, (int)batch, len, src_len, recs, tap_delay, tap_gain, (int)k_max, parts, clean,
                       clean_sb, noisy, noisy_sb);
    CUM_CHECK_LAUNCH();
    return CUM_OK;
  }
  hipLaunchKernelGGL(augment_mix_kernel<false>, grid, block, 0, (hipStream_t)stream, clean_src, clean_src_sb, noisy_src,
                     noisy_src_sb, (int)batch, len, src_len, recs, tap_delay, tap_gain, (int)k_max, parts, clean,
                     clean_sb, noisy, noisy_sb);
  CUM_CHECK_LAUNCH();
  hipLaunchKernelGGL(augment_scale_kernel, grid, block, 0, (hipStream_t)stream, len, recs, parts, clean, clean_sb, noisy,
                     noisy_sb);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}
