// Speech-quality metrics of a ragged batch of int16 clips (reference src/util/python_eval.py, pystoi.stoi).
//
//   metrics_frames_kernel   per 30 ms frame (480 samples, hop 120, 16 kHz): segmental SNR (:409 snr), LLR of order-16
//                           LPC (:336 llr, :380 lpcoeff; f64 throughout), WSS (:139 wss; 1024-point FFT in LDS)
//                           metrics_frames_kernel<true>: on the same frames, LPC, FFT and bands, the LPC cepstrum distance
//                           and the frequency-weighted segmental SNR of Hu & Loizou 2008 (tests/metrics_ext_ref.py)
//   metrics_sums_kernel / metrics_sums_reduce_kernel   per clip: exact int64 sum x^2, sum y^2, sum x y (overall SNR, SI-SDR)
//   metrics_rank_kernel / metrics_clip_mean_kernel   per clip: mean of the lowest round(0.95 n) frame values (NaN sorts
//                           last, as np.sort puts it), or the plain mean
//   stoi_*_kernel           STOI (Taal et al. 2011): polyphase 16 k -> 10 k, silent-frame removal, 512-point STFT in LDS,
//                           15 one-third-octave bands, 30-frame segments; stoi_ecorr_kernel: eSTOI (Jensen & Taal 2016)
//                           on the same band magnitudes
// Every sum runs in a fixed order inside one clip's own workgroups: two runs give the same bits, and a clip's result does
// not depend on the other clips of its batch.  No float atomics.
#include <math.h>
#include <vector>
#include "fft_lds.h"

namespace cum {

constexpr int kWin = 480, kHop = 120, kBands = 25, kLpc = 16;   // python_eval.py: round(30 ms * 16 kHz), winlength / 4
constexpr int kFpb = 16;                                         // frames per workgroup (one 75 %-overlapped span)
constexpr int kSpanCap = ((kFpb - 1) * kHop + kWin + 7 + 7) / 8 * 8;   // + up to 7 samples of 16-byte alignment
constexpr int kMetricWaves = 4;
constexpr double kEpsF64 = 2.220446049250313e-16;                // np.spacing(1) = np.finfo(float).eps

// one row per clip, uploaded to the workspace by the host entry
struct ClipRow {
  int64_t off, len, frame_off, n_frames, keep, aux0, aux1, aux2;
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// hi + lo += a * b without rounding the product or the running sum away (TwoProd by fma, TwoSum).  The LLR divides two
// quadratic forms of nearly equal size over an ill-conditioned Toeplitz matrix: plain f64 sums leave errors of a few
// 1e-6 in it on full-scale frames, these leave the f64 rounding of the result.
__device__ __forceinline__ void dd_add_prod(double &hi, double &lo, double a, double b) {
#pragma clang fp contract(off)
  const double p = a * b, pe = fma(a, b, -p);
  const double s = hi + p, bb = s - hi, e = (hi - (s - bb)) + (p - bb);
  hi = s;
  lo += e + pe;
}

// span of int16 samples [g0, g0 + n) -> LDS floats (exact), 16-byte loads from the aligned base below g0.  Returns the
// LDS index of sample g0.  Never reads at or past n_samples.
__device__ __forceinline__ int load_span(const int16_t *__restrict__ sig, int64_t n_samples, int64_t g0, int n, float *dst) {
  const int64_t a = g0 & ~(int64_t)7;
  const int lead = (int)(g0 - a), nch = (lead + n + 7) / 8;
  for (int q = threadIdx.x; q < nch; q += blockDim.x) {
    const int64_t s = a + 8 * (int64_t)q;
    if (s + 8 <= n_samples) {
      const int4 v = *reinterpret_cast<const int4 *>(sig + s);
      const int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        dst[8 * q + 2 * i] = (float)(int16_t)(w[i] & 0xffff);
        dst[8 * q + 2 * i + 1] = (float)(int16_t)((uint32_t)w[i] >> 16);
      }
    } else {
      for (int i = 0; i < 8; ++i) dst[8 * q + i] = s + i < n_samples ? (float)sig[s + i] : 0.f;
    }
  }
  return lead;
}

struct FrameParams {
  const int16_t *clean, *proc;
  int64_t n_samples;
  const ClipRow *clips;
  const double *window;        // [480] 0.5 (1 - cos(2 pi n / 481)), n = 1..480
  const int32_t *band_tab;     // [25][3] first bin, bin count, offset into band_w
  const double *band_w;        // truncated Gaussian weights of every band's support
  const double *tw;            // e^{-2 pi i m / 1024}, m = 0..512
  double *seg_snr, *llr, *wss;
  double *cep, *fwseg;         // the extended instantiation's outputs
};

template <bool EXT>
struct FramePw { typedef float2 T; };                    // bin powers of both signals, f32 (WSS)
template <>
struct FramePw<true> { typedef double2 T; };             // bin magnitudes, f64: fwseg subtracts two nearly equal band sums

// limits that keep a NaN (fmin / fmax would drop it)
__device__ __forceinline__ double limit_keep_nan(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// grid (ceil(max frames / kFpb), clips), 4 waves; each wave owns one frame at a time.  EXT = false: segSNR, LLR, WSS.
// EXT = true: the same staging, autocorrelation, Levinson recursion, FFT and band table, then the LPC cepstrum distance
// and the frequency-weighted segmental SNR (Hu & Loizou 2008) instead of the quadratic forms and the WSS peak search.
template <bool EXT>
__global__ __launch_bounds__(64 * kMetricWaves) void metrics_frames_kernel(const FrameParams p) {
  typedef FusedFft<512, double> F;
  __shared__ __attribute__((aligned(16))) float s_c[kSpanCap];
  __shared__ __attribute__((aligned(16))) float s_p[kSpanCap];
  __shared__ double s_win[kWin];
  __shared__ __attribute__((aligned(16))) double4 s_buf[kMetricWaves][F::SLOTS];
  __shared__ double2 s_tw[513];
  __shared__ typename FramePw<EXT>::T s_pw[kMetricWaves][512];
  __shared__ double s_R[kMetricWaves][2][kLpc + 1];
  __shared__ double s_A[kMetricWaves][2][kLpc + 1];
  __shared__ double s_E[kMetricWaves][2][kBands];

  const ClipRow clip = p.clips[blockIdx.y];
  const int64_t f0 = (int64_t)blockIdx.x * kFpb;
  if (f0 >= clip.n_frames) return;
  const int nfr = (int)min((int64_t)kFpb, clip.n_frames - f0);
  const int span = (nfr - 1) * kHop + kWin;
  const int64_t g0 = clip.off + f0 * kHop;
  const int lead = load_span(p.clean, p.n_samples, g0, span, s_c);
  load_span(p.proc, p.n_samples, g0, span, s_p);
  for (int i = threadIdx.x; i < kWin; i += blockDim.x) s_win[i] = p.window[i];
  for (int i = threadIdx.x; i <= 512; i += blockDim.x) s_tw[i] = reinterpret_cast<const double2 *>(p.tw)[i];
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = uniform(threadIdx.x >> 6);
  double4 *buf = s_buf[wave];
  double *xw = reinterpret_cast<double *>(buf);          // [0, 480) clean * window, [480, 960) processed * window (f64)
  for (int fl = wave; fl < nfr; fl += kMetricWaves) {
    const int b0 = lead + fl * kHop;
    const int64_t fo = clip.frame_off + f0 + fl;
    // ---- segmental SNR and the autocorrelation lags, on the f64 windowed frames
    double sig = 0.0, noi = 0.0;
    for (int n = lane; n < kWin; n += 64) {
      const double c = (double)s_c[b0 + n] * s_win[n], q = (double)s_p[b0 + n] * s_win[n];
      xw[n] = c;
      xw[kWin + n] = q;
      sig += c * c;
      noi += (c - q) * (c - q);
    }
    sig = wave_sum_f64(sig);
    noi = wave_sum_f64(noi);
    F::stage_fence();
    if (lane < 2 * (kLpc + 1)) {                         // one (signal, lag) per lane, an ordered compensated dot product
      const int s = lane / (kLpc + 1), k = lane - s * (kLpc + 1);
      const double *x = xw + s * kWin;
      double hi = 0.0, lo = 0.0;
      for (int n = 0; n < kWin - k; ++n) dd_add_prod(hi, lo, x[n], x[n + k]);
      s_R[wave][s][k] = hi + lo;
    }
    F::stage_fence();
    if (lane < 2) {                                      // Levinson-Durbin as lpcoeff (lane 0 clean, lane 1 processed)
      const double *R = s_R[wave][lane];
      double a[kLpc], ap[kLpc], E = R[0];
#pragma unroll
      for (int i = 0; i < kLpc; ++i) a[i] = 1.0;
#pragma unroll
      for (int i = 0; i < kLpc; ++i) {
#pragma unroll
        for (int j = 0; j < kLpc; ++j) ap[j] = a[j];
        double st = 0.0;
#pragma unroll
        for (int j = 0; j < kLpc; ++j)
          if (j < i) st = fma(ap[j], R[i - j], st);
        const double rc = (R[i + 1] - st) / E;
        a[i] = rc;
#pragma unroll
        for (int j = 0; j < kLpc; ++j)
          if (j < i) a[j] = ap[j] - ap[i - 1 - j] * rc;
        E = (1.0 - rc * rc) * E;
      }
      s_A[wave][lane][0] = 1.0;
#pragma unroll
      for (int j = 0; j < kLpc; ++j) s_A[wave][lane][j + 1] = -a[j];
    }
    F::stage_fence();
    if constexpr (EXT) {
      // cepstrum of 1 / A(z): c_1 = -a_1, c_k = -a_k - (1 / k) sum_{i < k} i c_i a_{k - i}; each lane overwrites its own R row
      if (lane < 2) {
        const double *A = s_A[wave][lane];
        double c[kLpc + 1];
#pragma unroll
        for (int k = 1; k <= kLpc; ++k) {
          double acc = 0.0;
#pragma unroll
          for (int i = 1; i < k; ++i) acc += (double)i * c[i] * A[k - i];
          c[k] = -A[k] - acc / (double)k;
        }
#pragma unroll
        for (int k = 1; k <= kLpc; ++k) s_R[wave][lane][k] = c[k];
      }
      F::stage_fence();
      if (lane == 0) {
        double d2 = 0.0;
#pragma unroll
        for (int k = 1; k <= kLpc; ++k) {
          const double d = s_R[wave][0][k] - s_R[wave][1][k];
          d2 += d * d;
        }
        p.cep[fo] = limit_keep_nan(4.342944819032518 * sqrt(2.0 * d2), 0.0, 10.0);   // 10 / ln 10
      }
    } else if (lane == 0) {                              // A' T(R_clean) A for A = processed, clean
      const double *R = s_R[wave][0];
      double qf[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const double *A = s_A[wave][s ^ 1];
        double qh = 0.0, ql = 0.0;
        for (int i = 0; i <= kLpc; ++i) {
          double th = 0.0, tl = 0.0;
          for (int j = 0; j <= kLpc; ++j) dd_add_prod(th, tl, A[j], R[i > j ? i - j : j - i]);
          dd_add_prod(qh, ql, A[i], th);
          ql = fma(A[i], tl, ql);
        }
        qf[s] = qh + ql;
      }
      p.llr[fo] = log(qf[0] / qf[1]);
      const double snr = 10.0 * log10(sig / (noi + kEpsF64) + kEpsF64);
      p.seg_snr[fo] = fmin(fmax(snr, -10.0), 35.0);
    }
    F::stage_fence();
    // ---- WSS: the frame / 32768 * window, zero-padded to 1024, as 512 packed complex points
#pragma unroll 2
    for (int i = 0; i < F::PER; ++i) {
      const int m = lane + 64 * i, n = 2 * m;
      double4 z = make_double4(0.0, 0.0, 0.0, 0.0);
      if (n < kWin)
        z = make_double4((double)s_c[b0 + n] / 32768.0 * s_win[n], (double)s_c[b0 + n + 1] / 32768.0 * s_win[n + 1],
                         (double)s_p[b0 + n] / 32768.0 * s_win[n], (double)s_p[b0 + n + 1] / 32768.0 * s_win[n + 1]);
      buf[F::pad(m)] = z;
    }
    F::stage_fence();
    F::forward(buf, s_tw, lane);
    for (int j = lane; j <= 256; j += 64) {             // bins in mirror pairs (j, 512 - j); bin 512 is not used
      const int m = j == 0 ? 0 : 512 - j;
      const double4 vj = buf[F::pad(F::pos(j))], vm = buf[F::pad(F::pos(m))];
      const double2 xj = make_double2(vj.x, vj.y), yj = make_double2(vj.z, vj.w), xm = make_double2(vm.x, vm.y), ym = make_double2(vm.z, vm.w);
      if constexpr (EXT) {
        if (j == 0) {
          s_pw[wave][0] = make_double2(fabs(xj.x + xj.y), fabs(yj.x + yj.y));
        } else {
          const double2 X = packed_bin(xj, xm, s_tw[j]), Y = packed_bin(yj, ym, s_tw[j]);
          s_pw[wave][j] = make_double2(sqrt(X.x * X.x + X.y * X.y), sqrt(Y.x * Y.x + Y.y * Y.y));
          if (m != j) {
            const double2 X2 = packed_bin(xm, xj, s_tw[m]), Y2 = packed_bin(ym, yj, s_tw[m]);
            s_pw[wave][m] = make_double2(sqrt(X2.x * X2.x + X2.y * X2.y), sqrt(Y2.x * Y2.x + Y2.y * Y2.y));
          }
        }
      } else if (j == 0) {
        const double cx = xj.x + xj.y, cy = yj.x + yj.y;
        s_pw[wave][0] = make_float2((float)(cx * cx), (float)(cy * cy));
      } else {
        const double2 X = packed_bin(xj, xm, s_tw[j]), Y = packed_bin(yj, ym, s_tw[j]);
        s_pw[wave][j] = make_float2((float)(X.x * X.x + X.y * X.y), (float)(Y.x * Y.x + Y.y * Y.y));
        if (m != j) {
          const double2 X2 = packed_bin(xm, xj, s_tw[m]), Y2 = packed_bin(ym, yj, s_tw[m]);
          s_pw[wave][m] = make_float2((float)(X2.x * X2.x + X2.y * X2.y), (float)(Y2.x * Y2.x + Y2.y * Y2.y));
        }
      }
    }
    F::stage_fence();
    if constexpr (EXT) {
      // fwseg: magnitudes normalised to unit sum over bins 0..511, critical-band sums of them, then the band SNRs
      // weighted by ce^0.2 (lane b: clean band b, lane 32 + b: processed)
      double sx = 0.0, sy = 0.0;
      for (int k = lane; k < 512; k += 64) {
        sx += s_pw[wave][k].x;
        sy += s_pw[wave][k].y;
      }
      sx = wave_sum_f64(sx) + kEpsF64;
      sy = wave_sum_f64(sy) + kEpsF64;
      const int b = lane & 31, s = lane >> 5;
      if (b < kBands) {
        const int lo = p.band_tab[3 * b], cnt = p.band_tab[3 * b + 1], wo = p.band_tab[3 * b + 2];
        double e = 0.0;
        for (int k = 0; k < cnt; ++k) {
          const double2 mg = s_pw[wave][lo + k];
          e = fma(p.band_w[wo + k], s ? mg.y / sy : mg.x / sx, e);
        }
        s_E[wave][s][b] = e;
      }
      F::stage_fence();
      double num = 0.0, den = 0.0;
      if (lane < kBands) {
        const double ce = s_E[wave][0][lane], pe = s_E[wave][1][lane];
        if (ce > 0.0) {
          const double W = pow(ce, 0.2), d = ce - pe;
          const double err = fmax(d * d, kEpsF64);
          num = W * (10.0 * log10(ce * ce / err));
          den = W;
        }
      }
      num = wave_sum_f64(num);
      den = wave_sum_f64(den);
      if (lane == 0) p.fwseg[fo] = den > 0.0 ? limit_keep_nan(num / den, -10.0, 35.0) : (double)NAN;
      F::stage_fence();
      continue;
    }
    {                                                    // critical-band energies: lane b clean, lane 32 + b processed
      const int b = lane & 31, s = lane >> 5;
      if (b < kBands) {
        const int lo = p.band_tab[3 * b], cnt = p.band_tab[3 * b + 1], wo = p.band_tab[3 * b + 2];
        double e = 0.0;
        for (int k = 0; k < cnt; ++k) {
          const auto pw = s_pw[wave][lo + k];
          e = fma(p.band_w[wo + k], (double)(s ? pw.y : pw.x), e);
        }
        s_E[wave][s][b] = 10.0 * log10(fmax(e, 1e-10));
      }
    }
    F::stage_fence();
    double num = 0.0, den = 0.0;
    if (lane < kBands - 1) {
      const int i = lane;
      double wsig[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const double *E = s_E[wave][s];
        double emax = E[0];
        for (int k = 1; k < kBands; ++k) emax = fmax(emax, E[k]);
        double peak;
        if (E[i + 1] - E[i] > 0.0) {                     // search right while the slope stays positive
          int n = i;
          while (n < kBands - 1 && E[n + 1] - E[n] > 0.0) ++n;
          peak = E[n - 1];                               // (python_eval.py takes the band below the peak here)
        } else {                                         // search left while the slope stays non-positive
          int n = i;
          while (n >= 0 && E[n + 1] - E[n] <= 0.0) --n;
          peak = E[n + 1];
        }
        wsig[s] = (20.0 / (20.0 + emax - E[i])) * (1.0 / (1.0 + peak - E[i]));
      }
      const double W = (wsig[0] + wsig[1]) / 2.0;
      const double d = (s_E[wave][0][i + 1] - s_E[wave][0][i]) - (s_E[wave][1][i + 1] - s_E[wave][1][i]);
      num = W * (d * d);
      den = W;
    }
    num = wave_sum_f64(num);
    den = wave_sum_f64(den);
    if (lane == 0) p.wss[fo] = num / den;
    F::stage_fence();                                    // (the next frame overwrites what other lanes just read)
  }
}

// NaN after every number, ties by index: the position of (v, i) in a stable sort, counted
__device__ __forceinline__ bool sorts_before(double vj, int64_t j, double v, int64_t i) {
  if (isnan(v)) return isnan(vj) && j < i;
  return !isnan(vj) && (vj < v || (vj == v && j < i));
}

// grid (ceil(max frames / 256), clips): rank of every frame value within its clip, tiled through LDS
__global__ __launch_bounds__(256) void metrics_rank_kernel(const double *__restrict__ vals, const ClipRow *__restrict__ clips,
                                                          int32_t *__restrict__ ranks) {
  __shared__ double s_v[256];
  const ClipRow c = clips[blockIdx.y];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if ((int64_t)blockIdx.x * 256 >= c.n_frames) return;
  const double v = i < c.n_frames ? vals[c.frame_off + i] : 0.0;
  int64_t r = 0;
  for (int64_t t0 = 0; t0 < c.n_frames; t0 += 256) {
    __syncthreads();
    if (t0 + threadIdx.x < c.n_frames) s_v[threadIdx.x] = vals[c.frame_off + t0 + threadIdx.x];
    __syncthreads();
    const int nt = (int)min((int64_t)256, c.n_frames - t0);
    for (int j = 0; j < nt; ++j) r += sorts_before(s_v[j], t0 + j, v, i);
  }
  if (i < c.n_frames) ranks[c.frame_off + i] = (int32_t)r;
}

// grid (clips): mean of the frame values whose rank is below keep (all of them when ranks is null), NaNs dropped on
// request; 0 / 0 = NaN for an empty selection, as np.mean of an empty array
__global__ __launch_bounds__(256) void metrics_clip_mean_kernel(const double *__restrict__ vals, const int32_t *__restrict__ ranks,
                                                               const ClipRow *__restrict__ clips, int drop_nan,
                                                               double *__restrict__ out) {
  __shared__ double s_s[256];
  __shared__ double s_n[256];
  const ClipRow c = clips[blockIdx.x];
  double s = 0.0, n = 0.0;
  for (int64_t i = threadIdx.x; i < c.n_frames; i += 256) {
    const double v = vals[c.frame_off + i];
    if (ranks && ranks[c.frame_off + i] >= c.keep) continue;
    if (drop_nan && isnan(v)) continue;
    s += v;
    n += 1.0;
  }
  s_s[threadIdx.x] = s;
  s_n[threadIdx.x] = n;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (threadIdx.x < o) {
      s_s[threadIdx.x] += s_s[threadIdx.x + o];
      s_n[threadIdx.x] += s_n[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = s_s[0] / s_n[0];
}

// ================================================================ exact integer sums (overall SNR, SI-SDR)
constexpr int kSumChunk = 8192;                          // samples per workgroup: 256 lanes x 4 groups of 8

__device__ __forceinline__ void sums_add(int64_t &xx, int64_t &yy, int64_t &xy, int x, int y) {
  // one product at a time into int64: (-32768)^2 is 2^30, and two of them already overflow an int32 pair sum
  xx += (int64_t)(x * x);
  yy += (int64_t)(y * y);
  xy += (int64_t)(x * y);
}

// grid (ceil(max chunks), clips): chunk c of a clip covers the 8-sample groups [a + c kSumChunk, a + (c + 1) kSumChunk) from
// the 16-byte aligned base a below the clip's start.  A group wholly inside the clip is one 16-byte load per signal;
// the lead and tail groups read sample by sample, inside the clip only.  part[(frame_off + c) * 3 + {0, 1, 2}].
__global__ __launch_bounds__(256) void metrics_sums_kernel(const int16_t *__restrict__ clean, const int16_t *__restrict__ proc,
                                                          const ClipRow *__restrict__ clips, int64_t *__restrict__ part) {
  __shared__ int64_t s_s[3][256];
  const ClipRow c = clips[blockIdx.y];
  if ((int64_t)blockIdx.x >= c.n_frames) return;         // n_frames: this clip's chunk count
  const int64_t a = c.off & ~(int64_t)7, end = c.off + c.len;
  int64_t xx = 0, yy = 0, xy = 0;
#pragma unroll
  for (int g = 0; g < kSumChunk / (8 * 256); ++g) {
    const int64_t s = a + (int64_t)blockIdx.x * kSumChunk + 8 * (int64_t)(g * 256 + threadIdx.x);
    if (s >= end) break;
    if (s >= c.off && s + 8 <= end) {
      const int4 u = *reinterpret_cast<const int4 *>(clean + s), v = *reinterpret_cast<const int4 *>(proc + s);
      const int uw[4] = {u.x, u.y, u.z, u.w}, vw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        sums_add(xx, yy, xy, (int)(int16_t)(uw[i] & 0xffff), (int)(int16_t)(vw[i] & 0xffff));
        sums_add(xx, yy, xy, uw[i] >> 16, vw[i] >> 16);
      }
    } else {
      for (int i = 0; i < 8; ++i)
        if (s + i >= c.off && s + i < end) sums_add(xx, yy, xy, (int)clean[s + i], (int)proc[s + i]);
    }
  }
  s_s[0][threadIdx.x] = xx;
  s_s[1][threadIdx.x] = yy;
  s_s[2][threadIdx.x] = xy;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (threadIdx.x < o) {
#pragma unroll
      for (int k = 0; k < 3; ++k) s_s[k][threadIdx.x] += s_s[k][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) part[(c.frame_off + blockIdx.x) * 3 + threadIdx.x] = s_s[threadIdx.x][0];
}

// grid (clips): the clip's chunk sums added up, out[clip][3]
__global__ __launch_bounds__(256) void metrics_sums_reduce_kernel(const ClipRow *__restrict__ clips, const int64_t *__restrict__ part,
                                                                 int64_t *__restrict__ out) {
  __shared__ int64_t s_s[3][256];
  const ClipRow c = clips[blockIdx.x];
  int64_t v[3] = {0, 0, 0};
  for (int64_t q = threadIdx.x; q < c.n_frames; q += 256) {
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] += part[(c.frame_off + q) * 3 + k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) s_s[k][threadIdx.x] = v[k];
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (threadIdx.x < o) {
#pragma unroll
      for (int k = 0; k < 3; ++k) s_s[k][threadIdx.x] += s_s[k][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) out[blockIdx.x * 3 + threadIdx.x] = s_s[threadIdx.x][0];
}

// ================================================================ STOI (pystoi.stoi; extended: Jensen & Taal 2016)
constexpr int kStoiFrame = 256, kStoiHop = 128, kStoiBands = 15, kStoiSeg = 30;
constexpr double kStoiDyn = 40.0, kStoiClip = 5.623413251903491;   // 10^(15 / 20): beta = -15 dB

// row: off, len | aux: rs_off, rs_len, nf (silence frames), ef_off, comp_off, tob_off
struct StoiRow {
  int64_t off, len, rs_off, rs_len, nf, ef_off, comp_off, tob_off;
};

struct StoiParams {
  const int16_t *clean, *proc;
  const StoiRow *clips;
  const double *taps;         // polyphase filter, already scaled by up (16 k only)
  int n_taps, up, down, pre_pad, pre_remove;
  const double *win;          // hanning(258)[1:-1]
  const double *tw;           // e^{-2 pi i m / 512}, m = 0..256
  const int32_t *bands;       // [15][2] first bin, end bin
  double *rs_x, *rs_y, *energy, *comp_x, *comp_y, *tob_x, *tob_y;
  int64_t *kept_src, *kept;
  double *out;
  double *out_e;              // eSTOI (stoi_ecorr_kernel)
};

// grid (ceil(max resampled length / 256), clips): y[m] = sum_n x[n] h[(m + pre_remove) down - n up - pre_pad]
// (scipy's upfirdn with the zero-padded filter of resample_poly); up = 0 copies the clip (10 kHz input)
__global__ __launch_bounds__(256) void stoi_resample_kernel(const StoiParams p) {
  const StoiRow c = p.clips[blockIdx.y];
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (m >= c.rs_len) return;
  const int16_t *x = p.clean + c.off, *y = p.proc + c.off;
  if (p.up == 0) {
    p.rs_x[c.rs_off + m] = (double)x[m];
    p.rs_y[c.rs_off + m] = (double)y[m];
    return;
  }
  const int64_t t = (m + p.pre_remove) * p.down - p.pre_pad;
  int64_t n_lo = t - p.n_taps + 1 <= 0 ? 0 : (t - p.n_taps + 1 + p.up - 1) / p.up;
  int64_t n_hi = t < 0 ? -1 : min(t / p.up, c.len - 1);
  double sx = 0.0, sy = 0.0;
  for (int64_t n = n_lo; n <= n_hi; ++n) {
    const double h = p.taps[t - n * p.up];
    sx = fma(h, (double)x[n], sx);
    sy = fma(h, (double)y[n], sy);
  }
  p.rs_x[c.rs_off + m] = sx;
  p.rs_y[c.rs_off + m] = sy;
}

// grid (ceil(max nf / 4), clips), one wave per frame: 20 log10(|w x_frame| + eps) of the clean signal
__global__ __launch_bounds__(256) void stoi_energy_kernel(const StoiParams p) {
  const StoiRow c = p.clips[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= c.nf) return;
  const double *x = p.rs_x + c.rs_off + f * kStoiHop;
  double s = 0.0;
  for (int n = lane; n < kStoiFrame; n += 64) {
    const double v = p.win[n] * x[n];
    s = fma(v, v, s);
  }
  s = wave_sum_f64(s);
  if (lane == 0) p.energy[c.ef_off + f] = 20.0 * log10(sqrt(s) + kEpsF64);
}

// grid (clips): frames within 40 dB of the clip's loudest are kept; their indices compacted in order
__global__ __launch_bounds__(256) void stoi_mask_kernel(const StoiParams p) {
  __shared__ double s_m[256];
  __shared__ int64_t s_c[256];
  const StoiRow c = p.clips[blockIdx.x];
  const double *e = p.energy + c.ef_off;
  double m = -INFINITY;
  for (int64_t f = threadIdx.x; f < c.nf; f += 256) m = fmax(m, e[f]);
  s_m[threadIdx.x] = m;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (threadIdx.x < o) s_m[threadIdx.x] = fmax(s_m[threadIdx.x], s_m[threadIdx.x + o]);
    __syncthreads();
  }
  const double emax = s_m[0];
  int64_t base = 0;
  for (int64_t f0 = 0; f0 < c.nf; f0 += 256) {
    const int64_t f = f0 + threadIdx.x;
    const int keep = f < c.nf && (emax - kStoiDyn - e[f]) < 0.0;
    __syncthreads();
    s_c[threadIdx.x] = keep;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {                  // inclusive scan
      const int64_t v = threadIdx.x >= o ? s_c[threadIdx.x - o] : 0;
      __syncthreads();
      s_c[threadIdx.x] += v;
      __syncthreads();
    }
    if (keep) p.kept_src[c.ef_off + base + s_c[threadIdx.x] - 1] = f;
    base += s_c[255];
  }
  if (threadIdx.x == 0) p.kept[blockIdx.x] = base;
}

// grid (ceil(max comp length / 256), clips): overlap-add of the kept windowed frames, (kept - 1) * 128 + 256 samples
__global__ __launch_bounds__(256) void stoi_ola_kernel(const StoiParams p) {
  const StoiRow c = p.clips[blockIdx.y];
  const int64_t nk = p.kept[blockIdx.y];
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (nk == 0 || t >= (nk - 1) * kStoiHop + kStoiFrame) return;
  const int64_t j = t / kStoiHop;
  const int o = (int)(t - j * kStoiHop);
  const int64_t *src = p.kept_src + c.ef_off;
  const double *x = p.rs_x + c.rs_off, *y = p.rs_y + c.rs_off;
  double vx = 0.0, vy = 0.0;
  if (j < nk) {
    const int64_t s = src[j] * kStoiHop + o;
    vx = p.win[o] * x[s];
    vy = p.win[o] * y[s];
  }
  if (j >= 1) {
    const int64_t s = src[j - 1] * kStoiHop + o + kStoiHop;
    vx += p.win[o + kStoiHop] * x[s];
    vy += p.win[o + kStoiHop] * y[s];
  }
  p.comp_x[c.comp_off + t] = vx;
  p.comp_y[c.comp_off + t] = vy;
}

// grid (ceil(max nf / 4), clips), one wave per STFT frame (kept - 1 of them): 512-point FFT of the windowed 256 samples in
// LDS, then the one-third-octave band magnitudes sqrt(sum |X_k|^2)
__global__ __launch_bounds__(64 * kMetricWaves) void stoi_tob_kernel(const StoiParams p) {
  typedef FusedFft<256, double> F;
  __shared__ __attribute__((aligned(16))) double4 s_buf[kMetricWaves][F::SLOTS];
  __shared__ double2 s_tw[257];
  __shared__ float2 s_pw[kMetricWaves][257];
  const StoiRow c = p.clips[blockIdx.y];
  const int64_t nk = p.kept[blockIdx.y], ns = nk > 0 ? nk - 1 : 0;
  if ((int64_t)blockIdx.x * kMetricWaves >= ns) return;
  for (int i = threadIdx.x; i <= 256; i += blockDim.x) s_tw[i] = reinterpret_cast<const double2 *>(p.tw)[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = uniform(threadIdx.x >> 6);
  const int64_t f = (int64_t)blockIdx.x * kMetricWaves + wave;
  if (f >= ns) return;
  double4 *buf = s_buf[wave];
  const double *x = p.comp_x + c.comp_off + f * kStoiHop, *y = p.comp_y + c.comp_off + f * kStoiHop;
#pragma unroll
  for (int i = 0; i < F::PER; ++i) {
    const int m = lane + 64 * i, n = 2 * m;
    double4 z = make_double4(0.0, 0.0, 0.0, 0.0);
    if (n < kStoiFrame) z = make_double4(p.win[n] * x[n], p.win[n + 1] * x[n + 1], p.win[n] * y[n], p.win[n + 1] * y[n + 1]);
    buf[F::pad(m)] = z;
  }
  F::stage_fence();
  F::forward(buf, s_tw, lane);
  for (int j = lane; j <= 128; j += 64) {
    const int m = j == 0 ? 0 : 256 - j;
    const double4 vj = buf[F::pad(F::pos(j))], vm = buf[F::pad(F::pos(m))];
    const double2 xj = make_double2(vj.x, vj.y), yj = make_double2(vj.z, vj.w), xm = make_double2(vm.x, vm.y), ym = make_double2(vm.z, vm.w);
    if (j == 0) {
      const double a = xj.x + xj.y, b = yj.x + yj.y, a2 = xj.x - xj.y, b2 = yj.x - yj.y;
      s_pw[wave][0] = make_float2((float)(a * a), (float)(b * b));
      s_pw[wave][256] = make_float2((float)(a2 * a2), (float)(b2 * b2));
    } else {
      const double2 X = packed_bin(xj, xm, s_tw[j]), Y = packed_bin(yj, ym, s_tw[j]);
      s_pw[wave][j] = make_float2((float)(X.x * X.x + X.y * X.y), (float)(Y.x * Y.x + Y.y * Y.y));
      if (m != j) {
        const double2 X2 = packed_bin(xm, xj, s_tw[m]), Y2 = packed_bin(ym, yj, s_tw[m]);
        s_pw[wave][m] = make_float2((float)(X2.x * X2.x + X2.y * X2.y), (float)(Y2.x * Y2.x + Y2.y * Y2.y));
      }
    }
  }
  F::stage_fence();
  const int b = lane & 15, s = lane >> 4;               // lanes 0-14 clean, 16-30 processed
  if (b < kStoiBands && s < 2) {
    double e = 0.0;
    for (int k = p.bands[2 * b]; k < p.bands[2 * b + 1]; ++k) e += (double)(s ? s_pw[wave][k].y : s_pw[wave][k].x);
    (s ? p.tob_y : p.tob_x)[(c.tob_off + f) * kStoiBands + b] = sqrt(e);
  }
}

// grid (clips): the intermediate intelligibility of every (30-frame segment, band), averaged
__global__ __launch_bounds__(256) void stoi_corr_kernel(const StoiParams p) {
  __shared__ double s_s[256];
  const StoiRow c = p.clips[blockIdx.x];
  const int64_t nk = p.kept[blockIdx.x], ns = nk > 0 ? nk - 1 : 0;
  if (ns < kStoiSeg) {                                   // pystoi: not enough frames, returns 1e-5
    if (threadIdx.x == 0) p.out[blockIdx.x] = 1e-5;
    return;
  }
  const int64_t J = ns - kStoiSeg + 1, pairs = J * kStoiBands;
  double acc = 0.0;
  for (int64_t q = threadIdx.x; q < pairs; q += 256) {
    const int64_t m = q / kStoiBands;
    const int b = (int)(q - m * kStoiBands);
    const double *X = p.tob_x + (c.tob_off + m) * kStoiBands + b, *Y = p.tob_y + (c.tob_off + m) * kStoiBands + b;
    double xx = 0.0, yy = 0.0;
    for (int t = 0; t < kStoiSeg; ++t) {
      xx = fma(X[t * kStoiBands], X[t * kStoiBands], xx);
      yy = fma(Y[t * kStoiBands], Y[t * kStoiBands], yy);
    }
    const double nc = sqrt(xx) / (sqrt(yy) + kEpsF64);
    double ym = 0.0, xm = 0.0;
    for (int t = 0; t < kStoiSeg; ++t) {
      ym += fmin(Y[t * kStoiBands] * nc, X[t * kStoiBands] * (1.0 + kStoiClip));
      xm += X[t * kStoiBands];
    }
    ym /= kStoiSeg;
    xm /= kStoiSeg;
    double yn = 0.0, xn = 0.0, xy = 0.0;
    for (int t = 0; t < kStoiSeg; ++t) {
      const double yp = fmin(Y[t * kStoiBands] * nc, X[t * kStoiBands] * (1.0 + kStoiClip)) - ym, xp = X[t * kStoiBands] - xm;
      yn = fma(yp, yp, yn);
      xn = fma(xp, xp, xn);
      xy = fma(yp, xp, xy);
    }
    acc += xy / ((sqrt(yn) + kEpsF64) * (sqrt(xn) + kEpsF64));
  }
  s_s[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (threadIdx.x < o) s_s[threadIdx.x] += s_s[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) p.out[blockIdx.x] = s_s[0] / (double)pairs;
}

// grid (clips), one wave per 30-frame segment at a time (wave w takes segments w, w + 4, ...): eSTOI (Jensen & Taal 2016)
// on the band magnitudes of stoi_tob_kernel.  Both 15 x 30 matrices of a segment: rows (bands) to zero mean and unit
// norm over the frames, then columns (frames) to zero mean and unit norm over the bands, every norm + eps (pystoi adds
// eps-sized noise instead); the segment's value is the sum of the products / 30.  Each wave adds its segments in order,
// the four wave sums are added in order: fixed summation order per clip.
__global__ __launch_bounds__(64 * kMetricWaves) void stoi_ecorr_kernel(const StoiParams p) {
  __shared__ double s_m[kMetricWaves][2][kStoiSeg * kStoiBands];
  __shared__ double s_acc[kMetricWaves];
  const StoiRow c = p.clips[blockIdx.x];
  const int64_t nk = p.kept[blockIdx.x], ns = nk > 0 ? nk - 1 : 0;
  if (ns < kStoiSeg) {                                   // as STOI: not enough frames
    if (threadIdx.x == 0) p.out_e[blockIdx.x] = 1e-5;
    return;
  }
  typedef FusedFft<256, double> F;                       // (for the wave-scope fence only)
  const int lane = threadIdx.x & 63, wave = uniform(threadIdx.x >> 6);
  const int64_t J = ns - kStoiSeg + 1;
  double *mx = s_m[wave][0], *my = s_m[wave][1];
  double acc = 0.0;
  for (int64_t m = wave; m < J; m += kMetricWaves) {
    const double *X = p.tob_x + (c.tob_off + m) * kStoiBands, *Y = p.tob_y + (c.tob_off + m) * kStoiBands;
    for (int i = lane; i < kStoiSeg * kStoiBands; i += 64) {   // element (frame t, band b) at t * 15 + b
      mx[i] = X[i];
      my[i] = Y[i];
    }
    F::stage_fence();
    {                                                    // rows: lanes 0-14 clean, 16-30 processed
      const int b = lane & 15, s = lane >> 4;
      if (b < kStoiBands && s < 2) {
        double *M = s ? my : mx;
        double mean = 0.0;
        for (int t = 0; t < kStoiSeg; ++t) mean += M[t * kStoiBands + b];
        mean /= kStoiSeg;
        double nn = 0.0;
        for (int t = 0; t < kStoiSeg; ++t) {
          const double v = M[t * kStoiBands + b] - mean;
          nn = fma(v, v, nn);
        }
        const double d = sqrt(nn) + kEpsF64;
        for (int t = 0; t < kStoiSeg; ++t) M[t * kStoiBands + b] = (M[t * kStoiBands + b] - mean) / d;
      }
    }
    F::stage_fence();
    {                                                    // columns: lanes 0-29 clean, 32-61 processed
      const int t = lane & 31, s = lane >> 5;
      if (t < kStoiSeg) {
        double *M = (s ? my : mx) + t * kStoiBands;
        double mean = 0.0;
        for (int b = 0; b < kStoiBands; ++b) mean += M[b];
        mean /= kStoiBands;
        double nn = 0.0;
        for (int b = 0; b < kStoiBands; ++b) {
          const double v = M[b] - mean;
          nn = fma(v, v, nn);
        }
        const double d = sqrt(nn) + kEpsF64;
        for (int b = 0; b < kStoiBands; ++b) M[b] = (M[b] - mean) / d;
      }
    }
    F::stage_fence();
    double dot = 0.0;
    if (lane < kStoiSeg)
      for (int b = 0; b < kStoiBands; ++b) dot = fma(mx[lane * kStoiBands + b], my[lane * kStoiBands + b], dot);
    dot = wave_sum_f64(dot);
    acc += dot / kStoiSeg;
    F::stage_fence();                                    // (the next segment overwrites what other lanes just read)
  }
  if (lane == 0) s_acc[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < kMetricWaves; ++w) t += s_acc[w];
    p.out_e[blockIdx.x] = t / (double)J;
  }
}

}  // namespace cum

using namespace cum;

// ---- host side
// The clip table goes to the head of the workspace from host memory that the entry owns: the upload is waited for before
// the entry returns, so the table may go out of scope (one stream synchronise per call).
static int upload_rows(const char *who, void *dst, const void *src, size_t bytes, hipStream_t st) {
  if (hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
    static char msg[128];
    snprintf(msg, sizeof msg, "%s: clip table upload failed", who);
    cum_set_error(msg);
    return CUM_ELAUNCH;
  }
  return CUM_OK;
}

static int check_clips(const char *who, const int16_t *clean, const int16_t *proc, int64_t n_samples, const int64_t *offsets,
                       const int64_t *lengths, int64_t n_clips, int64_t min_len) {
  static char msg[256];
  CUM_REQUIRE(n_clips > 0 && n_clips <= 65535, "metrics: the batch must hold 1 to 65535 clips");
  CUM_REQUIRE(offsets && lengths, "metrics: null offsets or lengths");
  CUM_REQUIRE(n_samples >= 0, "metrics: bad sample count");
  for (int64_t i = 0; i < n_clips; ++i) {
    if (lengths[i] < min_len) {
      snprintf(msg, sizeof msg, "%s: clip %lld has %lld samples, fewer than one window (%lld)", who, (long long)i,
               (long long)lengths[i], (long long)min_len);
      cum_set_error(msg);
      return CUM_EINVAL;
    }
    if (offsets[i] < 0 || offsets[i] > n_samples - lengths[i]) {
      snprintf(msg, sizeof msg, "%s: clip %lld lies outside the sample buffer", who, (long long)i);
      cum_set_error(msg);
      return CUM_EINVAL;
    }
  }
  CUM_REQUIRE(clean && proc, "metrics: null signal");
  CUM_REQUIRE((((uintptr_t)clean) | ((uintptr_t)proc)) % 16 == 0, "metrics: signals must be 16-byte aligned");
  return CUM_OK;
}

static int64_t round_half_even(double x) { return (int64_t)nearbyint(x); }   // Python's round() (default FE_TONEAREST)

extern "C" int64_t cum_metrics_frame_count(int64_t len) { return len < kWin ? -1 : (len - kWin) / kHop; }

extern "C" int64_t cum_metrics_reduce_keep(int64_t n_frames) { return round_half_even((double)n_frames * 0.95); }

extern "C" int64_t cum_metrics_workspace_bytes(int64_t n_clips, int64_t n_frames_total) {
  return n_clips * (int64_t)sizeof(ClipRow) + 4 * ((n_frames_total + 1) / 2 * 2);
}

static void frame_rows(const int64_t *offsets, const int64_t *lengths, int64_t n_clips, std::vector<ClipRow> &rows,
                       int64_t &total, int64_t &max_nf) {
  rows.resize(n_clips);
  total = 0;
  max_nf = 0;
  for (int64_t i = 0; i < n_clips; ++i) {
    const int64_t nf = cum_metrics_frame_count(lengths[i]);
    rows[i] = ClipRow{offsets[i], lengths[i], total, nf, cum_metrics_reduce_keep(nf), 0, 0, 0};
    total += nf;
    max_nf = nf > max_nf ? nf : max_nf;
  }
}

extern "C" int cum_metrics_frames(const int16_t *clean, const int16_t *processed, int64_t n_samples, const int64_t *offsets,
                                  const int64_t *lengths, int64_t n_clips, int32_t rate, const double *window,
                                  const int32_t *band_tab, const double *band_w, const double *tw, void *workspace,
                                  int64_t workspace_bytes, double *seg_snr, double *llr, double *wss, int64_t n_frames_total,
                                  void *stream) {
  CUM_REQUIRE(rate == 16000, "metrics_frames: the frame metrics run at 16 kHz only");
  if (int rc = check_clips("metrics_frames", clean, processed, n_samples, offsets, lengths, n_clips, kWin)) return rc;
  std::vector<ClipRow> rows;
  int64_t total, max_nf;
  frame_rows(offsets, lengths, n_clips, rows, total, max_nf);
  CUM_REQUIRE(total == n_frames_total, "metrics_frames: n_frames_total must be the sum of the clips' frame counts");
  CUM_REQUIRE(workspace && workspace_bytes >= cum_metrics_workspace_bytes(n_clips, total), "metrics_frames: workspace too small");
  CUM_REQUIRE(window && band_tab && band_w && tw, "metrics_frames: null table");
  CUM_REQUIRE(total == 0 || (seg_snr && llr && wss), "metrics_frames: null output");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = upload_rows("metrics_frames", workspace, rows.data(), n_clips * sizeof(ClipRow), st)) return rc;
  if (max_nf == 0) return CUM_OK;
  FrameParams p{clean, processed, n_samples, (const ClipRow *)workspace, window, band_tab, band_w, tw, seg_snr, llr, wss,
                nullptr, nullptr};
  hipLaunchKernelGGL(metrics_frames_kernel<false>, dim3((unsigned)cdiv64(max_nf, kFpb), (unsigned)n_clips),
                     dim3(64 * kMetricWaves), 0, st, p);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}

// cum_metrics_frames_ext <- Hu & Loizou 2008: the LPC cepstrum distance (Kitawaki et al. 1988) and the frequency-weighted
// segmental SNR (Tribolet et al. 1978) on the frames, window, LPC, FFT and critical bands of cum_metrics_frames; the
// definitions are restated in tests/metrics_ext_ref.py
extern "C" int cum_metrics_frames_ext(const int16_t *clean, const int16_t *processed, int64_t n_samples, const int64_t *offsets,
                                      const int64_t *lengths, int64_t n_clips, int32_t rate, const double *window,
                                      const int32_t *band_tab, const double *band_w, const double *tw, void *workspace,
                                      int64_t workspace_bytes, double *cep, double *fwseg, int64_t n_frames_total,
                                      void *stream) {
  CUM_REQUIRE(rate == 16000, "metrics_frames_ext: the frame metrics run at 16 kHz only");
  if (int rc = check_clips("metrics_frames_ext", clean, processed, n_samples, offsets, lengths, n_clips, kWin)) return rc;
  std::vector<ClipRow> rows;
  int64_t total, max_nf;
  frame_rows(offsets, lengths, n_clips, rows, total, max_nf);
  CUM_REQUIRE(total == n_frames_total, "metrics_frames_ext: n_frames_total must be the sum of the clips' frame counts");
  CUM_REQUIRE(workspace && workspace_bytes >= cum_metrics_workspace_bytes(n_clips, total),
              "metrics_frames_ext: workspace too small");
  CUM_REQUIRE(window && band_tab && band_w && tw, "metrics_frames_ext: null table");
  CUM_REQUIRE(total == 0 || (cep && fwseg), "metrics_frames_ext: null output");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = upload_rows("metrics_frames_ext", workspace, rows.data(), n_clips * sizeof(ClipRow), st)) return rc;
  if (max_nf == 0) return CUM_OK;
  FrameParams p{clean, processed, n_samples, (const ClipRow *)workspace, window, band_tab, band_w, tw, nullptr, nullptr,
                nullptr, cep, fwseg};
  hipLaunchKernelGGL(metrics_frames_kernel<true>, dim3((unsigned)cdiv64(max_nf, kFpb), (unsigned)n_clips),
                     dim3(64 * kMetricWaves), 0, st, p);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}

// per-clip mean of the frame values that are not NaN (fwsegSNR); NaN where a clip has none.  Same layout, workspace and
// checks as cum_metrics_clip_reduce.
extern "C" int cum_metrics_clip_nanmean(const double *values, const int64_t *lengths, int64_t n_clips, void *workspace,
                                        int64_t workspace_bytes, double *out, void *stream) {
  CUM_REQUIRE(n_clips > 0 && n_clips <= 65535 && lengths, "metrics_clip_nanmean: bad batch");
  std::vector<int64_t> offs(n_clips, 0);
  for (int64_t i = 0; i < n_clips; ++i) CUM_REQUIRE(lengths[i] >= kWin, "metrics_clip_nanmean: clip shorter than one window");
  std::vector<ClipRow> rows;
  int64_t total, max_nf;
  frame_rows(offs.data(), lengths, n_clips, rows, total, max_nf);
  CUM_REQUIRE(workspace && workspace_bytes >= cum_metrics_workspace_bytes(n_clips, total),
              "metrics_clip_nanmean: workspace too small");
  CUM_REQUIRE(out && (total == 0 || values), "metrics_clip_nanmean: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = upload_rows("metrics_clip_nanmean", workspace, rows.data(), n_clips * sizeof(ClipRow), st)) return rc;
  hipLaunchKernelGGL(metrics_clip_mean_kernel, dim3((unsigned)n_clips), dim3(256), 0, st, values, (const int32_t *)nullptr,
                     (const ClipRow *)workspace, 1, out);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}

// cum_metrics_sums: exact Sxx = sum x^2, Syy = sum y^2, Sxy = sum x y of every clip as int64 (out[i][3]), the integers
// behind the overall SNR and SI-SDR (Le Roux et al. 2019)
extern "C" int64_t cum_metrics_sums_workspace_bytes(const int64_t *lengths, int64_t n_clips) {
  if (!lengths || n_clips <= 0) return -1;
  int64_t chunks = 0;
  for (int64_t i = 0; i < n_clips; ++i) chunks += cdiv64((lengths[i] > 0 ? lengths[i] : 0) + 7, kSumChunk);
  return n_clips * (int64_t)sizeof(ClipRow) + chunks * 3 * 8;
}

extern "C" int cum_metrics_sums(const int16_t *clean, const int16_t *processed, int64_t n_samples, const int64_t *offsets,
                                const int64_t *lengths, int64_t n_clips, void *workspace, int64_t workspace_bytes,
                                int64_t *out, void *stream) {
  if (int rc = check_clips("metrics_sums", clean, processed, n_samples, offsets, lengths, n_clips, 1)) return rc;
  std::vector<ClipRow> rows(n_clips);
  int64_t chunks = 0, max_ch = 0;
  for (int64_t i = 0; i < n_clips; ++i) {
    // int64 holds 2^63 / 2^30 = 2^33 full-scale products
    CUM_REQUIRE(lengths[i] < ((int64_t)1 << 33), "metrics_sums: clip too long for exact int64 sums");
    const int64_t nch = cdiv64((offsets[i] & 7) + lengths[i], kSumChunk);     // chunks start at the aligned base
    rows[i] = ClipRow{offsets[i], lengths[i], chunks, nch, 0, 0, 0, 0};
    chunks += nch;
    max_ch = nch > max_ch ? nch : max_ch;
  }
  CUM_REQUIRE(workspace && workspace_bytes >= cum_metrics_sums_workspace_bytes(lengths, n_clips),
              "metrics_sums: workspace too small");
  CUM_REQUIRE(out, "metrics_sums: null output");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = upload_rows("metrics_sums", workspace, rows.data(), n_clips * sizeof(ClipRow), st)) return rc;
  const ClipRow *tab = (const ClipRow *)workspace;
  int64_t *part = (int64_t *)((char *)workspace + n_clips * sizeof(ClipRow));
  hipLaunchKernelGGL(metrics_sums_kernel, dim3((unsigned)max_ch, (unsigned)n_clips), dim3(256), 0, st, clean, processed, tab,
                     part);
  hipLaunchKernelGGL(metrics_sums_reduce_kernel, dim3((unsigned)n_clips), dim3(256), 0, st, tab, (const int64_t *)part, out);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}

extern "C" int cum_metrics_clip_reduce(const double *values, const int64_t *lengths, int64_t n_clips, int32_t mode,
                                       void *workspace, int64_t workspace_bytes, double *out, void *stream) {
  CUM_REQUIRE(mode >= 0 && mode <= 2, "metrics_clip_reduce: mode is 0 (mean), 1 (trimmed mean) or 2 (trimmed, NaN dropped)");
  CUM_REQUIRE(n_clips > 0 && n_clips <= 65535 && lengths, "metrics_clip_reduce: bad batch");
  std::vector<int64_t> offs(n_clips, 0);
  for (int64_t i = 0; i < n_clips; ++i) CUM_REQUIRE(lengths[i] >= kWin, "metrics_clip_reduce: clip shorter than one window");
  std::vector<ClipRow> rows;
  int64_t total, max_nf;
  frame_rows(offs.data(), lengths, n_clips, rows, total, max_nf);
  CUM_REQUIRE(total < ((int64_t)1 << 31), "metrics_clip_reduce: too many frames");
  CUM_REQUIRE(workspace && workspace_bytes >= cum_metrics_workspace_bytes(n_clips, total), "metrics_clip_reduce: workspace too small");
  CUM_REQUIRE(out && (total == 0 || values), "metrics_clip_reduce: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = upload_rows("metrics_clip_reduce", workspace, rows.data(), n_clips * sizeof(ClipRow), st)) return rc;
  const ClipRow *tab = (const ClipRow *)workspace;
  int32_t *ranks = (int32_t *)((char *)workspace + n_clips * sizeof(ClipRow));
  if (mode != 0 && max_nf > 0)
    hipLaunchKernelGGL(metrics_rank_kernel, dim3((unsigned)cdiv64(max_nf, 256), (unsigned)n_clips), dim3(256), 0, st, values,
                       tab, ranks);
  hipLaunchKernelGGL(metrics_clip_mean_kernel, dim3((unsigned)n_clips), dim3(256), 0, st, values, mode ? ranks : nullptr, tab,
                     mode == 2 ? 1 : 0, out);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}

// STOI layout: rows + kept counts + every per-clip buffer, in 8-byte elements
struct StoiLayout {
  std::vector<StoiRow> rows;
  int64_t rs, ef, comp, tob, max_rs, max_nf, max_comp, bytes;
};

static int64_t stoi_rs_len(int64_t len, int32_t rate) { return rate == 10000 ? len : cdiv64(len * 5, 8); }

static void stoi_layout(const int64_t *offsets, const int64_t *lengths, int64_t n_clips, int32_t rate, StoiLayout &L) {
  L.rows.resize(n_clips);
  L.rs = L.ef = L.comp = L.tob = L.max_rs = L.max_nf = L.max_comp = 0;
  for (int64_t i = 0; i < n_clips; ++i) {
    const int64_t n = stoi_rs_len(lengths[i], rate);
    const int64_t nf = n > kStoiFrame ? cdiv64(n - kStoiFrame, kStoiHop) : 0;   // range(0, n - 256, 128)
    const int64_t cap = nf * kStoiHop + kStoiHop;                             // (kept - 1) * 128 + 256 at most
    L.rows[i] = StoiRow{offsets ? offsets[i] : 0, lengths[i], L.rs, n, nf, L.ef, L.comp, L.ef};
    L.rs += n;
    L.ef += nf;
    L.comp += cap;
    L.max_rs = n > L.max_rs ? n : L.max_rs;
    L.max_nf = nf > L.max_nf ? nf : L.max_nf;
    L.max_comp = cap > L.max_comp ? cap : L.max_comp;
  }
  // rows | kept | rs_x rs_y | energy | kept_src | comp_x comp_y | tob_x tob_y
  L.bytes = 8 * (n_clips * 8 + n_clips + 2 * L.rs + 2 * L.ef + 2 * L.comp + 2 * L.ef * kStoiBands);
}

extern "C" int64_t cum_metrics_stoi_workspace_bytes(const int64_t *lengths, int64_t n_clips, int32_t rate) {
  if (!lengths || n_clips <= 0 || (rate != 16000 && rate != 10000)) return -1;
  StoiLayout L;
  stoi_layout(nullptr, lengths, n_clips, rate, L);
  return L.bytes;
}

// the body of both STOI entries; which: bit 0 STOI -> out, bit 1 eSTOI -> out_e, on one front end
static int stoi_run(const int16_t *clean, const int16_t *processed, int64_t n_samples, const int64_t *offsets,
                    const int64_t *lengths, int64_t n_clips, int32_t rate, const double *taps, int32_t n_taps,
                    const double *window, const double *tw, const int32_t *bands, void *workspace, int64_t workspace_bytes,
                    int which, double *out, double *out_e, void *stream) {
  CUM_REQUIRE(rate == 16000 || rate == 10000, "metrics_stoi: rate must be 16000 or 10000 Hz");
  if (int rc = check_clips("metrics_stoi", clean, processed, n_samples, offsets, lengths, n_clips, 1)) return rc;
  CUM_REQUIRE(rate == 10000 || (taps && n_taps > 0 && n_taps % 2 == 1), "metrics_stoi: bad resampling filter");
  CUM_REQUIRE(window && tw && bands && (!(which & 1) || out) && (!(which & 2) || out_e), "metrics_stoi: null pointer");
  StoiLayout L;
  stoi_layout(offsets, lengths, n_clips, rate, L);
  CUM_REQUIRE(workspace && workspace_bytes >= L.bytes, "metrics_stoi: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = upload_rows("metrics_stoi", workspace, L.rows.data(), n_clips * sizeof(StoiRow), st)) return rc;
  double *w = (double *)workspace;
  StoiParams p{};
  p.clean = clean;
  p.proc = processed;
  p.clips = (const StoiRow *)w;
  w += n_clips * 8;
  p.kept = (int64_t *)w;
  w += n_clips;
  p.rs_x = w; w += L.rs;
  p.rs_y = w; w += L.rs;
  p.energy = w; w += L.ef;
  p.kept_src = (int64_t *)w; w += L.ef;
  p.comp_x = w; w += L.comp;
  p.comp_y = w; w += L.comp;
  p.tob_x = w; w += L.ef * kStoiBands;
  p.tob_y = w;
  p.win = window;
  p.tw = tw;
  p.bands = bands;
  p.out = out;
  p.out_e = out_e;
  if (rate == 16000) {   // scipy.signal.resample_poly(x, 5, 8, window=h): zero pre-padding that centres the output
    const int up = 5, down = 8, half = (n_taps - 1) / 2;
    p.taps = taps;
    p.n_taps = n_taps;
    p.up = up;
    p.down = down;
    p.pre_pad = down - half % down;
    p.pre_remove = (half + p.pre_pad) / down;
  }
  const unsigned nc = (unsigned)n_clips;
  hipLaunchKernelGGL(stoi_resample_kernel, dim3((unsigned)cdiv64(L.max_rs, 256), nc), dim3(256), 0, st, p);
  if (L.max_nf > 0) hipLaunchKernelGGL(stoi_energy_kernel, dim3((unsigned)cdiv64(L.max_nf, 4), nc), dim3(256), 0, st, p);
  hipLaunchKernelGGL(stoi_mask_kernel, dim3(nc), dim3(256), 0, st, p);
  if (L.max_nf > 0) {
    hipLaunchKernelGGL(stoi_ola_kernel, dim3((unsigned)cdiv64(L.max_comp, 256), nc), dim3(256), 0, st, p);
    hipLaunchKernelGGL(stoi_tob_kernel, dim3((unsigned)cdiv64(L.max_nf, kMetricWaves), nc), dim3(64 * kMetricWaves), 0, st, p);
  }
  if (which & 1) hipLaunchKernelGGL(stoi_corr_kernel, dim3(nc), dim3(256), 0, st, p);
  if (which & 2) hipLaunchKernelGGL(stoi_ecorr_kernel, dim3(nc), dim3(64 * kMetricWaves), 0, st, p);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}

extern "C" int cum_metrics_stoi(const int16_t *clean, const int16_t *processed, int64_t n_samples, const int64_t *offsets,
                                const int64_t *lengths, int64_t n_clips, int32_t rate, const double *taps, int32_t n_taps,
                                const double *window, const double *tw, const int32_t *bands, void *workspace,
                                int64_t workspace_bytes, double *out, void *stream) {
  return stoi_run(clean, processed, n_samples, offsets, lengths, n_clips, rate, taps, n_taps, window, tw, bands, workspace,
                  workspace_bytes, 1, out, nullptr, stream);
}

// cum_metrics_stoi_ex <- pystoi.stoi with extended = False (which & 1 -> out), True (which & 2 -> out_e; Jensen & Taal 2016)
// or both; arguments, tables and workspace (cum_metrics_stoi_workspace_bytes) as cum_metrics_stoi
extern "C" int cum_metrics_stoi_ex(const int16_t *clean, const int16_t *processed, int64_t n_samples, const int64_t *offsets,
                                   const int64_t *lengths, int64_t n_clips, int32_t rate, const double *taps, int32_t n_taps,
                                   const double *window, const double *tw, const int32_t *bands, void *workspace,
                                   int64_t workspace_bytes, int32_t which, double *out, double *out_e, void *stream) {
  CUM_REQUIRE(which >= 1 && which <= 3, "metrics_stoi_ex: which is 1 (STOI), 2 (eSTOI) or 3 (both)");
  return stoi_run(clean, processed, n_samples, offsets, lengths, n_clips, rate, taps, n_taps, window, tw, bands, workspace,
                  workspace_bytes, which, out, out_e, stream);
}
