// Multi-resolution STFT loss around rocFFT (reference src/util/stft_loss.py:16-184).
//
// Per resolution the reference runs torch.stft twice and ~25 elementwise / reduction passes over
// (B, frames, bins) tensors, forward and backward.  Here the FFT itself stays with rocFFT (a plain
// batched r2c / c2r over contiguous frames) and everything around it is four HBM-bound kernels:
//   stft_frames_kernel   x -> windowed frames, reflect padding of torch.stft(center=True)     (:29-33)
//   stft_loss_partials / stft_loss_finalize   spectra -> sc = |Y-X|_F / |Y|_F, mag = mean|log Y - log X|
//                                             on sqrt(clamp(re^2+im^2, 1e-7))                 (:38,:59,:80)
//   stft_loss_grad_kernel  d(loss)/d(spectrum of x), pre-scaled for an unnormalised c2r
//   stft_fold_kernel     frame gradients -> signal gradient (window, overlap-add, reflect fold), gather form
// All sums are tree reductions in a fixed order: bit-reproducible, no float atomics.
#include "common.h"
#include "fft_lds.h"

namespace cum {

constexpr int kLossRows = 8;        // spectrum rows (frames) per workgroup in the loss kernels
constexpr float kClamp = 1e-7f;     // stft_loss.py:38

__device__ __forceinline__ int64_t reflect_index(int64_t s, int64_t len) {
  if (s < 0) s = -s;
  if (s >= len) s = 2 * (len - 1) - s;
  return s;
}

// grid (frames, batch); frames[b][f][n] = win[n - off] * x[b][reflect(f*hop + n - n_fft/2)], 0 outside the window
__global__ __launch_bounds__(256) void stft_frames_kernel(const float *__restrict__ x, int64_t len, int64_t x_sb,
                                                          int n_fft, int hop, int win_len,
                                                          const float *__restrict__ window,
                                                          float *__restrict__ frames, int64_t n_frames) {
  const int64_t f = blockIdx.x, b = blockIdx.y;
  const int off = (n_fft - win_len) / 2;
  const float *xb = x + b * x_sb;
  float *dst = frames + (b * n_frames + f) * n_fft;
  const int64_t s0 = f * hop - n_fft / 2;
  for (int n4 = threadIdx.x * 4; n4 < n_fft; n4 += 256 * 4) {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n4 + j;
      const int wi = n - off;
      v[j] = (wi >= 0 && wi < win_len) ? window[wi] * xb[reflect_index(s0 + n, len)] : 0.f;
    }
    *reinterpret_cast<float4 *>(dst + n4) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

struct LossTerms {
  float mx, my;      // clamped magnitudes
  bool live;         // re^2 + im^2 of x above the clamp (gradient flows)
};

// The rocFFT-route kernels spell the fused multiply-adds of their x / y arithmetic out and take no contraction from
// the compiler (bin_power, packed_bin_sym): left to it, a * b - c * d rounds one product in the x copy of an expression
// and the other in the y copy, and two EQUAL signals get magnitudes that differ in the last bit -- the loss of a signal
// against itself must be exactly 0 and its gradient too.  (The fused kernels keep their arithmetic and see equal frames
// when they load them: fused_load_frame.)
__device__ __forceinline__ float bin_power(float2 s) {
#pragma clang fp contract(off)
  return __builtin_fmaf(s.x, s.x, s.y * s.y);
}
__device__ __forceinline__ float2 cmul_sym(float2 a, float2 b) {
#pragma clang fp contract(off)
  return make_float2(__builtin_fmaf(a.x, b.x, -(a.y * b.y)), __builtin_fmaf(a.x, b.y, a.y * b.x));
}
__device__ __forceinline__ float2 packed_bin_sym(float2 za, float2 zb, float2 w) {      // packed_bin of fft_lds.h
#pragma clang fp contract(off)
  const float2 c1 = make_float2(0.5f * (1.f + w.y), -0.5f * w.x), c2 = make_float2(0.5f * (1.f - w.y), 0.5f * w.x);
  const float2 p = cmul_sym(c1, za), q = cmul_sym(c2, conjf2(zb));
  return make_float2(p.x + q.x, p.y + q.y);
}

__device__ __forceinline__ LossTerms loss_terms(float2 sx, float2 sy) {
  const float px = bin_power(sx), py = bin_power(sy);
  LossTerms t;
  t.mx = sqrtf(fmaxf(px, kClamp));
  t.my = sqrtf(fmaxf(py, kClamp));
  t.live = px >= kClamp;
  return t;
}

__device__ __forceinline__ float block_sum_256(float v, float *red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// rows = batch * frames spectrum rows of `bins` complex values; a workgroup owns kLossRows consecutive rows
__global__ __launch_bounds__(256) void stft_loss_partials_kernel(const float2 *__restrict__ sx,
                                                                 const float2 *__restrict__ sy, int64_t rows,
                                                                 int64_t n_frames, int bins, int64_t frame0,
                                                                 float *__restrict__ partials) {
  __shared__ float red[4];
  const int64_t r0 = (int64_t)blockIdx.x * kLossRows;
  const int nrow = (int)min((int64_t)kLossRows, rows - r0);
  float s1 = 0.f, s2 = 0.f, s3 = 0.f;
  for (int r = 0; r < nrow; ++r) {
    if ((r0 + r) % n_frames < frame0) continue;
    const int64_t base = (r0 + r) * bins;
    for (int k = threadIdx.x; k < bins; k += 256) {
      const LossTerms t = loss_terms(sx[base + k], sy[base + k]);
      const float d = t.my - t.mx;
      s1 += d * d;
      s2 += t.my * t.my;
      s3 += fabsf(logf(t.my) - logf(t.mx));
    }
  }
  s1 = block_sum_256(s1, red);
  s2 = block_sum_256(s2, red);
  s3 = block_sum_256(s3, red);
  if (threadIdx.x == 0) {
    partials[3 * (int64_t)blockIdx.x + 0] = s1;
    partials[3 * (int64_t)blockIdx.x + 1] = s2;
    partials[3 * (int64_t)blockIdx.x + 2] = s3;
  }
}

// one workgroup; stats = {sc, mag, |Y-X|_F, |Y|_F}
__global__ __launch_bounds__(1024) void stft_loss_finalize_kernel(const float *__restrict__ partials, int64_t n_parts,
                                                                  double count, float *__restrict__ stats) {
  __shared__ double red[3][16];
  double s[3] = {0.0, 0.0, 0.0};
  for (int64_t i = threadIdx.x; i < n_parts; i += 1024)
    for (int j = 0; j < 3; ++j) s[j] += (double)partials[3 * i + j];
  for (int j = 0; j < 3; ++j) {
    double v = s[j];
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[j][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int j = 0; j < 3; ++j) {
      double v = 0.0;
      for (int w = 0; w < 16; ++w) v += red[j][w];
      s[j] = v;
    }
    const double ndiff = sqrt(s[0]), ny = sqrt(s[1]);
    stats[0] = (float)(ndiff / ny);
    stats[1] = (float)(s[2] / count);
    stats[2] = (float)ndiff;
    stats[3] = (float)ny;
  }
}

// z = d(g_sc * sc + g_mag * mag)/d(spectrum of x), halved on the interior bins so that an unnormalised c2r of z is
// the gradient wrt the real frames (the hermitian extension counts those bins twice).
__global__ __launch_bounds__(256) void stft_loss_grad_kernel(const float2 *__restrict__ sx,
                                                             const float2 *__restrict__ sy, int64_t rows,
                                                             int64_t n_frames, int bins, int64_t frame0,
                                                             const float *__restrict__ stats,
                                                             const float *__restrict__ g_sc,
                                                             const float *__restrict__ g_mag, float inv_count,
                                                             float2 *__restrict__ z) {
  const int64_t r0 = (int64_t)blockIdx.x * kLossRows;
  const int nrow = (int)min((int64_t)kLossRows, rows - r0);
  const float c_sc = stats[2] > 0.f ? g_sc[0] / (stats[2] * stats[3]) : 0.f;   // 0 at |Y| = |X|, as torch's norm backward
  const float c_mag = g_mag[0] * inv_count;
  for (int r = 0; r < nrow; ++r) {
    const bool in_band = (r0 + r) % n_frames >= frame0;
    const int64_t base = (r0 + r) * bins;
    for (int k = threadIdx.x; k < bins; k += 256) {
      float2 out = make_float2(0.f, 0.f);
      if (in_band) {
        const float2 vx = sx[base + k];
        const LossTerms t = loss_terms(vx, sy[base + k]);
        if (t.live) {
          const float inv_mx = 1.f / t.mx;
          const float lg = logf(t.mx) - logf(t.my);
          const float sgn = lg > 0.f ? 1.f : (lg < 0.f ? -1.f : 0.f);
          float dm = c_sc * (t.mx - t.my) + c_mag * sgn * inv_mx;
          dm *= inv_mx * ((k == 0 || k == bins - 1) ? 1.f : 0.5f);
          out = make_float2(dm * vx.x, dm * vx.y);
        }
      }
      z[base + k] = out;
    }
  }
}

__global__ __launch_bounds__(256) void stft_loss_partials_packed_kernel(const float2 *__restrict__ zx,
                                                                        const float2 *__restrict__ zy, int64_t rows,
                                                                        int64_t n_frames, int H, int64_t frame0,
                                                                        const float2 *__restrict__ tw,
                                                                        float *__restrict__ partials) {
  __shared__ float red[4];
  const int64_t r0 = (int64_t)blockIdx.x * kLossRows;
  const int nrow = (int)min((int64_t)kLossRows, rows - r0);
  float s1 = 0.f, s2 = 0.f, s3 = 0.f;
  for (int r = 0; r < nrow; ++r) {
    if ((r0 + r) % n_frames < frame0) continue;
    const int64_t base = (r0 + r) * H;
    for (int k = threadIdx.x; k <= H; k += 256) {
      const int a = k == H ? 0 : k, b = k == 0 ? 0 : H - k;
      const float2 w = tw[k];
      const LossTerms t = loss_terms(packed_bin_sym(zx[base + a], zx[base + b], w), packed_bin_sym(zy[base + a], zy[base + b], w));
      const float d = t.my - t.mx;
      s1 += d * d;
      s2 += t.my * t.my;
      s3 += fabsf(logf(t.my) - logf(t.mx));
    }
  }
  s1 = block_sum_256(s1, red);
  s2 = block_sum_256(s2, red);
  s3 = block_sum_256(s3, red);
  if (threadIdx.x == 0) {
    partials[3 * (int64_t)blockIdx.x + 0] = s1;
    partials[3 * (int64_t)blockIdx.x + 1] = s2;
    partials[3 * (int64_t)blockIdx.x + 2] = s3;
  }
}

// g_k = dL/dRe X[k] + i dL/dIm X[k] of one bin (no hermitian halving: every bin 0..H enters the loss once)
__device__ __forceinline__ float2 bin_grad(float2 vx, float2 vy, float c_sc, float c_mag) {
  const LossTerms t = loss_terms(vx, vy);
  if (!t.live) return make_float2(0.f, 0.f);
  const float inv_mx = 1.f / t.mx;
  const float lg = logf(t.mx) - logf(t.my);
  const float sgn = lg > 0.f ? 1.f : (lg < 0.f ? -1.f : 0.f);
  const float dm = (c_sc * (t.mx - t.my) + c_mag * sgn * inv_mx) * inv_mx;
  return make_float2(dm * vx.x, dm * vx.y);
}

// gz[j] = dL/dRe Z[j] + i dL/dIm Z[j]:  conj(c1_j) g_j + c2_{H-j} conj(g_{H-j})  (j = 1..H-1);
// gz[0] = (1 + i) Re g_0 + (1 - i) Re g_H.  An unnormalised inverse complex FFT of gz is the gradient wrt the
// frame's samples (even samples in the real parts, odd ones in the imaginary parts).
__global__ __launch_bounds__(256) void stft_loss_grad_packed_kernel(const float2 *__restrict__ zx,
                                                                    const float2 *__restrict__ zy, int64_t rows,
                                                                    int64_t n_frames, int H, int64_t frame0,
                                                                    const float *__restrict__ stats,
                                                                    const float *__restrict__ g_sc,
                                                                    const float *__restrict__ g_mag, float inv_count,
                                                                    const float2 *__restrict__ tw,
                                                                    float2 *__restrict__ gz) {
  const int64_t r0 = (int64_t)blockIdx.x * kLossRows;
  const int nrow = (int)min((int64_t)kLossRows, rows - r0);
  const float c_sc = stats[2] > 0.f ? g_sc[0] / (stats[2] * stats[3]) : 0.f;   // 0 at |Y| = |X|, as torch's norm backward
  const float c_mag = g_mag[0] * inv_count;
  for (int r = 0; r < nrow; ++r) {
    const bool in_band = (r0 + r) % n_frames >= frame0;
    const int64_t base = (r0 + r) * H;
    for (int j = threadIdx.x; j <= H / 2; j += 256) {
      const int m = j == 0 ? 0 : H - j;                 // mirror index
      float2 oj = make_float2(0.f, 0.f), om = oj;
      if (in_band) {
        const float2 xj = zx[base + j], xm = zx[base + m], yj = zy[base + j], ym = zy[base + m];
        if (j == 0) {
          // X[0] = Re z + Im z, X[H] = Re z - Im z (both real)
          const float2 g0 = bin_grad(make_float2(xj.x + xj.y, 0.f), make_float2(yj.x + yj.y, 0.f), c_sc, c_mag);
          const float2 gh = bin_grad(make_float2(xj.x - xj.y, 0.f), make_float2(yj.x - yj.y, 0.f), c_sc, c_mag);
          oj = make_float2(g0.x + gh.x, g0.x - gh.x);
        } else {
          const float2 wj = tw[j], wm = tw[H - j];
          const float2 gj = bin_grad(packed_bin_sym(xj, xm, wj), packed_bin_sym(yj, ym, wj), c_sc, c_mag);
          const float2 gm = bin_grad(packed_bin_sym(xm, xj, wm), packed_bin_sym(ym, yj, wm), c_sc, c_mag);
          // conj(c1_k) = ((1 + w.y) + i w.x)/2 ; c2_k = ((1 - w.y) + i w.x)/2
          const float2 c1j = make_float2(0.5f * (1.f + wj.y), 0.5f * wj.x), c2j = make_float2(0.5f * (1.f - wj.y), 0.5f * wj.x);
          const float2 c1m = make_float2(0.5f * (1.f + wm.y), 0.5f * wm.x), c2m = make_float2(0.5f * (1.f - wm.y), 0.5f * wm.x);
          const float2 a = cmul(c1j, gj), b = cmul(c2m, conjf2(gm));
          oj = make_float2(a.x + b.x, a.y + b.y);
          const float2 c = cmul(c1m, gm), d = cmul(c2j, conjf2(gj));
          om = make_float2(c.x + d.x, c.y + d.y);
        }
      }
      gz[base + j] = oj;
      if (m != j) gz[base + m] = om;
    }
  }
}

// One thread per signal sample: sums win[n] * dframes[f][n] over every (f, n) whose padded position lands on it --
// the direct position and, near the ends, its mirror images in the reflect padding.
__global__ __launch_bounds__(256) void stft_fold_kernel(const float *__restrict__ dframes, int64_t len, int n_fft,
                                                        int hop, int win_len, const float *__restrict__ window,
                                                        int64_t n_frames, float *__restrict__ dx, int64_t dx_sb,
                                                        int accumulate) {
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (m >= len) return;
  const int off = (n_fft - win_len) / 2, half = n_fft / 2;
  const float *src = dframes + b * n_frames * n_fft;
  float acc = 0.f;
  int64_t pos[3];
  int npos = 0;
  pos[npos++] = m + half;
  if (m >= 1 && m <= half) pos[npos++] = half - m;                              // left padding mirrors x[1..half]
  if (m <= len - 2 && m >= len - 1 - half) pos[npos++] = half + 2 * (len - 1) - m;   // right padding
  for (int i = 0; i < npos; ++i) {
    const int64_t p = pos[i];
    // frames with off <= p - f*hop < off + win_len
    if (p - off < 0) continue;
    int64_t f_hi = (p - off) / hop;
    if (f_hi > n_frames - 1) f_hi = n_frames - 1;
    int64_t f_lo = p - off - win_len + 1;
    f_lo = f_lo <= 0 ? 0 : (f_lo + hop - 1) / hop;
    for (int64_t f = f_lo; f <= f_hi; ++f) {
      const int n = (int)(p - f * hop);
      acc += window[n - off] * src[f * n_fft + n];
    }
  }
  float *o = dx + b * dx_sb + m;
  *o = accumulate ? *o + acc : acc;
}


// ================================================================ fused form: framing + FFT + loss in ONE kernel
// The pipeline above moves every frame through HBM four times per signal (frames written, transformed in place by
// rocFFT: read + write, read again by the loss kernel): ~1.7 GB forward and ~1.7 GB backward per step at the training
// shape (16 clips x 160 000 samples x three resolutions), 1.0 ms -- for an op whose inputs are two 10 MB waveforms.  Here a
// wave owns a frame end to end: it reads the frame's samples of x and y straight from the waveforms (window in
// registers), transforms both at once in LDS (a float4 per point: x.re, x.im, y.re, y.im -- one instruction stream, one
// set of twiddles for both signals), and consumes the spectrum where it stands.  Forward: loss partial sums, nothing else
// leaves the CU.  Backward: the two transforms are REBUILT (cheaper than keeping 560 MB of spectra), the gradient spectrum
// overwrites them in place, an inverse transform in LDS yields the frame gradient, of which only the window's support is
// written for cum_stft_fold.
//
// Loss terms of one bin on the hardware's sqrt / log2 (1 ulp each; the HBM-bound kernels above use libm's, which would cost
// as much here as the transform itself): d = |Y| - |X|, |Y|^2, |log|Y| - log|X|| -- the logs straight from the clamped
// powers, log m = (ln 2 / 2) log2 p.
__device__ __forceinline__ void fused_terms(float2 sx, float2 sy, float &s1, float &s2, float &s3) {
  const float px = fmaxf(sx.x * sx.x + sx.y * sx.y, kClamp), py = fmaxf(sy.x * sy.x + sy.y * sy.y, kClamp);
  const float d = __builtin_amdgcn_sqrtf(py) - __builtin_amdgcn_sqrtf(px);
  s1 = fmaf(d, d, s1);
  s2 += py;
  s3 += (0.5f * kLn2) * fabsf(__builtin_amdgcn_logf(py) - __builtin_amdgcn_logf(px));
}

// bin_grad on the same instructions; sign(log|X| - log|Y|) = sign(|X|^2 - |Y|^2) on the clamped powers (no logarithm)
__device__ __forceinline__ float2 fused_bin_grad(float2 vx, float2 vy, float c_sc, float c_mag) {
  const float pxr = vx.x * vx.x + vx.y * vx.y;
  if (!(pxr >= kClamp)) return make_float2(0.f, 0.f);
  const float py = fmaxf(vy.x * vy.x + vy.y * vy.y, kClamp);
  const float inv_mx = __builtin_amdgcn_rsqf(pxr);
  const float mx = pxr * inv_mx, my = __builtin_amdgcn_sqrtf(py);
  const float sgn = pxr > py ? 1.f : (pxr < py ? -1.f : 0.f);
  const float dm = (c_sc * (mx - my) + c_mag * sgn * inv_mx) * inv_mx;
  return make_float2(dm * vx.x, dm * vx.y);
}

struct FusedStftParams {
  const float *x, *y, *window, *tw;
  int64_t len, x_sb, y_sb, n_frames, frame0, n_total;     // n_total = batch * n_frames
  int hop, win_len;
  float *partials;                                        // forward: [gridDim.x][3]
  const float *stats, *g_sc, *g_mag;                      // backward
  float inv_count;
  float *dframes;                                         // backward: [batch][n_frames][n_fft]
};

// the frame's packed samples of both signals -> buf (the window is read where it is used: win_len floats that stay in L1).
// Returns (wave-uniform) whether x == y on every sample the frame sees.  Such a frame has |Y| = |X| bin for bin: it adds
// exactly 0 to ||Y| - |X||^2 and to the log-magnitude sum and gets a zero gradient.  The transform cannot be left to show
// that: the compiler contracts a * b - c * d one way in the x half of a point and the other way in the y half, and two
// equal signals come out of it differing in the last bit.
template <int H>
__device__ __forceinline__ bool fused_load_frame(const FusedStftParams &p, int64_t b, int64_t f, int lane, float4 *buf) {
  typedef FusedFft<H> F;
  const int n_fft = 2 * H, off = (n_fft - p.win_len) / 2;
  const float *xb = p.x + b * p.x_sb, *yb = p.y + b * p.y_sb;
  const int64_t s0 = f * p.hop - H;
  // wave-uniform: no reflection and every pair 8-byte aligned (signals and window)
  const bool inner = s0 >= 0 && s0 + n_fft <= p.len && ((off | p.win_len) & 1) == 0 &&
                     ((((uintptr_t)(xb + s0)) | ((uintptr_t)(yb + s0)) | ((uintptr_t)p.window)) & 7) == 0;
  bool same = true;
#pragma unroll 2
  for (int i = 0; i < F::PER; ++i) {
    const int m = lane + 64 * i, n = 2 * m;
    float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n + 1 >= off && n < off + p.win_len) {            // (the window is zero outside its support)
      float x0, x1, y0, y1, w0, w1;
      if (inner) {
        const float2 xv = *reinterpret_cast<const float2 *>(xb + s0 + n), yv = *reinterpret_cast<const float2 *>(yb + s0 + n);
        const float2 wv = *reinterpret_cast<const float2 *>(p.window + (n - off));
        x0 = xv.x; x1 = xv.y; y0 = yv.x; y1 = yv.y; w0 = wv.x; w1 = wv.y;
      } else {
        const int64_t i0 = reflect_index(s0 + n, p.len), i1 = reflect_index(s0 + n + 1, p.len);
        x0 = xb[i0]; x1 = xb[i1]; y0 = yb[i0]; y1 = yb[i1];
        const int wi = n - off;
        w0 = (wi >= 0 && wi < p.win_len) ? p.window[wi] : 0.f;
        w1 = (wi + 1 >= 0 && wi + 1 < p.win_len) ? p.window[wi + 1] : 0.f;
      }
      z = make_float4(w0 * x0, w1 * x1, w0 * y0, w1 * y1);
      same = same && z.x == z.z && z.y == z.w;
    }
    buf[F::pad(m)] = z;
  }
  return __all(same) != 0;
}

template <int H>
__device__ __forceinline__ void fused_load_tables(const FusedStftParams &p, float2 *tw) {
  for (int k = threadIdx.x; k <= H; k += blockDim.x) tw[k] = reinterpret_cast<const float2 *>(p.tw)[k];
  __syncthreads();
}

constexpr int kFusedWaves = 4;

template <int H>
__global__ __launch_bounds__(64 * kFusedWaves) __attribute__((amdgpu_waves_per_eu(H == 256 ? 6 : (H == 512 ? 4 : 2)))) void stft_fused_fwd_kernel(const FusedStftParams p) {
  typedef FusedFft<H> F;
  __shared__ __attribute__((aligned(16))) float4 s_buf[kFusedWaves][F::SLOTS];
  __shared__ float2 s_tw[H + 1];
  __shared__ float s_red[3][kFusedWaves];
  const int lane = threadIdx.x & 63, wave = uniform(threadIdx.x >> 6);
  fused_load_tables<H>(p, s_tw);
  float4 *buf = s_buf[wave];
  float s1 = 0.f, s2 = 0.f, s3 = 0.f;
  const int nw = gridDim.x * kFusedWaves, n_total = (int)p.n_total, n_frames = (int)p.n_frames;   // (< 2^31: checked on the host)
  for (int fr = blockIdx.x * kFusedWaves + wave; fr < n_total; fr += nw) {
    const int b = fr / n_frames, f = fr - b * n_frames;
    if (f < p.frame0) continue;
    const bool same = fused_load_frame<H>(p, b, f, lane, buf);
    const float s1_in = s1, s3_in = s3;
    F::stage_fence();
    F::forward(buf, s_tw, lane);
    // bins in mirror pairs (j, H - j): both need exactly Z[j] and Z[H - j] -- one pair of LDS reads, two bins
#pragma unroll 1
    for (int i = 0; i <= F::PER / 2; ++i) {
      const int j = lane + 64 * i;
      if (j > H / 2) break;
      const int m = j == 0 ? 0 : H - j;
      const float4 vj = buf[F::pad(F::pos(j))], vm = buf[F::pad(F::pos(m))];
      const float2 xj = make_float2(vj.x, vj.y), yj = make_float2(vj.z, vj.w), xm = make_float2(vm.x, vm.y), ym = make_float2(vm.z, vm.w);
      if (j == 0) {                                       // X[0] = Re z + Im z, X[H] = Re z - Im z (both real)
        fused_terms(make_float2(xj.x + xj.y, 0.f), make_float2(yj.x + yj.y, 0.f), s1, s2, s3);
        fused_terms(make_float2(xj.x - xj.y, 0.f), make_float2(yj.x - yj.y, 0.f), s1, s2, s3);
      } else {
        const float2 wj = s_tw[j];
        fused_terms(packed_bin(xj, xm, wj), packed_bin(yj, ym, wj), s1, s2, s3);
        if (m != j) {
          const float2 wm = s_tw[m];
          fused_terms(packed_bin(xm, xj, wm), packed_bin(ym, yj, wm), s1, s2, s3);
        }
      }
    }
    if (same) { s1 = s1_in; s3 = s3_in; }                 // x == y over the frame: only |Y|^2 counts
    F::stage_fence();                                     // (the next frame's load overwrites what other lanes just read)
  }
  float v[3] = {s1, s2, s3};
#pragma unroll
  for (int j = 0; j < 3; ++j) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v[j] += __shfl_xor(v[j], o, 64);
    if (lane == 0) s_red[j][wave] = v[j];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < kFusedWaves; ++w) t += s_red[threadIdx.x][w];
    p.partials[3 * (int64_t)blockIdx.x + threadIdx.x] = t;
  }
}

template <int H>
__global__ __launch_bounds__(64 * kFusedWaves) __attribute__((amdgpu_waves_per_eu(H == 256 ? 6 : (H == 512 ? 4 : 2)))) void stft_fused_bwd_kernel(const FusedStftParams p) {
  typedef FusedFft<H> F;
  __shared__ __attribute__((aligned(16))) float4 s_buf[kFusedWaves][F::SLOTS];
  __shared__ float2 s_tw[H + 1];
  const int lane = threadIdx.x & 63, wave = uniform(threadIdx.x >> 6);
  fused_load_tables<H>(p, s_tw);
  float4 *buf = s_buf[wave];
  const float c_sc = p.stats[2] > 0.f ? p.g_sc[0] / (p.stats[2] * p.stats[3]) : 0.f;   // 0 at |Y| = |X|, as torch's norm backward
  const float c_mag = p.g_mag[0] * p.inv_count;
  const int n_fft = 2 * H, off = (n_fft - p.win_len) / 2;
  const int nw = gridDim.x * kFusedWaves, n_total = (int)p.n_total, n_frames = (int)p.n_frames;
  for (int fr = blockIdx.x * kFusedWaves + wave; fr < n_total; fr += nw) {
    const int b = fr / n_frames, f = fr - b * n_frames;
    float *dst = p.dframes + (int64_t)fr * n_fft;
    // outside the band, or x == y over the frame: no gradient, but cum_stft_fold reads the support
    const bool same = f >= p.frame0 && fused_load_frame<H>(p, b, f, lane, buf);
    if (f < p.frame0 || same) {
#pragma unroll
      for (int i = 0; i < F::PER; ++i) {
        const int n = 2 * (lane + 64 * i);
        if (n + 1 >= off && n < off + p.win_len) *reinterpret_cast<float2 *>(dst + n) = make_float2(0.f, 0.f);
      }
      F::stage_fence();
      continue;
    }
    F::stage_fence();
    F::forward(buf, s_tw, lane);
    // gradient spectrum gz over the transforms, in place: lanes own disjoint (j, H - j) pairs
#pragma unroll 1
    for (int i = 0; i <= F::PER / 2; ++i) {
      const int j = lane + 64 * i;
      if (j > H / 2) break;
      const int m = j == 0 ? 0 : H - j;
      const int pj = F::pad(F::pos(j)), pm = F::pad(F::pos(m));
      const float4 vj = buf[pj], vm = buf[pm];
      const float2 xj = make_float2(vj.x, vj.y), yj = make_float2(vj.z, vj.w), xm = make_float2(vm.x, vm.y), ym = make_float2(vm.z, vm.w);
      float2 oj, om = make_float2(0.f, 0.f);
      if (j == 0) {
        const float2 g0 = fused_bin_grad(make_float2(xj.x + xj.y, 0.f), make_float2(yj.x + yj.y, 0.f), c_sc, c_mag);
        const float2 gh = fused_bin_grad(make_float2(xj.x - xj.y, 0.f), make_float2(yj.x - yj.y, 0.f), c_sc, c_mag);
        oj = make_float2(g0.x + gh.x, g0.x - gh.x);
      } else {
        const float2 wj = s_tw[j], wm = s_tw[H - j];
        const float2 gj = fused_bin_grad(packed_bin(xj, xm, wj), packed_bin(yj, ym, wj), c_sc, c_mag);
        const float2 gm = fused_bin_grad(packed_bin(xm, xj, wm), packed_bin(ym, yj, wm), c_sc, c_mag);
        const float2 c1j = make_float2(0.5f * (1.f + wj.y), 0.5f * wj.x), c2j = make_float2(0.5f * (1.f - wj.y), 0.5f * wj.x);
        const float2 c1m = make_float2(0.5f * (1.f + wm.y), 0.5f * wm.x), c2m = make_float2(0.5f * (1.f - wm.y), 0.5f * wm.x);
        const float2 a = cmul(c1j, gj), bq = cmul(c2m, conjf2(gm));
        oj = make_float2(a.x + bq.x, a.y + bq.y);
        const float2 c = cmul(c1m, gm), d = cmul(c2j, conjf2(gj));
        om = make_float2(c.x + d.x, c.y + d.y);
      }
      *reinterpret_cast<float2 *>(&buf[pj]) = oj;
      if (m != j) *reinterpret_cast<float2 *>(&buf[pm]) = om;
    }
    F::stage_fence();
    F::inverse_xy(buf, s_tw, lane);
    // frame gradient: sample 2m in the real part, 2m + 1 in the imaginary part; only the window's support is ever read
#pragma unroll
    for (int i = 0; i < F::PER; ++i) {
      const int mm = lane + 64 * i, n = 2 * mm;
      if (n + 1 >= off && n < off + p.win_len) {
        const float4 v = buf[F::pad(mm)];
        *reinterpret_cast<float2 *>(dst + n) = make_float2(v.x, v.y);
      }
    }
    F::stage_fence();                                     // (the next frame's load overwrites what other lanes just read)
  }
}

}  // namespace cum

using namespace cum;

static int check_resolution(int64_t len, int n_fft, int hop, int win_len, int64_t n_frames) {
  CUM_REQUIRE(n_fft >= 8 && n_fft % 4 == 0 && hop > 0 && win_len > 0 && win_len <= n_fft, "stft: bad resolution");
  CUM_REQUIRE(len > n_fft / 2, "stft: signal shorter than the reflect padding");
  CUM_REQUIRE(n_frames == 1 + len / hop, "stft: n_frames must be 1 + len / hop");
  return CUM_OK;
}

extern "C" int cum_stft_frames(const float *x, int64_t batch, int64_t len, int64_t x_stride_b, int32_t n_fft,
                               int32_t hop, int32_t win_length, const float *window, float *frames, int64_t n_frames,
                               void *stream) {
  CUM_REQUIRE(batch >= 0 && batch < 65536, "stft_frames: bad batch");
  if (int rc = check_resolution(len, n_fft, hop, win_length, n_frames)) return rc;
  if (batch == 0) return CUM_OK;
  CUM_REQUIRE(x && window && frames, "stft_frames: null pointer");
  hipLaunchKernelGGL(stft_frames_kernel, dim3((unsigned)n_frames, (unsigned)batch), dim3(256), 0, (hipStream_t)stream,
                     x, len, x_stride_b, n_fft, hop, win_length, window, frames, n_frames);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}

extern "C" int64_t cum_stft_loss_workspace_elems(int64_t batch, int64_t n_frames) {
  return 3 * cdiv64(batch * n_frames, kLossRows);
}

extern "C" int cum_stft_loss_fwd(const float *spec_x, const float *spec_y, int64_t batch, int64_t n_frames,
                                 int32_t bins, int64_t frame0, float *workspace, float *stats, void *stream) {
  CUM_REQUIRE(batch > 0 && n_frames > 0 && bins > 0 && frame0 >= 0 && frame0 < n_frames, "stft_loss_fwd: bad shape");
  CUM_REQUIRE(spec_x && spec_y && workspace && stats, "stft_loss_fwd: null pointer");
  const int64_t rows = batch * n_frames, parts = cdiv64(rows, kLossRows);
  hipLaunchKernelGGL(stft_loss_partials_kernel, dim3((unsigned)parts), dim3(256), 0, (hipStream_t)stream,
                     (const float2 *)spec_x, (const float2 *)spec_y, rows, n_frames, bins, frame0, workspace);
  const double count = (double)batch * (double)(n_frames - frame0) * (double)bins;
  hipLaunchKernelGGL(stft_loss_finalize_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, workspace, parts, count,
                     stats);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}

extern "C" int cum_stft_loss_bwd(const float *spec_x, const float *spec_y, int64_t batch, int64_t n_frames,
                                 int32_t bins, int64_t frame0, const float *stats, const float *g_sc,
                                 const float *g_mag, float *zspec, void *stream) {
  CUM_REQUIRE(batch > 0 && n_frames > 0 && bins > 0 && frame0 >= 0 && frame0 < n_frames, "stft_loss_bwd: bad shape");
  CUM_REQUIRE(spec_x && spec_y && stats && g_sc && g_mag && zspec, "stft_loss_bwd: null pointer");
  const int64_t rows = batch * n_frames, parts = cdiv64(rows, kLossRows);
  const double count = (double)batch * (double)(n_frames - frame0) * (double)bins;
  hipLaunchKernelGGL(stft_loss_grad_kernel, dim3((unsigned)parts), dim3(256), 0, (hipStream_t)stream,
                     (const float2 *)spec_x, (const float2 *)spec_y, rows, n_frames, bins, frame0, stats, g_sc, g_mag,
                     (float)(1.0 / count), (float2 *)zspec);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}

extern "C" int cum_stft_fold(const float *dframes, int64_t batch, int64_t len, int32_t n_fft, int32_t hop,
                             int32_t win_length, const float *window, int64_t n_frames, float *dx,
                             int64_t dx_stride_b, int32_t accumulate, void *stream) {
  CUM_REQUIRE(batch >= 0 && batch < 65536, "stft_fold: bad batch");
  if (int rc = check_resolution(len, n_fft, hop, win_length, n_frames)) return rc;
  if (batch == 0) return CUM_OK;
  CUM_REQUIRE(dframes && window && dx, "stft_fold: null pointer");
  hipLaunchKernelGGL(stft_fold_kernel, dim3((unsigned)cdiv64(len, 256), (unsigned)batch), dim3(256), 0,
                     (hipStream_t)stream, dframes, len, n_fft, hop, win_length, window, n_frames, dx, dx_stride_b,
                     accumulate);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}

extern "C" int cum_stft_loss_fwd_packed(const float *zx, const float *zy, int64_t batch, int64_t n_frames, int32_t n_fft,
                                        int64_t frame0, const float *twiddle, float *workspace, float *stats,
                                        void *stream) {
  CUM_REQUIRE(batch > 0 && n_frames > 0 && n_fft >= 8 && n_fft % 4 == 0 && frame0 >= 0 && frame0 < n_frames,
              "stft_loss_fwd_packed: bad shape");
  CUM_REQUIRE(zx && zy && twiddle && workspace && stats, "stft_loss_fwd_packed: null pointer");
  const int64_t rows = batch * n_frames, parts = cdiv64(rows, kLossRows);
  const int H = n_fft / 2;
  hipLaunchKernelGGL(stft_loss_partials_packed_kernel, dim3((unsigned)parts), dim3(256), 0, (hipStream_t)stream,
                     (const float2 *)zx, (const float2 *)zy, rows, n_frames, H, frame0, (const float2 *)twiddle,
                     workspace);
  const double count = (double)batch * (double)(n_frames - frame0) * (double)(H + 1);
  hipLaunchKernelGGL(stft_loss_finalize_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, workspace, parts, count,
                     stats);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}

extern "C" int cum_stft_loss_bwd_packed(const float *zx, const float *zy, int64_t batch, int64_t n_frames, int32_t n_fft,
                                        int64_t frame0, const float *stats, const float *g_sc, const float *g_mag,
                                        const float *twiddle, float *gz, void *stream) {
  CUM_REQUIRE(batch > 0 && n_frames > 0 && n_fft >= 8 && n_fft % 4 == 0 && frame0 >= 0 && frame0 < n_frames,
              "stft_loss_bwd_packed: bad shape");
  CUM_REQUIRE(zx && zy && stats && g_sc && g_mag && twiddle && gz, "stft_loss_bwd_packed: null pointer");
  const int64_t rows = batch * n_frames, parts = cdiv64(rows, kLossRows);
  const int H = n_fft / 2;
  const double count = (double)batch * (double)(n_frames - frame0) * (double)(H + 1);
  hipLaunchKernelGGL(stft_loss_grad_packed_kernel, dim3((unsigned)parts), dim3(256), 0, (hipStream_t)stream,
                     (const float2 *)zx, (const float2 *)zy, rows, n_frames, H, frame0, stats, g_sc, g_mag,
                     (float)(1.0 / count), (const float2 *)twiddle, (float2 *)gz);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}

// ---- fused entries (n_fft in {512, 1024, 2048}: cum_stft_fused_supported)
extern "C" int cum_stft_fused_supported(int32_t n_fft) { return n_fft == 512 || n_fft == 1024 || n_fft == 2048; }

static int fused_grid(int64_t n_total) {
  // a multiple of the CU count, enough waves to cover the frames at a few frames per wave; a function of the shape only,
  // so the partial sums (one per workgroup, fixed order) are reproducible
  const int64_t want = cdiv64(n_total, 4 * kFusedWaves);
  const int64_t g = want < 256 ? (want < 1 ? 1 : want) : (want < 2048 ? cdiv64(want, 256) * 256 : 2048);
  return (int)g;
}

extern "C" int64_t cum_stft_fused_workspace_elems(int64_t batch, int64_t n_frames) { return 3 * (int64_t)fused_grid(batch * n_frames); }

static int fused_params(FusedStftParams &p, const float *x, const float *y, int64_t batch, int64_t len, int64_t x_sb,
                        int64_t y_sb, int32_t n_fft, int32_t hop, int32_t win_length, const float *window,
                        const float *twiddle, int64_t n_frames, int64_t frame0) {
  CUM_REQUIRE(cum_stft_fused_supported(n_fft), "stft_fused: n_fft must be 512, 1024 or 2048");
  CUM_REQUIRE(batch > 0 && batch < 65536 && frame0 >= 0 && frame0 < n_frames && batch * n_frames < 2147483647LL,
              "stft_fused: bad batch / frame0");
  if (int rc = check_resolution(len, n_fft, hop, win_length, n_frames)) return rc;
  CUM_REQUIRE(x && y && window && twiddle, "stft_fused: null pointer");
  p.x = x; p.y = y; p.window = window; p.tw = twiddle;
  p.len = len; p.x_sb = x_sb; p.y_sb = y_sb; p.n_frames = n_frames; p.frame0 = frame0; p.n_total = batch * n_frames;
  p.hop = hop; p.win_len = win_length;
  return CUM_OK;
}

extern "C" int cum_stft_fused_fwd(const float *x, const float *y, int64_t batch, int64_t len, int64_t x_stride_b,
                                  int64_t y_stride_b, int32_t n_fft, int32_t hop, int32_t win_length, const float *window,
                                  const float *twiddle, int64_t n_frames, int64_t frame0, float *workspace, float *stats,
                                  void *stream) {
  FusedStftParams p{};
  if (int rc = fused_params(p, x, y, batch, len, x_stride_b, y_stride_b, n_fft, hop, win_length, window, twiddle, n_frames, frame0)) return rc;
  CUM_REQUIRE(workspace && stats, "stft_fused_fwd: null pointer");
  p.partials = workspace;
  const int grid = fused_grid(p.n_total);
  hipStream_t st = (hipStream_t)stream;
  if (n_fft == 512) hipLaunchKernelGGL(stft_fused_fwd_kernel<256>, dim3(grid), dim3(64 * kFusedWaves), 0, st, p);
  else if (n_fft == 1024) hipLaunchKernelGGL(stft_fused_fwd_kernel<512>, dim3(grid), dim3(64 * kFusedWaves), 0, st, p);
  else hipLaunchKernelGGL(stft_fused_fwd_kernel<1024>, dim3(grid), dim3(64 * kFusedWaves), 0, st, p);
  CUM_CHECK_LAUNCH();
  const double count = (double)batch * (double)(n_frames - frame0) * (double)(n_fft / 2 + 1);
  hipLaunchKernelGGL(stft_loss_finalize_kernel, dim3(1), dim3(1024), 0, st, workspace, (int64_t)grid, count, stats);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}

extern "C" int cum_stft_fused_bwd(const float *x, const float *y, int64_t batch, int64_t len, int64_t x_stride_b,
                                  int64_t y_stride_b, int32_t n_fft, int32_t hop, int32_t win_length, const float *window,
                                  const float *twiddle, int64_t n_frames, int64_t frame0, const float *stats,
                                  const float *g_sc, const float *g_mag, float *dframes, void *stream) {
  FusedStftParams p{};
  if (int rc = fused_params(p, x, y, batch, len, x_stride_b, y_stride_b, n_fft, hop, win_length, window, twiddle, n_frames, frame0)) return rc;
  CUM_REQUIRE(stats && g_sc && g_mag && dframes && ((uintptr_t)dframes & 7) == 0, "stft_fused_bwd: null or misaligned pointer");
  p.stats = stats; p.g_sc = g_sc; p.g_mag = g_mag; p.dframes = dframes;
  const double count = (double)batch * (double)(n_frames - frame0) * (double)(n_fft / 2 + 1);
  p.inv_count = (float)(1.0 / count);
  const int grid = fused_grid(p.n_total);
  hipStream_t st = (hipStream_t)stream;
  if (n_fft == 512) hipLaunchKernelGGL(stft_fused_bwd_kernel<256>, dim3(grid), dim3(64 * kFusedWaves), 0, st, p);
  else if (n_fft == 1024) hipLaunchKernelGGL(stft_fused_bwd_kernel<512>, dim3(grid), dim3(64 * kFusedWaves), 0, st, p);
  else hipLaunchKernelGGL(stft_fused_bwd_kernel<1024>, dim3(grid), dim3(64 * kFusedWaves), 0, st, p);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}
