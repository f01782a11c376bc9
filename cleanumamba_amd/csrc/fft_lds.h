// In-LDS complex FFT of one wave (FusedFft<H>) and the packed real-input spectrum (packed_bin), shared by the fused
// STFT loss (stft_loss.hip), the speech metrics (metrics.hip) and the band-mask FFT convolution (bandmask.hip).
#pragma once
#include "common.h"

namespace cum {

// ---- packed real FFT: the N real samples of a frame are transformed as H = N/2 complex numbers
// z[m] = x[2m] + i x[2m+1] by ONE complex FFT (Z), and the real-input spectrum is recovered where it is consumed:
//   X[k] = c1_k Z[k mod H] + c2_k conj(Z[(H-k) mod H]),  c1_k = (1 - i w_k)/2, c2_k = (1 + i w_k)/2, w_k = e^{-2 pi i k/N}
// for k = 0..H.  rocFFT's own r2c / c2r do the same with a separate pass over the spectrum before / after the
// complex FFT (r2c_even_post / c2r_even_pre: 0.4 ms per step); here that pass rides in the loss kernels.
__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 conjf2(float2 a) { return make_float2(a.x, -a.y); }
__device__ __forceinline__ float2 packed_bin(float2 za, float2 zb, float2 w) {
  // c1 = (1 - i w)/2 = ((1 + w.y) - i w.x)/2 ; c2 = (1 + i w)/2 = ((1 - w.y) + i w.x)/2
  const float2 c1 = make_float2(0.5f * (1.f + w.y), -0.5f * w.x), c2 = make_float2(0.5f * (1.f - w.y), 0.5f * w.x);
  const float2 p = cmul(c1, za), q = cmul(c2, conjf2(zb));
  return make_float2(p.x + q.x, p.y + q.y);
}
__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ double2 packed_bin(double2 za, double2 zb, double2 w) {
  const double2 c1 = make_double2(0.5 * (1.0 + w.y), -0.5 * w.x), c2 = make_double2(0.5 * (1.0 - w.y), 0.5 * w.x);
  const double2 p = cmul(c1, za), q = cmul(c2, make_double2(zb.x, -zb.y));
  return make_double2(p.x + q.x, p.y + q.y);
}

// Element types of FusedFft: f32 (the STFT loss) or f64 (the speech metrics, whose band energies span 100 dB)
template <typename T>
struct FftVec;
template <>
struct FftVec<float> {
  typedef float4 v4;
  typedef float2 v2;
  __device__ static __forceinline__ float4 mk4(float a, float b, float c, float d) { return make_float4(a, b, c, d); }
  __device__ static __forceinline__ float2 mk2(float a, float b) { return make_float2(a, b); }
};
template <>
struct FftVec<double> {
  typedef double4 v4;
  typedef double2 v2;
  __device__ static __forceinline__ double4 mk4(double a, double b, double c, double d) { return make_double4(a, b, c, d); }
  __device__ static __forceinline__ double2 mk2(double a, double b) { return make_double2(a, b); }
};

// Transform: the frame's n_fft real samples as H = n_fft / 2 complex points (packed_bin above), in-place radix-4
// decimation in frequency (one leading radix-2 stage when log2 H is odd); the output stands in base-4 digit-reversed order,
// X[k] at fused_pos(k) -- consumed in that order, never sorted.  The inverse is the exact transpose (decimation in time on
// the digit-reversed layout, conjugate twiddles), unnormalised like the rocFFT path.  LDS slot of point e: e + (e >> 4)
// (one pad slot per 16: the late stages' stride-4 / stride-16 accesses would otherwise meet on 4 of the 16 bank groups).
// Validated against numpy's FFT as a scalar model before it was written (index maps, twiddle exponents, the transpose).
template <int H, typename T = float>
struct FusedFft {
  typedef typename FftVec<T>::v4 V4;   // one point of both signals: x.re, x.im, y.re, y.im
  typedef typename FftVec<T>::v2 V2;
  __device__ static __forceinline__ V4 mk4(T a, T b, T c, T d) { return FftVec<T>::mk4(a, b, c, d); }
  __device__ static __forceinline__ V2 mk2(T a, T b) { return FftVec<T>::mk2(a, b); }
  static constexpr int LOGH = H == 256 ? 8 : H == 512 ? 9 : H == 1024 ? 10 : H == 2048 ? 11 : H == 4096 ? 12 : 13;
  static constexpr bool LEAD2 = (LOGH & 1) != 0;
  static constexpr int PER = H / 64;                 // points per lane
  static constexpr int SLOTS = H + H / 16;
  // Measured and not kept (tools/prof_stft.sh, same box; forward 76 / 80 / 108 us, backward 113 / 116 / 162 us as shipped):
  //   next frame's samples prefetched into registers while the current frame is transformed (+ window in registers):
  //     90 / 94 / 109 and 126 / 153 / 217 us -- the registers cost one to two waves per SIMD, and the waves ARE the
  //     latency hiding here (an ablation puts the exposed load phase at a third of the kernel: more waves, not prefetch);
  //   contiguous runs of frames per wave (L1 reuse of the overlapping windows) instead of round-robin: 86 / 86 / 114;
  //   W^2j, W^3j by complex multiplication instead of two more table look-ups: within noise.
  // butterflies of one stage a lane keeps in flight: H = 1024 fits two waves per SIMD (LDS capacity), which need some
  // instruction-level overlap of their own; the smaller sizes run four or five waves per SIMD on <= 106 registers.
  // (Keeping each lane's stage twiddles in registers across its frames instead of looking them up in LDS was measured
  //  slower at every size: the 18 ... 44 extra registers cost a wave per SIMD, 117 -> 130 us on the 1024-point backward.)
  static constexpr int UNR = H == 1024 ? 2 : H > 1024 ? 4 : 1;   // (H > 1024: the V2 form below, one wave per SIMD at most)

  __device__ static __forceinline__ int pad(int e) { return e + (e >> 4); }

  // position of bin k in the transform's output order
  __device__ static __forceinline__ int pos(int k) {
    int p = 0, rem = k, L = H;
    if constexpr (LEAD2) {
      p = (rem & 1) * (H / 2);
      rem >>= 1;
      L = H / 2;
    }
#pragma unroll
    for (int s = 0; s < (LOGH / 2); ++s) {
      p += (rem & 3) * (L >> 2);
      rem >>= 2;
      L >>= 2;
    }
    return p;
  }

  // e^{-2 pi i e / L} from the table tw[m] = e^{-2 pi i m / (2H)}, m = 0..H
  __device__ static __forceinline__ V2 twiddle(const V2 *tw, int e, int L) {
    int m = e * (2 * H / L);
    const bool neg = m > H;
    m = neg ? m - H : m;
    V2 w = tw[m];
    if (neg) { w.x = -w.x; w.y = -w.y; }
    return w;
  }

  __device__ static __forceinline__ V4 cmul4(V4 v, V2 w) {
    return mk4(v.x * w.x - v.y * w.y, v.x * w.y + v.y * w.x, v.z * w.x - v.w * w.y, v.z * w.y + v.w * w.x);
  }
  __device__ static __forceinline__ V4 add4(V4 a, V4 b) { return mk4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
  __device__ static __forceinline__ V4 sub4(V4 a, V4 b) { return mk4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }

  // Between two stages other LANES' stores are read back.  The LDS executes a wave's accesses in order, so no hardware
  // barrier is needed; what must not happen is the compiler moving a stage's loads above the previous stage's stores
  // (it sees only this lane's addresses).  A wavefront-scope fence + wave barrier pins that order at zero instructions.
  __device__ static __forceinline__ void stage_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }

  // forward transform of both signals (wave-private buffer: the LDS executes a wave's accesses in order, no barrier)
  __device__ static __forceinline__ void forward(V4 *buf, const V2 *tw, int lane) {
    int L = H;
    if constexpr (LEAD2) {
#pragma unroll UNR
      for (int i = 0; i < H / 128; ++i) {
        const int j = lane + 64 * i;                       // H / 2 butterflies
        const V4 a = buf[pad(j)], b = buf[pad(j + H / 2)];
        buf[pad(j)] = add4(a, b);
        buf[pad(j + H / 2)] = cmul4(sub4(a, b), twiddle(tw, j, H));
      }
      L = H / 2;
      stage_fence();
    }
#pragma unroll
    for (int st = 0; st < LOGH / 2; ++st, L >>= 2) {
      const int q4 = L >> 2;
#pragma unroll UNR
      for (int i = 0; i < H / 256; ++i) {
        const int q = lane + 64 * i;                       // H / 4 butterflies
        const int j = q & (q4 - 1), p = ((q - j) << 2) + j;   // group (q / q4) * L + j
        const V4 a = buf[pad(p)], b = buf[pad(p + q4)], c = buf[pad(p + 2 * q4)], d = buf[pad(p + 3 * q4)];
        const V4 t0 = add4(a, c), t1 = sub4(a, c), t2 = add4(b, d), u = sub4(b, d);
        const V4 t3 = mk4(u.y, -u.x, u.w, -u.z);                  // (b - d) * (-i)
        buf[pad(p)] = add4(t0, t2);
        if (L > 4) {
          buf[pad(p + q4)] = cmul4(add4(t1, t3), twiddle(tw, j, L));
          buf[pad(p + 2 * q4)] = cmul4(sub4(t0, t2), twiddle(tw, 2 * j, L));
          buf[pad(p + 3 * q4)] = cmul4(sub4(t1, t3), twiddle(tw, 3 * j, L));
        } else {                                                               // last stage: j = 0, twiddles are 1
          buf[pad(p + q4)] = add4(t1, t3);
          buf[pad(p + 2 * q4)] = sub4(t0, t2);
          buf[pad(p + 3 * q4)] = sub4(t1, t3);
        }
      }
      stage_fence();
    }
  }

  // unnormalised inverse of the .xy halves (input in the forward's output order, output in natural order)
  __device__ static __forceinline__ void inverse_xy(V4 *buf, const V2 *tw, int lane) {
    auto ld = [&](int e) { const V4 v = buf[pad(e)]; return mk2(v.x, v.y); };
    auto st2 = [&](int e, float2 v) { float2 *q = reinterpret_cast<float2 *>(&buf[pad(e)]); *q = v; };
    auto cmulc = [](float2 v, float2 w) { return make_float2(v.x * w.x + v.y * w.y, v.y * w.x - v.x * w.y); };   // v * conj(w)
    int L = 4;
#pragma unroll
    for (int stg = 0; stg < LOGH / 2; ++stg, L <<= 2) {
      const int q4 = L >> 2;
#pragma unroll UNR
      for (int i = 0; i < H / 256; ++i) {
        const int q = lane + 64 * i;
        const int j = q & (q4 - 1), p = ((q - j) << 2) + j;
        float2 a = ld(p), b = ld(p + q4), c = ld(p + 2 * q4), d = ld(p + 3 * q4);
        if (L > 4) {
          b = cmulc(b, twiddle(tw, j, L));
          c = cmulc(c, twiddle(tw, 2 * j, L));
          d = cmulc(d, twiddle(tw, 3 * j, L));
        }
        const float2 s0 = make_float2(a.x + c.x, a.y + c.y), s1 = make_float2(a.x - c.x, a.y - c.y);
        const float2 s2 = make_float2(b.x + d.x, b.y + d.y), u = make_float2(b.x - d.x, b.y - d.y);
        const float2 s3 = make_float2(-u.y, u.x);                              // i (b - d)
        st2(p, make_float2(s0.x + s2.x, s0.y + s2.y));
        st2(p + q4, make_float2(s1.x + s3.x, s1.y + s3.y));
        st2(p + 2 * q4, make_float2(s0.x - s2.x, s0.y - s2.y));
        st2(p + 3 * q4, make_float2(s1.x - s3.x, s1.y - s3.y));
      }
      stage_fence();
    }
    if constexpr (LEAD2) {
#pragma unroll UNR
      for (int i = 0; i < H / 128; ++i) {
        const int j = lane + 64 * i;
        const float2 a = ld(j), b = cmulc(ld(j + H / 2), twiddle(tw, j, H));
        st2(j, make_float2(a.x + b.x, a.y + b.y));
        st2(j + H / 2, make_float2(a.x - b.x, a.y - b.y));
      }
      stage_fence();
    }
  }
  // ---- one complex signal per buffer (V2 elements): the overlap-save blocks of bandmask.hip, H = 4096.  The same index
  // maps, twiddles and slot padding as the V4 form above; forward_c leaves X[k] at pos(k), inverse_c takes that order back
  // to natural order, unnormalised.
  __device__ static __forceinline__ V2 cmul2(V2 v, V2 w) { return mk2(v.x * w.x - v.y * w.y, v.x * w.y + v.y * w.x); }
  __device__ static __forceinline__ V2 cmul2c(V2 v, V2 w) { return mk2(v.x * w.x + v.y * w.y, v.y * w.x - v.x * w.y); }   // v conj(w)
  __device__ static __forceinline__ V2 add2(V2 a, V2 b) { return mk2(a.x + b.x, a.y + b.y); }
  __device__ static __forceinline__ V2 sub2(V2 a, V2 b) { return mk2(a.x - b.x, a.y - b.y); }

  __device__ static __forceinline__ void forward_c(V2 *buf, const V2 *tw, int lane) {
    int L = H;
    if constexpr (LEAD2) {
#pragma unroll UNR
      for (int i = 0; i < H / 128; ++i) {
        const int j = lane + 64 * i;
        const V2 a = buf[pad(j)], b = buf[pad(j + H / 2)];
        buf[pad(j)] = add2(a, b);
        buf[pad(j + H / 2)] = cmul2(sub2(a, b), twiddle(tw, j, H));
      }
      L = H / 2;
      stage_fence();
    }
#pragma unroll
    for (int st = 0; st < LOGH / 2; ++st, L >>= 2) {
      const int q4 = L >> 2;
#pragma unroll UNR
      for (int i = 0; i < H / 256; ++i) {
        const int q = lane + 64 * i;
        const int j = q & (q4 - 1), p = ((q - j) << 2) + j;
        const V2 a = buf[pad(p)], b = buf[pad(p + q4)], c = buf[pad(p + 2 * q4)], d = buf[pad(p + 3 * q4)];
        const V2 t0 = add2(a, c), t1 = sub2(a, c), t2 = add2(b, d), u = sub2(b, d);
        const V2 t3 = mk2(u.y, -u.x);                                          // (b - d) * (-i)
        buf[pad(p)] = add2(t0, t2);
        if (L > 4) {
          buf[pad(p + q4)] = cmul2(add2(t1, t3), twiddle(tw, j, L));
          buf[pad(p + 2 * q4)] = cmul2(sub2(t0, t2), twiddle(tw, 2 * j, L));
          buf[pad(p + 3 * q4)] = cmul2(sub2(t1, t3), twiddle(tw, 3 * j, L));
        } else {
          buf[pad(p + q4)] = add2(t1, t3);
          buf[pad(p + 2 * q4)] = sub2(t0, t2);
          buf[pad(p + 3 * q4)] = sub2(t1, t3);
        }
      }
      stage_fence();
    }
  }

  __device__ static __forceinline__ void inverse_c(V2 *buf, const V2 *tw, int lane) {
    int L = 4;
#pragma unroll
    for (int stg = 0; stg < LOGH / 2; ++stg, L <<= 2) {
      const int q4 = L >> 2;
#pragma unroll UNR
      for (int i = 0; i < H / 256; ++i) {
        const int q = lane + 64 * i;
        const int j = q & (q4 - 1), p = ((q - j) << 2) + j;
        V2 a = buf[pad(p)], b = buf[pad(p + q4)], c = buf[pad(p + 2 * q4)], d = buf[pad(p + 3 * q4)];
        if (L > 4) {
          b = cmul2c(b, twiddle(tw, j, L));
          c = cmul2c(c, twiddle(tw, 2 * j, L));
          d = cmul2c(d, twiddle(tw, 3 * j, L));
        }
        const V2 s0 = add2(a, c), s1 = sub2(a, c), s2 = add2(b, d), u = sub2(b, d);
        const V2 s3 = mk2(-u.y, u.x);                                          // i (b - d)
        buf[pad(p)] = add2(s0, s2);
        buf[pad(p + q4)] = add2(s1, s3);
        buf[pad(p + 2 * q4)] = sub2(s0, s2);
        buf[pad(p + 3 * q4)] = sub2(s1, s3);
      }
      stage_fence();
    }
    if constexpr (LEAD2) {
#pragma unroll UNR
      for (int i = 0; i < H / 128; ++i) {
        const int j = lane + 64 * i;
        const V2 a = buf[pad(j)], b = cmul2c(buf[pad(j + H / 2)], twiddle(tw, j, H));
        buf[pad(j)] = add2(a, b);
        buf[pad(j + H / 2)] = sub2(a, b);
      }
      stage_fence();
    }
  }
};

}  // namespace cum
