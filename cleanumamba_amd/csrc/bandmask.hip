// BandMask for gfx950: the band-stop stage of the training augmentation, in front of cum_augment_pairs.
//
//   cum_band_mask_pairs   <- the hook `noise, clean_audio = augment((noise, clean_audio))` of the train loop
//                            (src/training/train.py:262-265): remove one mel band from speech and noisy alike, as the
//                            BandMask of the denoiser lineage does
//
// The filter of a row is h = delta + lowpass(c_lo) - lowpass(c_hi), two Hamming-windowed sincs of half-width W <= 1600:
// up to 3 201 taps, applied by overlap-save on the in-LDS FFT of fft_lds.h at N = 4096.  Two launches:
//   band_filter   one workgroup per row: the taps in f64, rounded to f32, placed circularly (h[k] at k mod N), one forward
//                 transform, the spectrum times 1 / N into the workspace in the transform's own digit-reversed order.
//                 Workgroup 0 also leaves the twiddle table (f64 sincospi, rounded once) at the head of the workspace.
//   band_apply    one wave per block of N samples starting at j V - W (V = N - 2 W valid outputs), zero outside the
//                 row: z = C + i Y, one forward transform, one multiply by the row's spectrum, one inverse; h is real, so
//                 Re and Im are the two filtered signals.  Outputs [j V, j V + V) of both are stored.
// A row with W = 0 is copied.  No atomics: every output is computed once, by one wave, in one order that depends on
// (n, W) alone -- not on the batch, the grid or the row's place in it.
#include <atomic>

#include "common.h"
#include "fft_lds.h"

namespace cum {

constexpr int kBandN = 4096;             // block length (why not 8192)
constexpr int kBandWaves = 3;            // blocks in flight per workgroup: 32 KB of twiddles + 3 x 34 KB of 160 KB
constexpr int kBandWMax = 1600;
constexpr int kBandFilterThreads = 256;
constexpr int kBandBatch = 16;           // global loads a lane of band_apply keeps in flight
typedef FusedFft<kBandN> BandFft;
constexpr int kBandTwBytes = ((kBandN + 1) * 8 + 15) / 16 * 16;       // tw[0..N], the next buffer on a 16-byte boundary
constexpr int kBandBufBytes = BandFft::SLOTS * 8;
constexpr int kBandTwFloats = kBandTwBytes / 4;                        // the same table at the head of the workspace
static_assert(kBandBufBytes % 16 == 0 && kBandTwBytes + kBandWaves * kBandBufBytes <= 160 * 1024, "LDS of one CU");

typedef float float4b __attribute__((ext_vector_type(4)));

// (W, c_lo, c_hi) of a record {W, c_lo bits, c_hi bits, 0}: W clamped into [0, 1600]; a cutoff that is not finite or
// outside 0 <= c_lo <= c_hi <= 0.5 makes the row a copy (W = 0), so a bad table cannot index anywhere
__device__ __forceinline__ int band_row(const int32_t *__restrict__ rec, float &c_lo, float &c_hi) {
  int W = rec[0];
  W = W < 0 ? 0 : (W > kBandWMax ? kBandWMax : W);
  c_lo = __builtin_bit_cast(float, rec[1]);
  c_hi = __builtin_bit_cast(float, rec[2]);
  const bool ok = c_lo >= 0.f && c_lo <= c_hi && c_hi <= 0.5f;        // (false for a NaN; an infinity fails a side)
  return ok ? W : 0;
}

// 2 c sinc(2 c k) in f64, sinc(x) = sin(pi x) / (pi x)
__device__ __forceinline__ double band_lowpass(double c, int k) {
  if (k == 0 || c == 0.0) return k == 0 ? 2.0 * c : 0.0;
  const double x = 2.0 * c * (double)k;
  return 2.0 * c * (sinpi(x) / (3.14159265358979323846 * x));
}

__global__ __launch_bounds__(kBandFilterThreads) void band_filter_kernel(const int32_t *__restrict__ recs,
                                                                        float *__restrict__ workspace) {
  extern __shared__ __attribute__((aligned(16))) char band_lds[];
  float2 *tw = reinterpret_cast<float2 *>(band_lds);
  float2 *buf = reinterpret_cast<float2 *>(band_lds + kBandTwBytes);
  const int b = blockIdx.x, tid = threadIdx.x;
  float c_lo, c_hi;
  const int W = band_row(recs + 4 * (int64_t)b, c_lo, c_hi);
  if (W == 0 && b != 0) return;                            // (uniform over the workgroup)
  for (int k = tid; k <= kBandN; k += kBandFilterThreads) {                    // tw[m] = e^{-2 pi i m / (2 N)}
    double s, c;
    sincospi((double)k / (double)kBandN, &s, &c);
    tw[k] = make_float2((float)c, (float)-s);
    if (b == 0) reinterpret_cast<float2 *>(workspace)[k] = tw[k];
  }
  if (W == 0) return;
  for (int e = tid; e < BandFft::SLOTS; e += kBandFilterThreads) buf[e] = make_float2(0.f, 0.f);
  __syncthreads();
  const double lo = (double)c_lo, hi = (double)c_hi;
  for (int i = tid; i <= 2 * W; i += kBandFilterThreads) {
    const int k = i - W;
    const double w = 0.54 - 0.46 * cospi((double)i / (double)W);
    // (the difference before the window: with c_lo == c_hi it is exactly 0 whatever the compiler contracts)
    const double h = (k == 0 ? 1.0 : 0.0) + (band_lowpass(lo, k) - band_lowpass(hi, k)) * w;
    buf[BandFft::pad(k & (kBandN - 1))] = make_float2((float)h, 0.f);
  }
  __syncthreads();
  if (tid < 64) BandFft::forward_c(buf, tw, tid);
  __syncthreads();
  float2 *__restrict__ spec = reinterpret_cast<float2 *>(workspace + kBandTwFloats) + (int64_t)b * kBandN;
  const float inv_n = 1.f / (float)kBandN;                 // (a power of two: the inverse's scale, exact)
  for (int e = tid; e < kBandN; e += kBandFilterThreads) {
    const float2 v = buf[BandFft::pad(e)];
    spec[e] = make_float2(v.x * inv_n, v.y * inv_n);
  }
}

// row[t] = get(t) for t in [t0, t1), one wave: scalar stores up to the first 16-byte boundary of the run, 16-byte stores
// from there on, scalar stores for the last t1 mod 4
template <typename F>
__device__ __forceinline__ void band_store_run(float *__restrict__ row, int64_t t0, int64_t t1, int lane, F get) {
  int64_t a = t0 + ((4 - (int)((reinterpret_cast<uintptr_t>(row + t0) >> 2) & 3)) & 3);
  a = a < t1 ? a : t1;
  for (int64_t t = t0 + lane; t < a; t += 64) row[t] = get(t);
  const int64_t groups = (t1 - a) >> 2;
#pragma unroll 4
  for (int64_t g = lane; g < groups; g += 64) {
    const int64_t t = a + 4 * g;
    const float4b v = {get(t), get(t + 1), get(t + 2), get(t + 3)};
    *reinterpret_cast<float4b *>(row + t) = v;
  }
  for (int64_t t = a + 4 * groups + lane; t < t1; t += 64) row[t] = get(t);
}

__global__ __launch_bounds__(64 * kBandWaves) void band_apply_kernel(const float *__restrict__ csrc, int64_t csrc_sb,
                                                                    const float *__restrict__ ysrc, int64_t ysrc_sb,
                                                                    int64_t n, const int32_t *__restrict__ recs,
                                                                    const float *__restrict__ workspace,
                                                                    float *__restrict__ clean, int64_t clean_sb,
                                                                    float *__restrict__ noisy, int64_t noisy_sb) {
  extern __shared__ __attribute__((aligned(16))) char band_lds[];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = uniform(threadIdx.x >> 6);
  float c_lo, c_hi;
  const int W = band_row(recs + 4 * (int64_t)b, c_lo, c_hi);
  const int V = kBandN - 2 * W;
  const int64_t n_blocks = (n + V - 1) / V;
  const int64_t first = (int64_t)blockIdx.x * kBandWaves, step = (int64_t)gridDim.x * kBandWaves;
  if (first >= n_blocks) return;                           // (uniform over the workgroup: before any barrier)
  const float *__restrict__ cb = csrc + (int64_t)b * csrc_sb;
  const float *__restrict__ yb = ysrc + (int64_t)b * ysrc_sb;
  float *__restrict__ dc = clean + (int64_t)b * clean_sb;
  float *__restrict__ dn = noisy + (int64_t)b * noisy_sb;

  if (W == 0) {                                            // a copy, bit for bit
    for (int64_t j = first + wave; j < n_blocks; j += step) {
      const int64_t t0 = j * kBandN, t1 = t0 + kBandN < n ? t0 + kBandN : n;
      band_store_run(dc, t0, t1, lane, [&](int64_t t) { return cb[t]; });
      band_store_run(dn, t0, t1, lane, [&](int64_t t) { return yb[t]; });
    }
    return;
  }

  // Every global load below stands in a batch of kBandBatch loads with no branch around them (a point outside the
  // row reads the row's sample 0 and is zeroed afterwards): with one wave per SIMD nothing else hides a load's latency,
  // and a load per loop trip costs that latency 64 times per block.
  float2 *tw = reinterpret_cast<float2 *>(band_lds);
  {
    constexpr int kTrips = (kBandN + 64 * kBandWaves) / (64 * kBandWaves);   // ceil((N + 1) / threads)
    float2 w[kTrips];
#pragma unroll
    for (int r = 0; r < kTrips; ++r) {
      const int k = threadIdx.x + 64 * kBandWaves * r;
      w[r] = reinterpret_cast<const float2 *>(workspace)[k <= kBandN ? k : kBandN];
    }
#pragma unroll
    for (int r = 0; r < kTrips; ++r) {
      const int k = threadIdx.x + 64 * kBandWaves * r;
      if (k <= kBandN) tw[k] = w[r];
    }
  }
  __syncthreads();
  float2 *buf = reinterpret_cast<float2 *>(band_lds + kBandTwBytes + wave * kBandBufBytes);
  const float2 *__restrict__ spec = reinterpret_cast<const float2 *>(workspace + kBandTwFloats) + (int64_t)b * kBandN;
  for (int64_t j = first + wave; j < n_blocks; j += step) {
    const int64_t base = j * V - W;                        // sample of point 0; point i holds output base + i, W <= i < N - W
#pragma unroll 1
    for (int r0 = 0; r0 < kBandN / 64; r0 += kBandBatch) {
      float c[kBandBatch], y[kBandBatch];
#pragma unroll
      for (int u = 0; u < kBandBatch; ++u) {
        const int64_t t = base + lane + 64 * (r0 + u);
        const int64_t at = t >= 0 && t < n ? t : 0;
        c[u] = cb[at], y[u] = yb[at];
      }
#pragma unroll
      for (int u = 0; u < kBandBatch; ++u) {
        const int i = lane + 64 * (r0 + u);
        const int64_t t = base + i;
        const bool on_row = t >= 0 && t < n;
        buf[BandFft::pad(i)] = make_float2(on_row ? c[u] : 0.f, on_row ? y[u] : 0.f);
      }
    }
    BandFft::stage_fence();
    BandFft::forward_c(buf, tw, lane);
#pragma unroll 1
    for (int r0 = 0; r0 < kBandN / 64; r0 += kBandBatch) {
      float2 g[kBandBatch];
#pragma unroll
      for (int u = 0; u < kBandBatch; ++u) g[u] = spec[lane + 64 * (r0 + u)];
#pragma unroll
      for (int u = 0; u < kBandBatch; ++u) {
        const int e = lane + 64 * (r0 + u);
        buf[BandFft::pad(e)] = BandFft::cmul2(buf[BandFft::pad(e)], g[u]);
      }
    }
    BandFft::stage_fence();
    BandFft::inverse_c(buf, tw, lane);
    const int64_t t0 = j * V, t1 = t0 + V < n ? t0 + V : n;
    const float *out = reinterpret_cast<const float *>(buf);
    band_store_run(dc, t0, t1, lane, [&](int64_t t) { return out[2 * BandFft::pad((int)(t - base))]; });
    band_store_run(dn, t0, t1, lane, [&](int64_t t) { return out[2 * BandFft::pad((int)(t - base)) + 1]; });
    BandFft::stage_fence();                                // (the next block's load overwrites what other lanes just read)
  }
}

}  // namespace cum

using namespace cum;

extern "C" int32_t cum_band_mask_block(void) { return kBandN; }

extern "C" int64_t cum_band_mask_workspace_elems(int32_t batch) {
  if (batch < 1) return 0;
  return kBandTwFloats + 2 * (int64_t)batch * kBandN;      // the twiddle table, then one complex spectrum per row
}

// both kernels take more dynamic LDS than the default limit: raised once per device (the call costs tens of microseconds
// on the host, more than the launches it precedes)
static int band_lds_limits(int filter_bytes, int apply_bytes) {
  static std::atomic<uint64_t> done{0};
  int device = 0;
  hipError_t e = hipGetDevice(&device);
  if (e == hipSuccess && device >= 0 && device < 64 && ((done.load(std::memory_order_acquire) >> device) & 1)) return CUM_OK;
  if (e == hipSuccess)
    e = hipFuncSetAttribute((const void *)band_filter_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, filter_bytes);
  if (e == hipSuccess)
    e = hipFuncSetAttribute((const void *)band_apply_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, apply_bytes);
  if (e != hipSuccess) {
    cum_set_error(hipGetErrorString(e));
    return CUM_ELAUNCH;
  }
  if (device >= 0 && device < 64) done.fetch_or(uint64_t(1) << device, std::memory_order_release);
  return CUM_OK;
}

extern "C" int cum_band_mask_pairs(const float *clean_src, int64_t clean_src_sb, const float *noisy_src,
                                   int64_t noisy_src_sb, int32_t batch, int64_t n, const int32_t *recs, float *workspace,
                                   float *clean, int64_t clean_sb, float *noisy, int64_t noisy_sb, void *stream) {
  CUM_REQUIRE(batch >= 1, "band_mask_pairs: batch must be at least 1");
  CUM_REQUIRE(batch <= 32767, "band_mask_pairs: batch must be at most 32767 (rows on the grid's y axis)");
  CUM_REQUIRE(n >= 1, "band_mask_pairs: n must be at least 1");
  CUM_REQUIRE(clean_src_sb >= n && noisy_src_sb >= n, "band_mask_pairs: clean_src_sb and noisy_src_sb must be at least n");
  CUM_REQUIRE(clean_sb >= n && noisy_sb >= n, "band_mask_pairs: clean_sb and noisy_sb must be at least n");
  CUM_REQUIRE(clean_src && noisy_src && recs && workspace && clean && noisy, "band_mask_pairs: null pointer");
  CUM_REQUIRE(((reinterpret_cast<uintptr_t>(clean) | reinterpret_cast<uintptr_t>(noisy)) & 15) == 0,
              "band_mask_pairs: clean and noisy must be 16-byte aligned");
  CUM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "band_mask_pairs: workspace must be 8-byte aligned");
  CUM_REQUIRE(((reinterpret_cast<uintptr_t>(clean_src) | reinterpret_cast<uintptr_t>(noisy_src) |
                reinterpret_cast<uintptr_t>(recs)) & 3) == 0,
              "band_mask_pairs: clean_src, noisy_src and recs must be 4-byte aligned");
  // the grid cannot know a row's W (nothing is read on the host): room for the shortest block, V = N - 2 * 1600, capped
  // at about four workgroups per CU; a workgroup past its row's last block leaves at once, the others stride
  const int64_t most = cdiv64(cdiv64(n, kBandN - 2 * kBandWMax), kBandWaves);
  const int64_t cap = 1024 / batch > 1 ? 1024 / batch : 1;
  const dim3 grid((unsigned)(most < cap ? most : cap), (unsigned)batch);
  const int filter_lds = kBandTwBytes + kBandBufBytes, apply_lds = kBandTwBytes + kBandWaves * kBandBufBytes;
  const int rc = band_lds_limits(filter_lds, apply_lds);
  if (rc != CUM_OK) return rc;
  hipLaunchKernelGGL(band_filter_kernel, dim3((unsigned)batch), dim3(kBandFilterThreads), filter_lds, (hipStream_t)stream,
                     recs, workspace);
  CUM_CHECK_LAUNCH();
  hipLaunchKernelGGL(band_apply_kernel, grid, dim3(64 * kBandWaves), apply_lds, (hipStream_t)stream, clean_src,
                     clean_src_sb, noisy_src, noisy_src_sb, n, recs, (const float *)workspace, clean, clean_sb, noisy,
                     noisy_sb);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}
