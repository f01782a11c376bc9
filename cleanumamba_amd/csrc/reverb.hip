// Room impulse responses for gfx950: the reverberation stage of the training augmentation, in front of the band mask and
// of cum_augment_pairs.
//
//   cum_reverb_pairs   <- the hook `noise, clean_audio = augment((noise, clean_audio))` of the train loop
//                         (src/training/train.py:262-265): convolve the speech of a row with a measured room response,
//                         as the DNS synthesiser does before it adds the noise
//
// Row b carries an id r = recs[4 b] into a bank of responses; h = bank[r] has T <= 16 384 dense f32 taps, h[0] the direct
// path.  Cr = h * C (causal, C zero outside the row), clean = Cr, noisy = (Y - C) + Cr.  Uniformly partitioned
// overlap-save on the in-LDS FFT of fft_lds.h at N = 4096, partitions and output blocks P = N / 2 long.  Three launches:
//   reverb_filter   one workgroup per (partition k, row): h[k P, (k + 1) P) zero-padded to N, one forward transform, the
//                   spectrum times 1 / N into the workspace in the transform's own digit-reversed order.  Workgroup (0, 0)
//                   also leaves the twiddle table (f64 sincospi, rounded once) at the head of the workspace.
//   reverb_blocks   one wave per input block j: C[(j - 1) P, (j + 1) P), zero outside the row, one forward transform, the
//                   spectrum X[j] into the workspace.  The imaginary lane stays empty.
//   reverb_apply    one wave per output block m: sum_{k < min(K, m + 1)} X[m - k] H[k], ascending k, one fma chain per
//                   component; one inverse transform; points [P, N) are Cr[m P, (m + 1) P).
// The products are element-wise, so no spectrum is ever sorted.  A row whose id is outside [0, n_rirs) is copied by
// reverb_apply and skipped by the other two.  No atomics: every output is computed once, by one wave, in one order that
// depends on (n, T) alone -- not on the batch, the grid or the row's place in it.
#include <atomic>

#include "common.h"
#include "fft_lds.h"

namespace cum {

constexpr int kRevN = 4096;              // FFT length
constexpr int kRevP = kRevN / 2;         // partition of the response = valid outputs per block
constexpr int kRevTMax = 16384;          // taps per response: 8 partitions
constexpr int kRevKMax = kRevTMax / kRevP;
constexpr int kRevWaves = 3;             // blocks in flight per workgroup: 32 KB of twiddles + 3 x 34 KB of 160 KB
constexpr int kRevFilterThreads = 256;
constexpr int kRevBatch = 16;            // global loads a lane keeps in flight
typedef FusedFft<kRevN> RevFft;
constexpr int kRevTwBytes = ((kRevN + 1) * 8 + 15) / 16 * 16;         // tw[0..N], the next buffer on a 16-byte boundary
constexpr int kRevBufBytes = RevFft::SLOTS * 8;
constexpr int kRevTwFloats = kRevTwBytes / 4;                          // the same table at the head of the workspace
static_assert(kRevBufBytes % 16 == 0 && kRevTwBytes + kRevWaves * kRevBufBytes <= 160 * 1024, "LDS of one CU");
static_assert(kRevTMax % kRevP == 0 && kRevN % (64 * kRevBatch) == 0, "whole partitions, whole load batches");

typedef float float4r __attribute__((ext_vector_type(4)));

// Taps T of row b's response and its first float in the blob, or 0: the row is a copy.  The id outside [0, n_rirs) is a
// copy; the device table is not trusted: an offset outside the blob is a copy, and T is clamped into [1, T_MAX] and then
// to what the blob holds behind the offset, so a bad table never indexes outside the blob.
__device__ __forceinline__ int reverb_row(const int32_t *__restrict__ recs, int b, const int32_t *__restrict__ rirs,
                                          int n_rirs, int64_t bank_floats, int64_t &off) {
  const int r = recs[4 * (int64_t)b];
  off = 0;
  if (r < 0 || r >= n_rirs) return 0;
  const int32_t *e = rirs + 4 * (int64_t)r;
  off = (int64_t)(((uint64_t)(uint32_t)e[1] << 32) | (uint64_t)(uint32_t)e[0]);
  if (off < 0 || off >= bank_floats) return 0;
  int T = e[2];
  T = T < 1 ? 1 : (T > kRevTMax ? kRevTMax : T);
  const int64_t room = bank_floats - off;
  return room < T ? (int)room : T;
}

__device__ __forceinline__ int64_t reverb_blocks_of(int64_t n) { return (n + kRevP - 1) / kRevP; }

// workspace: the twiddle table; batch x kRevKMax response spectra; batch x ceil(n / P) block spectra
__device__ __forceinline__ float2 *reverb_hspec(float *workspace, int b, int k) {
  return reinterpret_cast<float2 *>(workspace + kRevTwFloats) + ((int64_t)b * kRevKMax + k) * kRevN;
}
__device__ __forceinline__ float2 *reverb_xspec(float *workspace, int batch, int64_t n_blocks, int b, int64_t j) {
  return reinterpret_cast<float2 *>(workspace + kRevTwFloats) + ((int64_t)batch * kRevKMax + (int64_t)b * n_blocks + j) * kRevN;
}

// the workgroup's copy of the twiddle table, from the head of the workspace (every load in flight before the first store)
template <int THREADS>
__device__ __forceinline__ void reverb_load_twiddles(float2 *tw, const float *__restrict__ workspace) {
  constexpr int kTrips = (kRevN + THREADS) / THREADS;      // ceil((N + 1) / threads)
  float2 w[kTrips];
#pragma unroll
  for (int r = 0; r < kTrips; ++r) {
    const int k = threadIdx.x + THREADS * r;
    w[r] = reinterpret_cast<const float2 *>(workspace)[k <= kRevN ? k : kRevN];
  }
#pragma unroll
  for (int r = 0; r < kTrips; ++r) {
    const int k = threadIdx.x + THREADS * r;
    if (k <= kRevN) tw[k] = w[r];
  }
}

__global__ __launch_bounds__(kRevFilterThreads) void reverb_filter_kernel(const int32_t *__restrict__ recs,
                                                                         const float *__restrict__ bank, int64_t bank_floats,
                                                                         const int32_t *__restrict__ rirs, int n_rirs,
                                                                         float *__restrict__ workspace) {
  extern __shared__ __attribute__((aligned(16))) char rev_lds[];
  float2 *tw = reinterpret_cast<float2 *>(rev_lds);
  float2 *buf = reinterpret_cast<float2 *>(rev_lds + kRevTwBytes);
  const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const bool first = k == 0 && b == 0;
  int64_t off;
  const int T = reverb_row(recs, b, rirs, n_rirs, bank_floats, off);
  const bool mine = (int64_t)k * kRevP < T;                // (T = 0: no partition at all)
  if (!mine && !first) return;                             // (uniform over the workgroup)
  for (int m = tid; m <= kRevN; m += kRevFilterThreads) {                      // tw[m] = e^{-2 pi i m / (2 N)}
    double s, c;
    sincospi((double)m / (double)kRevN, &s, &c);
    tw[m] = make_float2((float)c, (float)-s);
    if (first) reinterpret_cast<float2 *>(workspace)[m] = tw[m];
  }
  if (!mine) return;
  const int have = T - k * kRevP < kRevP ? T - k * kRevP : kRevP;              // taps of this partition, 1 ... P
  const float *__restrict__ h = bank + off + (int64_t)k * kRevP;
  for (int e = tid; e < kRevN; e += kRevFilterThreads) buf[RevFft::pad(e)] = make_float2(e < have ? h[e] : 0.f, 0.f);
  __syncthreads();
  if (tid < 64) RevFft::forward_c(buf, tw, tid);
  __syncthreads();
  float2 *__restrict__ spec = reverb_hspec(workspace, b, k);
  const float inv_n = 1.f / (float)kRevN;                  // (a power of two: the inverse's scale, exact)
  for (int e = tid; e < kRevN; e += kRevFilterThreads) {
    const float2 v = buf[RevFft::pad(e)];
    spec[e] = make_float2(v.x * inv_n, v.y * inv_n);
  }
}

__global__ __launch_bounds__(64 * kRevWaves) void reverb_blocks_kernel(const float *__restrict__ csrc, int64_t csrc_sb,
                                                                      int batch, int64_t n, const int32_t *__restrict__ recs,
                                                                      int64_t bank_floats, const int32_t *__restrict__ rirs,
                                                                      int n_rirs, float *__restrict__ workspace) {
  extern __shared__ __attribute__((aligned(16))) char rev_lds[];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = uniform(threadIdx.x >> 6);
  const int64_t n_blocks = reverb_blocks_of(n);
  const int64_t first = (int64_t)blockIdx.x * kRevWaves, step = (int64_t)gridDim.x * kRevWaves;
  int64_t off;
  if (first >= n_blocks || reverb_row(recs, b, rirs, n_rirs, bank_floats, off) == 0) return;   // (uniform: before any barrier)
  const float *__restrict__ cb = csrc + (int64_t)b * csrc_sb;
  float2 *tw = reinterpret_cast<float2 *>(rev_lds);
  reverb_load_twiddles<64 * kRevWaves>(tw, workspace);
  __syncthreads();
  float2 *buf = reinterpret_cast<float2 *>(rev_lds + kRevTwBytes + wave * kRevBufBytes);
  for (int64_t j = first + wave; j < n_blocks; j += step) {
    const int64_t base = (j - 1) * kRevP;                  // sample of point 0
    // (branch-free batches of loads: a point outside the row reads the row's sample 0 and is zeroed afterwards)
#pragma unroll 1
    for (int r0 = 0; r0 < kRevN / 64; r0 += kRevBatch) {
      float c[kRevBatch];
#pragma unroll
      for (int u = 0; u < kRevBatch; ++u) {
        const int64_t t = base + lane + 64 * (r0 + u);
        c[u] = cb[t >= 0 && t < n ? t : 0];
      }
#pragma unroll
      for (int u = 0; u < kRevBatch; ++u) {
        const int i = lane + 64 * (r0 + u);
        const int64_t t = base + i;
        buf[RevFft::pad(i)] = make_float2(t >= 0 && t < n ? c[u] : 0.f, 0.f);
      }
    }
    RevFft::stage_fence();
    RevFft::forward_c(buf, tw, lane);
    float2 *__restrict__ spec = reverb_xspec(workspace, batch, n_blocks, b, j);
#pragma unroll 4
    for (int r = 0; r < kRevN / 64; ++r) spec[lane + 64 * r] = buf[RevFft::pad(lane + 64 * r)];
    RevFft::stage_fence();                                 // (the next block's load overwrites what other lanes just read)
  }
}

// row[t] = get(t) for t in [t0, t1), one wave: scalar stores up to the first 16-byte boundary of the run, 16-byte stores
// from there on, scalar stores for the last t1 mod 4
template <typename F>
__device__ __forceinline__ void reverb_store_run(float *__restrict__ row, int64_t t0, int64_t t1, int lane, F get) {
  int64_t a = t0 + ((4 - (int)((reinterpret_cast<uintptr_t>(row + t0) >> 2) & 3)) & 3);
  a = a < t1 ? a : t1;
  for (int64_t t = t0 + lane; t < a; t += 64) row[t] = get(t);
  const int64_t groups = (t1 - a) >> 2;
#pragma unroll 4
  for (int64_t g = lane; g < groups; g += 64) {
    const int64_t t = a + 4 * g;
    const float4r v = {get(t), get(t + 1), get(t + 2), get(t + 3)};
    *reinterpret_cast<float4r *>(row + t) = v;
  }
  for (int64_t t = a + 4 * groups + lane; t < t1; t += 64) row[t] = get(t);
}

__global__ __launch_bounds__(64 * kRevWaves) void reverb_apply_kernel(const float *__restrict__ csrc, int64_t csrc_sb,
                                                                     const float *__restrict__ ysrc, int64_t ysrc_sb,
                                                                     int batch, int64_t n, const int32_t *__restrict__ recs,
                                                                     int64_t bank_floats, const int32_t *__restrict__ rirs,
                                                                     int n_rirs, float *__restrict__ workspace,
                                                                     float *__restrict__ clean, int64_t clean_sb,
                                                                     float *__restrict__ noisy, int64_t noisy_sb) {
  extern __shared__ __attribute__((aligned(16))) char rev_lds[];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = uniform(threadIdx.x >> 6);
  const int64_t n_blocks = reverb_blocks_of(n);
  const int64_t first = (int64_t)blockIdx.x * kRevWaves, step = (int64_t)gridDim.x * kRevWaves;
  if (first >= n_blocks) return;                           // (uniform over the workgroup: before any barrier)
  int64_t off;
  const int T = reverb_row(recs, b, rirs, n_rirs, bank_floats, off);
  const float *__restrict__ cb = csrc + (int64_t)b * csrc_sb;
  const float *__restrict__ yb = ysrc + (int64_t)b * ysrc_sb;
  float *__restrict__ dc = clean + (int64_t)b * clean_sb;
  float *__restrict__ dn = noisy + (int64_t)b * noisy_sb;

  if (T == 0) {                                            // a copy, bit for bit
    for (int64_t m = first + wave; m < n_blocks; m += step) {
      const int64_t t0 = m * kRevP, t1 = t0 + kRevP < n ? t0 + kRevP : n;
      reverb_store_run(dc, t0, t1, lane, [&](int64_t t) { return cb[t]; });
      reverb_store_run(dn, t0, t1, lane, [&](int64_t t) { return yb[t]; });
    }
    return;
  }

  const int K = (T + kRevP - 1) / kRevP;
  float2 *tw = reinterpret_cast<float2 *>(rev_lds);
  reverb_load_twiddles<64 * kRevWaves>(tw, workspace);
  __syncthreads();
  float2 *buf = reinterpret_cast<float2 *>(rev_lds + kRevTwBytes + wave * kRevBufBytes);
  for (int64_t m = first + wave; m < n_blocks; m += step) {
    const int parts = m + 1 < K ? (int)(m + 1) : K;        // X[m - k] exists for k <= m
    const float2 *__restrict__ hs = reverb_hspec(workspace, b, 0);
    const float2 *__restrict__ xs = reverb_xspec(workspace, batch, n_blocks, b, m);
#pragma unroll 1
    for (int r0 = 0; r0 < kRevN / 64; r0 += kRevBatch) {
      float2 acc[kRevBatch];
#pragma unroll
      for (int u = 0; u < kRevBatch; ++u) acc[u] = make_float2(0.f, 0.f);
#pragma unroll 1
      for (int k = 0; k < parts; ++k) {                    // ascending k: one fma chain per component
        float2 x[kRevBatch], g[kRevBatch];
#pragma unroll
        for (int u = 0; u < kRevBatch; ++u) {
          const int e = lane + 64 * (r0 + u);
          x[u] = xs[e - (int64_t)k * kRevN], g[u] = hs[e + (int64_t)k * kRevN];
        }
#pragma unroll
        for (int u = 0; u < kRevBatch; ++u) {
          acc[u].x = fmaf(x[u].x, g[u].x, acc[u].x);
          acc[u].x = fmaf(-x[u].y, g[u].y, acc[u].x);
          acc[u].y = fmaf(x[u].x, g[u].y, acc[u].y);
          acc[u].y = fmaf(x[u].y, g[u].x, acc[u].y);
        }
      }
#pragma unroll
      for (int u = 0; u < kRevBatch; ++u) buf[RevFft::pad(lane + 64 * (r0 + u))] = acc[u];
    }
    RevFft::stage_fence();
    RevFft::inverse_c(buf, tw, lane);
    const int64_t t0 = m * kRevP, t1 = t0 + kRevP < n ? t0 + kRevP : n;
    const float *out = reinterpret_cast<const float *>(buf);
    auto cr = [&](int64_t t) { return out[2 * RevFft::pad((int)(t - t0) + kRevP)]; };
    reverb_store_run(dc, t0, t1, lane, cr);
    reverb_store_run(dn, t0, t1, lane, [&](int64_t t) { return (yb[t] - cb[t]) + cr(t); });
    RevFft::stage_fence();                                 // (the next block's products overwrite what other lanes just read)
  }
}

}  // namespace cum

using namespace cum;

extern "C" int32_t cum_reverb_block(void) { return kRevN; }

extern "C" int32_t cum_reverb_max_taps(void) { return kRevTMax; }

extern "C" int64_t cum_reverb_workspace_elems(int32_t batch, int64_t n) {
  if (batch < 1 || n < 1) return 0;
  // the twiddle table, then per row the spectra of kRevKMax partitions and of ceil(n / P) input blocks
  return kRevTwFloats + 2 * (int64_t)batch * kRevN * (kRevKMax + cdiv64(n, kRevP));
}

// the kernels take more dynamic LDS than the default limit: raised once per device
static int reverb_lds_limits(int filter_bytes, int wave_bytes) {
  static std::atomic<uint64_t> done{0};
  int device = 0;
  hipError_t e = hipGetDevice(&device);
  if (e == hipSuccess && device >= 0 && device < 64 && ((done.load(std::memory_order_acquire) >> device) & 1)) return CUM_OK;
  if (e == hipSuccess)
    e = hipFuncSetAttribute((const void *)reverb_filter_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, filter_bytes);
  if (e == hipSuccess)
    e = hipFuncSetAttribute((const void *)reverb_blocks_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, wave_bytes);
  if (e == hipSuccess)
    e = hipFuncSetAttribute((const void *)reverb_apply_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, wave_bytes);
  if (e != hipSuccess) {
    cum_set_error(hipGetErrorString(e));
    return CUM_ELAUNCH;
  }
  if (device >= 0 && device < 64) done.fetch_or(uint64_t(1) << device, std::memory_order_release);
  return CUM_OK;
}

extern "C" int cum_reverb_pairs(const float *clean_src, int64_t clean_src_sb, const float *noisy_src, int64_t noisy_src_sb,
                                int32_t batch, int64_t n, const int32_t *recs, const float *bank, int64_t bank_floats,
                                const int32_t *rirs_host, const int32_t *rirs, int32_t n_rirs, float *workspace,
                                float *clean, int64_t clean_sb, float *noisy, int64_t noisy_sb, void *stream) {
  CUM_REQUIRE(batch >= 1, "reverb_pairs: batch must be at least 1");
  CUM_REQUIRE(batch <= 32767, "reverb_pairs: batch must be at most 32767 (rows on the grid's y axis)");
  CUM_REQUIRE(n >= 1, "reverb_pairs: n must be at least 1");
  CUM_REQUIRE(clean_src_sb >= n && noisy_src_sb >= n, "reverb_pairs: clean_src_sb and noisy_src_sb must be at least n");
  CUM_REQUIRE(clean_sb >= n && noisy_sb >= n, "reverb_pairs: clean_sb and noisy_sb must be at least n");
  CUM_REQUIRE(clean_src && noisy_src && recs && workspace && clean && noisy && bank && rirs_host && rirs,
              "reverb_pairs: null pointer");
  CUM_REQUIRE(((reinterpret_cast<uintptr_t>(clean) | reinterpret_cast<uintptr_t>(noisy)) & 15) == 0,
              "reverb_pairs: clean and noisy must be 16-byte aligned");
  CUM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "reverb_pairs: workspace must be 8-byte aligned");
  CUM_REQUIRE(((reinterpret_cast<uintptr_t>(clean_src) | reinterpret_cast<uintptr_t>(noisy_src) |
                reinterpret_cast<uintptr_t>(recs) | reinterpret_cast<uintptr_t>(bank) |
                reinterpret_cast<uintptr_t>(rirs_host) | reinterpret_cast<uintptr_t>(rirs)) & 3) == 0,
              "reverb_pairs: clean_src, noisy_src, recs, bank, rirs_host and rirs must be 4-byte aligned");
  CUM_REQUIRE(n_rirs >= 1 && bank_floats >= 1, "reverb_pairs: n_rirs and bank_floats must be at least 1");
  for (int32_t r = 0; r < n_rirs; ++r) {
    const int32_t *e = rirs_host + 4 * (int64_t)r;
    const int64_t off = (int64_t)(((uint64_t)(uint32_t)e[1] << 32) | (uint64_t)(uint32_t)e[0]);
    CUM_REQUIRE(e[2] >= 1 && e[2] <= kRevTMax, "reverb_pairs: a response's taps must lie in [1, 16384]");
    CUM_REQUIRE(off >= 0 && (off & 3) == 0, "reverb_pairs: a response's offset must be on the 16-byte grid of the bank");
    CUM_REQUIRE(off <= bank_floats - e[2], "reverb_pairs: a response's span leaves the bank");
  }
  // the host cannot know a row's response (nothing is read here): the grids follow (batch, n) alone, capped at about
  // four workgroups per CU; a workgroup of a row without a response copies its share (apply) or leaves (the others)
  const int64_t most = cdiv64(cdiv64(n, kRevP), kRevWaves);
  const int64_t cap = 1024 / batch > 1 ? 1024 / batch : 1;
  const dim3 grid((unsigned)(most < cap ? most : cap), (unsigned)batch);
  const int filter_lds = kRevTwBytes + kRevBufBytes, wave_lds = kRevTwBytes + kRevWaves * kRevBufBytes;
  const int rc = reverb_lds_limits(filter_lds, wave_lds);
  if (rc != CUM_OK) return rc;
  hipLaunchKernelGGL(reverb_filter_kernel, dim3(kRevKMax, (unsigned)batch), dim3(kRevFilterThreads), filter_lds,
                     (hipStream_t)stream, recs, bank, bank_floats, rirs, n_rirs, workspace);
  CUM_CHECK_LAUNCH();
  hipLaunchKernelGGL(reverb_blocks_kernel, grid, dim3(64 * kRevWaves), wave_lds, (hipStream_t)stream, clean_src,
                     clean_src_sb, batch, n, recs, bank_floats, rirs, n_rirs, workspace);
  CUM_CHECK_LAUNCH();
  hipLaunchKernelGGL(reverb_apply_kernel, grid, dim3(64 * kRevWaves), wave_lds, (hipStream_t)stream, clean_src,
                     clean_src_sb, noisy_src, noisy_src_sb, batch, n, recs, bank_floats, rirs, n_rirs, workspace, clean,
                     clean_sb, noisy, noisy_sb);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}
