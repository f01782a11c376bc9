// Input end of the train step for gfx950: the float batch assembled on the device from staged int16 PCM.
//
//   cum_pcm_batch_f32   <- CleanNoisyPairDataset.__getitem__'s int16 -> float scaling and its tiling of a clip shorter
//                          than the crop (src/util/dataset.py:108-150), and the two host-to-device batch copies of the
//                          train loop (src/training/train.py:259-260), which become one int16 upload per batch
//
// The kernel moves 2 bytes in and 4 bytes out per sample and does nothing else, so its only job is to keep every global
// access a row-contiguous 16 bytes: a row that fills the crop (n == len) reads eight samples per lane with one 16-byte
// load and writes them with two 16-byte stores; a tiled row (n < len), or an output row that does not start on a
// 16-byte boundary, takes the element path, which walks t mod n without a division per sample.
#include "common.h"

namespace cum {

constexpr int PT = 256;            // threads per workgroup
constexpr int PV = 8;              // samples per lane and sweep on the wide path (one 16-byte load)
constexpr float kPcmScale = 1.f / 32768.f;

typedef short short8 __attribute__((ext_vector_type(8)));
typedef float float4v __attribute__((ext_vector_type(4)));

// grid: (workgroups along the row, 2 * batch rows).  Row r < batch is clean clip r, row batch + b noisy clip b.
__global__ __launch_bounds__(PT) void pcm_batch_kernel(const int16_t *__restrict__ pcm, int64_t pitch,
                                                      const int32_t *__restrict__ src_len, int batch, int64_t len,
                                                      float *__restrict__ clean, int64_t clean_sb,
                                                      float *__restrict__ noisy, int64_t noisy_sb) {
  const int r = blockIdx.y;
  const int b = r < batch ? r : r - batch;
  const int16_t *__restrict__ src = pcm + (int64_t)r * pitch;
  float *__restrict__ dst = r < batch ? clean + (int64_t)b * clean_sb : noisy + (int64_t)b * noisy_sb;
  // a bad table can never index outside the row: n in [1, len], and len <= pitch was checked on the host
  int64_t n = src_len[b];
  n = n < 1 ? 1 : (n > len ? len : n);
  const int64_t tid = (int64_t)blockIdx.x * PT + threadIdx.x, nthreads = (int64_t)gridDim.x * PT;

  if (n == len && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {          // wave-uniform: whole rows take one path
    const int64_t nvec = len / PV;
    for (int64_t v = tid; v < nvec; v += nthreads) {
      const short8 s = *reinterpret_cast<const short8 *>(src + v * PV);    // row start and v * 8 are 16-byte multiples
      float4v lo = {(float)s[0], (float)s[1], (float)s[2], (float)s[3]};
      float4v hi = {(float)s[4], (float)s[5], (float)s[6], (float)s[7]};
      float4v *o = reinterpret_cast<float4v *>(dst + v * PV);
      o[0] = lo * kPcmScale;
      o[1] = hi * kPcmScale;
    }
    for (int64_t t = nvec * PV + tid; t < len; t += nthreads) dst[t] = (float)src[t] * kPcmScale;
    return;
  }
  // element path: t mod n carried along the grid-stride loop (one division per lane, not one per sample)
  if (tid >= len) return;
  int64_t idx = tid % n;
  const int64_t step = nthreads % n;
  for (int64_t t = tid; t < len; t += nthreads) {
    dst[t] = (float)src[idx] * kPcmScale;
    idx += step;
    if (idx >= n) idx -= n;
  }
}

}  // namespace cum

using namespace cum;

extern "C" int cum_pcm_batch_f32(const int16_t *pcm, int64_t pitch, const int32_t *src_len, int32_t batch, int64_t len,
                                 float *clean, int64_t clean_sb, float *noisy, int64_t noisy_sb, void *stream) {
  CUM_REQUIRE(batch >= 1, "pcm_batch: batch must be at least 1");
  CUM_REQUIRE(batch <= 32767, "pcm_batch: batch must be at most 32767 (2 * batch rows on the grid's y axis)");
  CUM_REQUIRE(len >= 1, "pcm_batch: len must be at least 1");
  CUM_REQUIRE(pitch >= len, "pcm_batch: pitch must be at least len");
  CUM_REQUIRE(pitch % 8 == 0, "pcm_batch: pitch must be a multiple of 8 samples (16-byte rows)");
  CUM_REQUIRE(clean_sb >= len && noisy_sb >= len, "pcm_batch: clean_sb and noisy_sb must be at least len");
  CUM_REQUIRE(pcm && src_len && clean && noisy, "pcm_batch: null pointer");
  CUM_REQUIRE(((reinterpret_cast<uintptr_t>(pcm) | reinterpret_cast<uintptr_t>(clean) |
                reinterpret_cast<uintptr_t>(noisy)) & 15) == 0,
              "pcm_batch: pcm, clean and noisy must be 16-byte aligned");
  int64_t gx = cdiv64(len, (int64_t)PT * PV);
  gx = gx > 1024 ? 1024 : gx;
  hipLaunchKernelGGL(pcm_batch_kernel, dim3((unsigned)gx, (unsigned)(2 * batch)), dim3(PT), 0, (hipStream_t)stream, pcm,
                     pitch, src_len, (int)batch, len, clean, clean_sb, noisy, noisy_sb);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}
