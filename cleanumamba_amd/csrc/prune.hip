// Structured channel pruning on the device, for gfx950 (cleanumamba_amd/pruning/).
//
//   cum_prune_importance  <- PruningModule.channel_importances of the reference (src/pruning/pruninggroup.py:160-226),
//                            for every (group, module, channel) of a host-compiled table in ONE launch: the five sums
//                            sum w^2, sum g^2, sum |w g|, sum (w g)^2 and |sum w g| over a channel's elements, read in place
//                            through strided descriptors (no transposes, no copies), g divided by the device-side loss
//                            scale.  Every channel is reduced by one wave in a fixed order, in f64: no atomics, bitwise
//                            reproducible.
//   cum_prune_gather      <- the per-tensor index_select of prune_parameter_and_grad (src/pruning/util.py:328-349) for a
//                            model whose parameters, gradients and Adam moments live in four flat buffers
//                            (training/flat_optim.py): one launch moves the kept elements of every parameter from the old
//                            layout into the new one, in all four buffers, bit-exact.  Kept indices come as one list per
//                            dimension of a parameter, not as a per-element table.
//   cum_prune_mask        <- the trial prune of the reference's layer-wise calibration
//                            (src/pruning/layerwise_calibration.py:120-135: deepcopy + group.prune + forward) done in
//                            place: the elements a prune would remove are saved to a compact buffer and zeroed, and
//                            written back bit-exact after the trial forward.  Selected rows come as a device list of
//                            indices per descriptor, so any channel set works.
// All are memory-bound.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "common.h"

namespace cum {

constexpr int kImpWaves = 4;        // waves (work items) per workgroup of the importance kernel
constexpr int kGatherThreads = 256;
constexpr int kGatherQuads = 4;     // 4-element quads per thread: 4096 elements per workgroup

struct ImpItem {
  int32_t desc, c0;                 // descriptor, first channel (lanes_on_channels: 64 channels from c0; else channel c0)
};

__device__ __forceinline__ void imp_add(double w, double g, double (&s)[5]) {
  const double wg = w * g;
  s[0] = fma(w, w, s[0]);
  s[1] = fma(g, g, s[1]);
  s[2] += fabs(wg);
  s[3] = fma(wg, wg, s[3]);
  s[4] += wg;
}

__global__ __launch_bounds__(64 * kImpWaves) void prune_importance_kernel(const cum_prune_imp_desc *__restrict__ descs,
                                                                          const ImpItem *__restrict__ items, int32_t n_items,
                                                                          const float *__restrict__ scale,
                                                                          float *__restrict__ out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int it = blockIdx.x * kImpWaves + wave;
  if (it >= n_items) return;
  const ImpItem item = items[it];
  const cum_prune_imp_desc d = descs[item.desc];
  const double inv_scale = scale ? 1.0 / (double)scale[0] : 1.0;
  const int32_t inner = d.n0 * d.n1;
  const int32_t count = d.heads * inner;
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (d.lanes_on_channels) {
    // lane = channel: neighbouring lanes read neighbouring columns (dim-1 modules, tiny rows); each lane walks its
    // channel's elements in index order
    const int c = item.c0 + lane;
    if (c < d.channels) {
      const int64_t base = d.off + (int64_t)c * d.ch_stride;
      for (int h = 0; h < d.heads; ++h)
        for (int i0 = 0; i0 < d.n0; ++i0)
          for (int i1 = 0; i1 < d.n1; ++i1) {
            const int64_t a = base + (int64_t)h * d.head_stride + (int64_t)i0 * d.s0 + (int64_t)i1 * d.s1;
            const double w = (double)d.w[a];
            const double g = d.g ? (double)d.g[a] * inv_scale : 0.0;
            imp_add(w, g, s);
          }
      float *o = out + (d.out + c) * 5;
      o[0] = (float)s[0];
      o[1] = (float)s[1];
      o[2] = (float)s[2];
      o[3] = (float)s[3];
      o[4] = (float)fabs(s[4]);
    }
    return;
  }
  // one wave per channel: lanes stride over the channel's elements (contiguous rows: coalesced), then a fixed butterfly
  const int64_t base = d.off + (int64_t)item.c0 * d.ch_stride;
  for (int32_t j = lane; j < count; j += 64) {
    const int32_t h = j / inner, r = j - h * inner;
    const int32_t i0 = r / d.n1, i1 = r - i0 * d.n1;
    const int64_t a = base + (int64_t)h * d.head_stride + (int64_t)i0 * d.s0 + (int64_t)i1 * d.s1;
    const double w = (double)d.w[a];
    const double g = d.g ? (double)d.g[a] * inv_scale : 0.0;
    imp_add(w, g, s);
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s[k] += __shfl_xor(s[k], o, 64);
  }
  if (lane == 0) {
    float *o = out + (d.out + item.c0) * 5;
    o[0] = (float)s[0];
    o[1] = (float)s[1];
    o[2] = (float)s[2];
    o[3] = (float)s[3];
    o[4] = (float)fabs(s[4]);
  }
}

struct GatherArgs {
  const cum_prune_gather_desc *descs;
  const int64_t *block_start;       // n_desc + 1 prefix sums of the workgroups per descriptor
  const int32_t *keep;
  int32_t n_desc;
  const float *src[4];
  float *dst[4];
};

// element e of the NEW (pruned) parameter, row-major over new_dims -> its element in the old parameter
__device__ __forceinline__ int64_t gather_src_index(const cum_prune_gather_desc &d, const int32_t *__restrict__ keep,
                                                    int32_t e) {
  // (fixed trip counts: the index array stays in registers)
  int32_t idx[3] = {0, 0, 0};
  int32_t rest = e;
#pragma unroll
  for (int k = 2; k >= 0; --k) {
    if (k < d.ndim) {
      const int32_t q = rest / d.new_dims[k];
      idx[k] = rest - q * d.new_dims[k];
      rest = q;
    }
  }
  int64_t src = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (k < d.ndim) {
      const int32_t i = d.keep[k] >= 0 ? keep[d.keep[k] + idx[k]] : idx[k];
      src = src * d.old_dims[k] + i;
    }
  }
  return src;
}

// NB buffers (2: parameters + gradients; 4: + both Adam moments).  Three paths per parameter, chosen per workgroup:
//   rows  innermost dimension kept whole, its extent a multiple of 4, source 16-byte aligned: every aligned quad of the
//         new parameter is an aligned quad of one kept row -> one index computation and one float4 load / store per
//         buffer per quad (conv weights, the pruned rows of the projections, every parameter nothing was removed from);
//   flat  nothing removed, extents not a multiple of 4: float4 over the whole quads, the last quad scalar (+ padding);
//   any   the innermost dimension loses elements: one element per lane, consecutive lanes on consecutive new elements
//         (coalesced stores, loads along the kept runs).
// Positions from n_new up to the next multiple of 4 are the parameter's alignment padding and are written as zeros.
template <int NB>
__global__ __launch_bounds__(kGatherThreads) void prune_gather_kernel(const GatherArgs a) {
  int lo = 0, hi = a.n_desc - 1;
  const int64_t b = blockIdx.x;
  while (lo < hi) {                   // the descriptor of this workgroup (a few hundred parameters at most)
    const int mid = (lo + hi + 1) >> 1;
    if (a.block_start[mid] <= b) lo = mid;
    else hi = mid - 1;
  }
  const cum_prune_gather_desc d = a.descs[lo];
  const int last = d.ndim - 1;
  const bool identity = d.keep[0] < 0 && d.keep[1] < 0 && d.keep[2] < 0;
  const bool rows = d.keep[last] < 0 && (d.new_dims[last] & 3) == 0 && (d.src & 3) == 0;
  const int64_t first = (b - a.block_start[lo]) * (int64_t)(kGatherThreads * kGatherQuads * 4);
  const int64_t span = (d.n_new + 3) & ~(int64_t)3;
  if (rows || (identity && (d.src & 3) == 0)) {
    // every quad's loads are issued before any store (the buffers are not declared disjoint to the compiler: a store
    // would otherwise fence the next quad's loads), kGatherQuads x NB float4 in flight per thread
    float4 v[kGatherQuads][NB];
#pragma unroll
    for (int q = 0; q < kGatherQuads; ++q) {
      const int64_t e0 = first + ((int64_t)q * kGatherThreads + threadIdx.x) * 4;
      if (e0 + 4 <= d.n_new) {
        const int64_t s = d.src + (identity ? e0 : gather_src_index(d, a.keep, (int32_t)e0));
#pragma unroll
        for (int t = 0; t < NB; ++t) v[q][t] = *reinterpret_cast<const float4 *>(a.src[t] + s);
      } else if (e0 < span) {         // (identity only) the last, partial quad
        float x[NB][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
          for (int t = 0; t < NB; ++t) x[t][k] = e0 + k < d.n_new ? a.src[t][d.src + e0 + k] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < NB; ++t) v[q][t] = make_float4(x[t][0], x[t][1], x[t][2], x[t][3]);
      }
    }
#pragma unroll
    for (int q = 0; q < kGatherQuads; ++q) {
      const int64_t e0 = first + ((int64_t)q * kGatherThreads + threadIdx.x) * 4;
      if (e0 < span) {
#pragma unroll
        for (int t = 0; t < NB; ++t) *reinterpret_cast<float4 *>(a.dst[t] + d.dst + e0) = v[q][t];
      }
    }
    return;
  }
#pragma unroll 4
  for (int j = 0; j < kGatherQuads * 4; ++j) {
    const int64_t e = first + (int64_t)j * kGatherThreads + threadIdx.x;
    if (e >= span) break;
    if (e < d.n_new) {
      const int64_t s = d.src + (identity ? e : gather_src_index(d, a.keep, (int32_t)e));
#pragma unroll
      for (int t = 0; t < NB; ++t) a.dst[t][d.dst + e] = a.src[t][s];
    } else {
#pragma unroll
      for (int t = 0; t < NB; ++t) a.dst[t][d.dst + e] = 0.f;
    }
  }
}

constexpr int kMaskThreads = 256;
constexpr int kMaskPer = 4;         // elements per thread: 1024 per workgroup

struct MaskArgs {
  const cum_prune_mask_desc *descs;
  const int64_t *block_start;       // n_desc + 1 prefix sums of the workgroups per descriptor
  const int64_t *save_start;        // n_desc prefix sums of the saved elements per descriptor
  const int32_t *idx;
  int32_t n_desc;
  float *save;
  int32_t restore;
};

// Element e of descriptor d (row j of its list, element (i0, i1) of that row; rows_fastest: consecutive e on
// consecutive selected rows, for column selections) -> its offset in d.w.  save[save_start + e] holds its value.
__global__ __launch_bounds__(kMaskThreads) void prune_mask_kernel(const MaskArgs a) {
  int lo = 0, hi = a.n_desc - 1;
  const int64_t b = blockIdx.x;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.block_start[mid] <= b) lo = mid;
    else hi = mid - 1;
  }
  const cum_prune_mask_desc d = a.descs[lo];
  const int64_t inner = (int64_t)d.n0 * d.n1;
  const int64_t count = (int64_t)d.n_rows * inner;
  const int64_t first = (b - a.block_start[lo]) * (int64_t)(kMaskThreads * kMaskPer);
  float *__restrict__ save = a.save + a.save_start[lo];
  const int32_t *__restrict__ rows = a.idx + d.first;
#pragma unroll
  for (int k = 0; k < kMaskPer; ++k) {
    const int64_t e = first + (int64_t)k * kMaskThreads + threadIdx.x;
    if (e >= count) break;
    int64_t j, r;
    if (d.rows_fastest) {
      r = e / d.n_rows;
      j = e - r * d.n_rows;
    } else {
      j = e / inner;
      r = e - j * inner;
    }
    const int64_t i0 = r / d.n1, i1 = r - i0 * d.n1;
    const int64_t off = (int64_t)rows[j] * d.row_stride + i0 * d.s0 + i1 * d.s1;
    if (a.restore) {
      d.w[off] = save[e];
    } else {
      save[e] = d.w[off];
      d.w[off] = 0.f;
    }
  }
}

}  // namespace cum

using namespace cum;

// ---- host side
static char g_prune_msg[256];

static int prune_fail(const char *fmt, long long a, long long b = 0) {
  snprintf(g_prune_msg, sizeof g_prune_msg, fmt, a, b);
  cum_set_error(g_prune_msg);
  return CUM_EINVAL;
}

// The tables go to the workspace from host memory the entry owns; the upload is waited for before the entry returns.
static int prune_upload(const char *who, void *dst, const void *src, size_t bytes, hipStream_t st) {
  if (bytes == 0) return CUM_OK;
  if (hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
    snprintf(g_prune_msg, sizeof g_prune_msg, "%s: table upload failed", who);
    cum_set_error(g_prune_msg);
    return CUM_ELAUNCH;
  }
  return CUM_OK;
}

static int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

static int64_t imp_items(const cum_prune_imp_desc &d) {
  return d.lanes_on_channels ? (d.channels + 63) / 64 : d.channels;
}

extern "C" int64_t cum_prune_importance_workspace_bytes(const cum_prune_imp_desc *descs, int32_t n_desc) {
  if (!descs || n_desc <= 0) return -1;
  int64_t items = 0;
  for (int32_t i = 0; i < n_desc; ++i) items += imp_items(descs[i]);
  return align256((int64_t)n_desc * (int64_t)sizeof(cum_prune_imp_desc)) + align256(items * (int64_t)sizeof(ImpItem));
}

extern "C" int cum_prune_importance(const cum_prune_imp_desc *descs, int32_t n_desc, const float *scale, float *out,
                                    int64_t n_out, void *workspace, int64_t workspace_bytes, void *stream) {
  CUM_REQUIRE(descs && n_desc > 0, "prune_importance: empty descriptor table");
  CUM_REQUIRE(out && n_out > 0, "prune_importance: null or empty output");
  int64_t items = 0;
  for (int32_t i = 0; i < n_desc; ++i) {
    const cum_prune_imp_desc &d = descs[i];
    if (!d.w) return prune_fail("prune_importance: descriptor %lld has a null parameter pointer", i);
    if (d.channels <= 0 || d.heads <= 0 || d.n0 <= 0 || d.n1 <= 0)
      return prune_fail("prune_importance: descriptor %lld has an empty extent", i);
    if ((int64_t)d.heads * d.n0 * d.n1 > INT32_MAX)
      return prune_fail("prune_importance: descriptor %lld has more than 2^31 elements per channel", i);
    if (d.off < 0 || d.ch_stride < 0 || d.head_stride < 0 || d.s0 < 0 || d.s1 < 0)
      return prune_fail("prune_importance: descriptor %lld has a negative offset or stride", i);
    const int64_t last = d.off + (int64_t)(d.channels - 1) * d.ch_stride + (int64_t)(d.heads - 1) * d.head_stride +
                         (int64_t)(d.n0 - 1) * d.s0 + (int64_t)(d.n1 - 1) * d.s1;
    if (last >= d.numel) return prune_fail("prune_importance: descriptor %lld reads past its tensor (element %lld)", i, last);
    if (d.out < 0 || d.out + d.channels > n_out)
      return prune_fail("prune_importance: descriptor %lld writes past the output (%lld rows)", i, n_out);
    items += imp_items(d);
  }
  CUM_REQUIRE(items <= INT32_MAX / 2, "prune_importance: too many channels");
  CUM_REQUIRE(workspace && workspace_bytes >= cum_prune_importance_workspace_bytes(descs, n_desc),
              "prune_importance: workspace too small");
  std::vector<ImpItem> table;
  table.reserve(items);
  for (int32_t i = 0; i < n_desc; ++i) {
    const int step = descs[i].lanes_on_channels ? 64 : 1;
    for (int32_t c = 0; c < descs[i].channels; c += step) table.push_back(ImpItem{i, c});
  }
  char *ws = (char *)workspace;
  const int64_t dbytes = align256((int64_t)n_desc * (int64_t)sizeof(cum_prune_imp_desc));
  hipStream_t st = (hipStream_t)stream;
  int rc = prune_upload("prune_importance", ws, descs, (size_t)n_desc * sizeof(cum_prune_imp_desc), st);
  if (rc == CUM_OK) rc = prune_upload("prune_importance", ws + dbytes, table.data(), table.size() * sizeof(ImpItem), st);
  if (rc != CUM_OK) return rc;
  const int64_t blocks = cdiv64(items, kImpWaves);
  hipLaunchKernelGGL(prune_importance_kernel, dim3((unsigned)blocks), dim3(64 * kImpWaves), 0, st,
                     (const cum_prune_imp_desc *)ws, (const ImpItem *)(ws + dbytes), (int32_t)items, scale, out);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}

static int64_t gather_blocks(const cum_prune_gather_desc &d) {
  return cdiv64(d.n_new, kGatherThreads * kGatherQuads * 4);
}

extern "C" int64_t cum_prune_gather_workspace_bytes(int32_t n_desc, int64_t n_keep) {
  if (n_desc <= 0 || n_keep < 0) return -1;
  return align256((int64_t)n_desc * (int64_t)sizeof(cum_prune_gather_desc)) + align256((int64_t)(n_desc + 1) * 8) +
         align256(n_keep * 4);
}

extern "C" int cum_prune_gather(const cum_prune_gather_desc *descs, int32_t n_desc, const int32_t *keep, int64_t n_keep,
                                const float *src_p, const float *src_g, const float *src_m, const float *src_v,
                                int64_t src_numel, float *dst_p, float *dst_g, float *dst_m, float *dst_v,
                                int64_t dst_numel, void *workspace, int64_t workspace_bytes, void *stream) {
  CUM_REQUIRE(descs && n_desc > 0, "prune_gather: empty descriptor table");
  CUM_REQUIRE(n_keep >= 0 && (n_keep == 0 || keep), "prune_gather: null keep lists");
  CUM_REQUIRE(src_p && src_g && dst_p && dst_g, "prune_gather: null parameter or gradient buffer");
  const bool moments = src_m || src_v || dst_m || dst_v;
  CUM_REQUIRE(!moments || (src_m && src_v && dst_m && dst_v), "prune_gather: the four moment pointers go together");
  CUM_REQUIRE(((uintptr_t)src_p | (uintptr_t)src_g | (uintptr_t)src_m | (uintptr_t)src_v | (uintptr_t)dst_p |
               (uintptr_t)dst_g | (uintptr_t)dst_m | (uintptr_t)dst_v) % 16 == 0,
              "prune_gather: buffers must be 16-byte aligned");
  CUM_REQUIRE(src_numel >= 0 && dst_numel >= 0, "prune_gather: bad buffer size");
  std::vector<int64_t> start(n_desc + 1, 0);
  int64_t prev_end = 0;
  for (int32_t i = 0; i < n_desc; ++i) {
    const cum_prune_gather_desc &d = descs[i];
    if (d.ndim < 1 || d.ndim > 3) return prune_fail("prune_gather: descriptor %lld: ndim must be 1..3", i);
    int64_t n_old = 1, n_new = 1;
    for (int k = 0; k < 3; ++k) {
      const bool used = k < d.ndim;
      const int32_t od = used ? d.old_dims[k] : 1, nd = used ? d.new_dims[k] : 1;
      if (od <= 0 || nd <= 0 || nd > od) return prune_fail("prune_gather: descriptor %lld dimension %lld: bad extent", i, k);
      if (!used && d.keep[k] >= 0) return prune_fail("prune_gather: descriptor %lld: keep list on unused dimension %lld", i, k);
      if (d.keep[k] < 0) {
        if (nd != od) return prune_fail("prune_gather: descriptor %lld dimension %lld shrinks without a keep list", i, k);
      } else {
        if (d.keep[k] + nd > n_keep) return prune_fail("prune_gather: descriptor %lld dimension %lld: keep list out of range", i, k);
        const int32_t *kl = keep + d.keep[k];
        for (int32_t j = 0; j < nd; ++j)
          if (kl[j] < 0 || kl[j] >= od || (j > 0 && kl[j] <= kl[j - 1]))
            return prune_fail("prune_gather: descriptor %lld dimension %lld: keep list not increasing within the old extent", i, k);
      }
      n_old *= od;
      n_new *= nd;
    }
    if (n_old > INT32_MAX) return prune_fail("prune_gather: descriptor %lld: more than 2^31 elements", i);
    if (d.n_new != n_new) return prune_fail("prune_gather: descriptor %lld: n_new %lld is not the product of new_dims", i, d.n_new);
    const int64_t span = (n_new + 3) & ~(int64_t)3;                  // the new slot, alignment padding included
    if (d.src < 0 || d.src + n_old > src_numel) return prune_fail("prune_gather: descriptor %lld reads past the old buffers", i);
    if ((d.dst & 3) != 0) return prune_fail("prune_gather: descriptor %lld: destination not 16-byte aligned", i);
    if (d.dst < prev_end || d.dst + span > dst_numel)
      return prune_fail("prune_gather: descriptor %lld: destination overlaps its predecessor or leaves the new buffers", i);
    prev_end = d.dst + span;
    start[i + 1] = start[i] + gather_blocks(d);
  }
  CUM_REQUIRE(start[n_desc] > 0 && start[n_desc] < INT32_MAX, "prune_gather: bad total size");
  CUM_REQUIRE(workspace && workspace_bytes >= cum_prune_gather_workspace_bytes(n_desc, n_keep),
              "prune_gather: workspace too small");
  char *ws = (char *)workspace;
  const int64_t dbytes = align256((int64_t)n_desc * (int64_t)sizeof(cum_prune_gather_desc));
  const int64_t sbytes = align256((int64_t)(n_desc + 1) * 8);
  hipStream_t st = (hipStream_t)stream;
  int rc = prune_upload("prune_gather", ws, descs, (size_t)n_desc * sizeof(cum_prune_gather_desc), st);
  if (rc == CUM_OK) rc = prune_upload("prune_gather", ws + dbytes, start.data(), (size_t)(n_desc + 1) * 8, st);
  if (rc == CUM_OK) rc = prune_upload("prune_gather", ws + dbytes + sbytes, keep, (size_t)n_keep * 4, st);
  if (rc != CUM_OK) return rc;
  GatherArgs a{(const cum_prune_gather_desc *)ws, (const int64_t *)(ws + dbytes), (const int32_t *)(ws + dbytes + sbytes),
               n_desc, {src_p, src_g, src_m, src_v}, {dst_p, dst_g, dst_m, dst_v}};
  if (moments)
    hipLaunchKernelGGL(prune_gather_kernel<4>, dim3((unsigned)start[n_desc]), dim3(kGatherThreads), 0, st, a);
  else
    hipLaunchKernelGGL(prune_gather_kernel<2>, dim3((unsigned)start[n_desc]), dim3(kGatherThreads), 0, st, a);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}

static int64_t mask_count(const cum_prune_mask_desc &d) { return (int64_t)d.n_rows * d.n0 * d.n1; }

extern "C" int64_t cum_prune_mask_save_elems(const cum_prune_mask_desc *descs, int32_t n_desc) {
  if (!descs || n_desc <= 0) return -1;
  int64_t n = 0;
  for (int32_t i = 0; i < n_desc; ++i) {
    if (descs[i].n_rows < 0 || descs[i].n0 <= 0 || descs[i].n1 <= 0) return -1;
    n += mask_count(descs[i]);
  }
  return n;
}

extern "C" int64_t cum_prune_mask_workspace_bytes(int32_t n_desc, int64_t n_idx) {
  if (n_desc <= 0 || n_idx < 0) return -1;
  return align256((int64_t)n_desc * (int64_t)sizeof(cum_prune_mask_desc)) + 2 * align256((int64_t)(n_desc + 1) * 8) +
         align256(n_idx * 4);
}

extern "C" int cum_prune_mask(const cum_prune_mask_desc *descs, int32_t n_desc, const int32_t *idx, int64_t n_idx,
                              float *save, int64_t n_save, int32_t restore, void *workspace, int64_t workspace_bytes,
                              void *stream) {
  CUM_REQUIRE(descs && n_desc > 0, "prune_mask: empty descriptor table");
  CUM_REQUIRE(n_idx >= 0 && (n_idx == 0 || idx), "prune_mask: null index list");
  CUM_REQUIRE(restore == 0 || restore == 1, "prune_mask: restore must be 0 or 1");
  std::vector<int64_t> start(n_desc + 1, 0), save_start(n_desc + 1, 0);
  std::vector<std::pair<uintptr_t, uintptr_t>> spans;
  for (int32_t i = 0; i < n_desc; ++i) {
    const cum_prune_mask_desc &d = descs[i];
    if (!d.w) return prune_fail("prune_mask: descriptor %lld has a null tensor pointer", i);
    if (d.n0 <= 0 || d.n1 <= 0 || d.rows <= 0 || d.n_rows < 0)
      return prune_fail("prune_mask: descriptor %lld has an empty or negative extent", i);
    if (d.numel <= 0 || d.row_stride < 0 || d.s0 < 0 || d.s1 < 0)
      return prune_fail("prune_mask: descriptor %lld has a bad size or a negative stride", i);
    const int64_t last = (int64_t)(d.rows - 1) * d.row_stride + (int64_t)(d.n0 - 1) * d.s0 + (int64_t)(d.n1 - 1) * d.s1;
    if (last >= d.numel) return prune_fail("prune_mask: descriptor %lld reaches past its tensor (element %lld)", i, last);
    if (d.first < 0 || d.first + d.n_rows > n_idx)
      return prune_fail("prune_mask: descriptor %lld: row list outside the index list (%lld indices)", i, n_idx);
    for (int32_t j = 0; j < d.n_rows; ++j) {
      const int32_t r = idx[d.first + j];
      if (r < 0 || r >= d.rows || (j > 0 && r <= idx[d.first + j - 1]))
        return prune_fail("prune_mask: descriptor %lld: row list not increasing within [0, rows) at position %lld", i, j);
    }
    spans.emplace_back((uintptr_t)d.w, (uintptr_t)(d.w + d.numel));
    save_start[i + 1] = save_start[i] + mask_count(d);
    start[i + 1] = start[i] + cdiv64(mask_count(d), kMaskThreads * kMaskPer);
  }
  // a saved value must be the original one: no element may belong to two descriptors
  std::sort(spans.begin(), spans.end());
  for (size_t i = 1; i < spans.size(); ++i)
    if (spans[i].first < spans[i - 1].second)
      return prune_fail("prune_mask: two descriptors cover overlapping memory (%lld tensors)", (long long)spans.size());
  CUM_REQUIRE(save_start[n_desc] <= n_save, "prune_mask: save buffer too small");
  CUM_REQUIRE(start[n_desc] < INT32_MAX, "prune_mask: too many elements");
  if (start[n_desc] == 0) return CUM_OK;           // nothing selected
  CUM_REQUIRE(save, "prune_mask: null save buffer");
  CUM_REQUIRE(workspace && workspace_bytes >= cum_prune_mask_workspace_bytes(n_desc, n_idx),
              "prune_mask: workspace too small");
  char *ws = (char *)workspace;
  const int64_t dbytes = align256((int64_t)n_desc * (int64_t)sizeof(cum_prune_mask_desc));
  const int64_t sbytes = align256((int64_t)(n_desc + 1) * 8);
  hipStream_t st = (hipStream_t)stream;
  int rc = prune_upload("prune_mask", ws, descs, (size_t)n_desc * sizeof(cum_prune_mask_desc), st);
  if (rc == CUM_OK) rc = prune_upload("prune_mask", ws + dbytes, start.data(), (size_t)(n_desc + 1) * 8, st);
  if (rc == CUM_OK) rc = prune_upload("prune_mask", ws + dbytes + sbytes, save_start.data(), (size_t)(n_desc + 1) * 8, st);
  if (rc == CUM_OK) rc = prune_upload("prune_mask", ws + dbytes + 2 * sbytes, idx, (size_t)n_idx * 4, st);
  if (rc != CUM_OK) return rc;
  MaskArgs a{(const cum_prune_mask_desc *)ws, (const int64_t *)(ws + dbytes), (const int64_t *)(ws + dbytes + sbytes),
             (const int32_t *)(ws + dbytes + 2 * sbytes), n_desc, save, restore};
  hipLaunchKernelGGL(prune_mask_kernel, dim3((unsigned)start[n_desc]), dim3(kMaskThreads), 0, st, a);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}
