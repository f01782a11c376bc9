// Slot-row mover of the per-layer stream pool (cum_stream_slots_move; cleanumamba_amd/network/layerpool.py).
// The reference keeps ONE stream's state in Python attributes of the model (feed / _denoise_frame,
// src/network/CleanUMamba.py:358-490: the running std, the per-layer conv caches, the Mamba conv / SSM states).  A pool
// keeps that state per SLOT, one row of an f32 store [capacity][state_stride], and runs any subset of the slots as a dense
// batch of the per-layer hop, whose buffers hold stream j of the batch at `dense + j * pitch`.  One launch moves every
// segment of every named slot:
//   gather  (direction 0): dense[seg] + j * pitch [0, len)  =  store[slots[j]] + off [0, len)
//   scatter (direction 1): the other way round
// and a gather also clears, per dense row buffer, the two byte ranges that frame the batch's rows (its leading row and
// the slack rows behind the last stream): a smaller batch's framing rows lie where a larger batch kept stream rows.
// (A gather that names no slot only clears: a batch that shrinks keeps its leading streams in place.)
// The work is (slot, segment, 16-byte piece) units spread over the grid: 512 units per workgroup, so that one slot of a
// 2 MB row is 256 workgroups.  A segment whose store offset, dense base and dense pitch are all multiples of 16 moves as
// 16-byte vectors (its last, shorter piece as dwords); any other segment moves dword by dword (pruned models' Mamba
// states have per-stream sizes such as d_inner x 13 x 4 bytes).  Plain vector loads and stores only.
#include <vector>

#include "common.h"

namespace cum {

constexpr int kMoveThreads = 256, kMoveUnits = 512, kMoveMaxSegs = 256, kMoveSegInts = 4, kMoveClearInts = 4;

// pieces of one segment: 16-byte pieces where both sides allow vectors (the last may be short), else dwords
__host__ __device__ inline bool move_seg_vec(const int64_t *seg, bool store_vec) {
  return store_vec && ((seg[0] | seg[1] | seg[2]) & 15) == 0;
}
__host__ __device__ inline int64_t move_seg_units(const int64_t *seg, bool store_vec) {
  return move_seg_vec(seg, store_vec) ? (seg[3] + 15) / 16 : seg[3] / 4;
}

// Unit u of a slot's list: where it reads and writes, as a 16-byte piece (kind 1) or a dword (2); kind 0: nothing left to
// do (past the list, or the short last piece of a vector segment, which is moved here dword by dword).
struct MoveUnit {
  const char *src;
  char *dst;
  int kind;
};
__device__ __forceinline__ MoveUnit move_locate(int u, int total, const int32_t *first, const int64_t *sseg, int n_segs,
                                       bool store_vec, char *row, int j, int direction) {
  MoveUnit m = {nullptr, nullptr, 0};
  if (u >= total) return m;
  int lo = 0, hi = n_segs - 1;                          // the segment g with first[g] <= u < first[g + 1]
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (first[mid] <= u) lo = mid; else hi = mid - 1;
  }
  const int64_t *seg = sseg + lo * kMoveSegInts;
  const int64_t len = seg[3];
  char *d = (char *)(uintptr_t)seg[0] + (int64_t)j * seg[1];
  char *s = row + seg[2];
  const char *src = direction == 0 ? s : d;
  char *dst = direction == 0 ? d : s;
  const int64_t p = u - first[lo];
  if (!move_seg_vec(seg, store_vec)) {
    m.src = src + p * 4, m.dst = dst + p * 4, m.kind = 2;
  } else if (p * 16 + 16 <= len) {
    m.src = src + p * 16, m.dst = dst + p * 16, m.kind = 1;
  } else {
    for (int64_t q = p * 16; q < len; q += 4) *(uint32_t *)(dst + q) = *(const uint32_t *)(src + q);
  }
  return m;
}

__global__ __launch_bounds__(kMoveThreads) void stream_slots_move_kernel(int direction, char *store, int64_t stride_bytes,
                                                                         const int32_t *__restrict__ slots, int n,
                                                                         const int64_t *__restrict__ segs, int n_segs,
                                                                         const int64_t *__restrict__ clears,
                                                                         int n_clears) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.y == n) {
    // the framing rows of the dense row buffers (a gather only): grid-stride over each range, dword stores
    for (int c = 0; c < n_clears; ++c) {
      const int64_t *r = clears + (int64_t)c * kMoveClearInts;
      char *base = (char *)(uintptr_t)r[0];
      const int64_t head = r[1] / 4, tail = r[3] / 4;
      for (int64_t i = (int64_t)blockIdx.x * kMoveThreads + tid; i < head + tail; i += (int64_t)gridDim.x * kMoveThreads)
        *(float *)(i < head ? base + i * 4 : base + r[2] + (i - head) * 4) = 0.f;
    }
    return;
  }
  __shared__ int32_t first[kMoveMaxSegs + 1];          // first[g]: the first unit of segment g in a slot's unit list
  __shared__ int64_t sseg[kMoveMaxSegs * kMoveSegInts];  // the segment table (every unit looks its segment up)
  const bool store_vec = (((uintptr_t)store | (uint64_t)stride_bytes) & 15) == 0;
  for (int i = tid; i < n_segs * kMoveSegInts; i += kMoveThreads) sseg[i] = segs[i];
  __syncthreads();
  for (int g = tid; g < n_segs; g += kMoveThreads)
    first[g + 1] = (int32_t)move_seg_units(sseg + g * kMoveSegInts, store_vec);
  __syncthreads();
  if (tid == 0) {
    first[0] = 0;
    for (int g = 0; g < n_segs; ++g) first[g + 1] += first[g];
  }
  __syncthreads();
  const int total = first[n_segs];
  const int j = blockIdx.y;
  char *row = store + (int64_t)slots[j] * stride_bytes;
  // a thread's two units: both loads are issued before the first store, so that they are in flight together
  static_assert(kMoveUnits == 2 * kMoveThreads, "two units per thread");
  const int u0 = blockIdx.x * kMoveUnits + tid;
  const MoveUnit a = move_locate(u0, total, first, sseg, n_segs, store_vec, row, j, direction);
  const MoveUnit b = move_locate(u0 + kMoveThreads, total, first, sseg, n_segs, store_vec, row, j, direction);
  uint4 va = {}, vb = {};
  uint32_t wa = 0, wb = 0;
  if (a.kind == 1) va = *(const uint4 *)a.src;
  else if (a.kind == 2) wa = *(const uint32_t *)a.src;
  if (b.kind == 1) vb = *(const uint4 *)b.src;
  else if (b.kind == 2) wb = *(const uint32_t *)b.src;
  if (a.kind == 1) *(uint4 *)a.dst = va;
  else if (a.kind == 2) *(uint32_t *)a.dst = wa;
  if (b.kind == 1) *(uint4 *)b.dst = vb;
  else if (b.kind == 2) *(uint32_t *)b.dst = wb;
}

}  // namespace cum

using namespace cum;

extern "C" int cum_stream_slots_move(int32_t direction, float *store, int64_t state_stride, int32_t capacity,
                                     const int32_t *slots_host, const int32_t *slots, int32_t n,
                                     const int64_t *segs_host, const int64_t *segs, int32_t n_segs,
                                     const int64_t *clears_host, const int64_t *clears, int32_t n_clears, void *stream) {
  CUM_REQUIRE(direction == 0 || direction == 1, "stream_slots_move: direction is 0 (gather) or 1 (scatter)");
  CUM_REQUIRE(n >= 0 && n <= 65534 && capacity >= 0 && state_stride > 0 && n_segs >= 0 && n_segs <= kMoveMaxSegs &&
                  n_clears >= 0,
              "stream_slots_move: bad shape");
  const bool clear = direction == 0 && n_clears > 0;
  if (n_segs == 0 || (n == 0 && !clear)) return CUM_OK;        // (a gather of no slot only clears)
  CUM_REQUIRE(store && segs_host && segs && (n == 0 || (slots_host && slots)), "stream_slots_move: null pointer");
  CUM_REQUIRE(!clear || (clears_host && clears), "stream_slots_move: null pointer");
  CUM_REQUIRE(((uintptr_t)store & 3) == 0, "stream_slots_move: the store must be 4-byte aligned");
  std::vector<uint8_t> seen((size_t)capacity, 0);
  for (int32_t j = 0; j < n; ++j) {
    const int32_t s = slots_host[j];
    CUM_REQUIRE(s >= 0 && s < capacity, "stream_slots_move: a slot outside the pool (slot < capacity)");
    CUM_REQUIRE(!seen[s], "stream_slots_move: a slot is named twice");
    seen[s] = 1;
  }
  const int64_t row_bytes = state_stride * 4;
  const bool store_vec = (((uintptr_t)store | (uint64_t)row_bytes) & 15) == 0;
  int64_t units = 0;
  for (int32_t g = 0; g < n_segs; ++g) {
    const int64_t *r = segs_host + (int64_t)g * kMoveSegInts;
    CUM_REQUIRE(r[0] != 0, "stream_slots_move: null pointer (a segment's dense base)");
    CUM_REQUIRE(r[3] > 0 && r[3] % 4 == 0 && r[2] >= 0 && r[2] % 4 == 0 && (r[0] & 3) == 0 && r[1] % 4 == 0,
                "stream_slots_move: a segment's base, pitch, offset and length are multiples of 4 bytes, the length > 0");
    CUM_REQUIRE(r[2] + r[3] <= row_bytes, "stream_slots_move: a segment overruns the store row");
    CUM_REQUIRE(r[1] >= r[3] || n <= 1, "stream_slots_move: a segment's dense pitch is shorter than the segment");
    for (int32_t h = 0; h < g; ++h) {
      const int64_t *q = segs_host + (int64_t)h * kMoveSegInts;
      CUM_REQUIRE(r[2] + r[3] <= q[2] || q[2] + q[3] <= r[2], "stream_slots_move: segments overlap in the store row");
    }
    units += move_seg_units(r, store_vec);
  }
  CUM_REQUIRE(units < ((int64_t)1 << 31) - kMoveUnits, "stream_slots_move: a store row of 2^31 pieces or more");
  if (clear) {
    for (int32_t c = 0; c < n_clears; ++c) {
      const int64_t *r = clears_host + (int64_t)c * kMoveClearInts;
      CUM_REQUIRE(r[0] != 0, "stream_slots_move: null pointer (a row buffer to clear)");
      CUM_REQUIRE((r[0] & 3) == 0 && r[1] >= 0 && r[1] % 4 == 0 && r[2] >= r[1] && r[2] % 4 == 0 && r[3] >= 0 &&
                      r[3] % 4 == 0,
                  "stream_slots_move: a clear record {base, head bytes, tail offset, tail bytes} is not dword ranges");
    }
  }
  // (a launch that only clears needs a few workgroups: the framing rows are a handful of KB)
  const dim3 grid((unsigned)(n == 0 ? 8 : cdiv64(units, kMoveUnits)), (unsigned)(n + (clear ? 1 : 0)));
  hipLaunchKernelGGL(stream_slots_move_kernel, grid, dim3(kMoveThreads), 0, (hipStream_t)stream, (int)direction,
                     (char *)store, row_bytes, slots, (int)n, segs, (int)n_segs, clears, clear ? (int)n_clears : 0);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}
