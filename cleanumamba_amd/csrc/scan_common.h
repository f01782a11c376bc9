// Shared pieces of the selective-scan kernels (scan_fwd.hip, scan_bwd.hip).
//
// MI355X mapping (not the upstream time-parallel BlockScan design):
//   * lane  <-> channel d (64 channels per workgroup: coalesced 256-B rows in the
//     channel-contiguous layout the in_proj GEMM produces),
//   * wave  <-> slice of NS = 8 states; the NW = ceil(N/8) waves of a workgroup cover
//     all states of its 64 channels (N = 64 -> 8 waves, 512 threads),
//   * time is walked sequentially; x_t lives in VGPRs for the whole sequence,
//   * B_t / C_t are wave-uniform -> a chunk's [16][N] tiles are staged in LDS with coalesced
//     loads and read back as wave-uniform ds_read_b128 broadcasts,
//   * per 16-step chunk the workgroup computes softplus / silu once per (t, d) into
//     LDS (phase A), scans (phase B), and sums the per-wave partial results over the
//     state slices through LDS (phase C).
#pragma once
#include "common.h"

namespace cum {

constexpr int TB = 16;  // steps per chunk == checkpoint interval
constexpr int SUB = 8;  // steps whose states are held in registers in backward
constexpr int NS = 8;   // states per wave (ckpt_store / ckpt_load assume 8)

// Two states of one lane side by side: the scan arithmetic is written on pairs so that it maps onto the packed
// f32 VALU ops (v_pk_mul_f32 / v_pk_fma_f32: two results per lane per issue slot).
typedef float f2 __attribute__((ext_vector_type(2)));

struct ScanParams {
  cum_scan_shape s;
  cum_scan_grad_strides gs;
  // u, delta, z, out, dout, du, ddelta, dz hold elements of s.io_dtype (f32 or bf16); everything else is f32
  const void *u, *delta, *z;
  const float *A, *Bm, *Cm, *D, *bias;
  void *out;
  void *ypre;            // forward, optional: y before the gate (out's element type and strides), for the backward
  const void *ypre_in;   // backward, optional: the forward's ypre (dout's strides); else y is rebuilt
  float *last_state, *ckpt;
  const void *dout;
  const float *ckpt_in;
  void *du, *ddelta, *dz;
  float *ws_dA, *ws_dD, *ws_dbias, *ws_dB, *ws_dC;
  int nchunks, ngroups;
  // segmented (time-parallel) forward, scan_seg.hip: nseg segments of seg_chunks chunks; carry = its workspace
  int nseg, seg_chunks;
  float *carry;
  // forward, optional (cum_selective_scan_fwd_from): the state entering t = 0, last_state's layout; NULL = zero
  const float *init_state;
};

// The entering state of the wave's slice [n0, n0 + nvalid) of channel dc (a valid channel for every lane) into the
// registers the recurrence walks, where the kernels set x = 0.  Padding states stay 0.  Called only by the ENTER
// instantiations of the forward kernels (launched when init_state is given): the ones the plain entries reach carry
// no trace of it -- a run-time test of the pointer cost them a register and scalar spills (profiles/scan_fwd_resources.md).
template <int NP2>
__device__ __forceinline__ void scan_enter(const ScanParams &p, int b, int dc, int n0, int nvalid, f2 (&x)[NP2]) {
  const float *is = p.init_state + ((int64_t)b * p.s.dim + dc) * p.s.dstate + n0;
#pragma unroll
  for (int j = 0; j < 2 * NP2; ++j)
    if (j < nvalid) x[j / 2][j % 2] = is[j];
}

// Checkpoint buffer, d_state <= 16 (one or two waves per workgroup): the NS states a lane (channel d) of wave w holds,
// entering half h of chunk c of clip b, as 32 contiguous bytes -- [(b, c, h, w, d)][NS]: two 16-byte accesses per lane,
// 2 KB contiguous per wave.
__device__ __forceinline__ int64_t ckpt_slot(int b, int nchunks, int c, int h, int NW, int w, int Dm, int d) {
  return (((((int64_t)b * nchunks + c) * 2 + h) * NW + w) * Dm + d) * NS;
}
__device__ __forceinline__ void ckpt_store(float *ck, int64_t slot, const f2 (&x)[NS / 2]) {
  float4 *q = reinterpret_cast<float4 *>(ck + slot);
  q[0] = make_float4(x[0].x, x[0].y, x[1].x, x[1].y);
  q[1] = make_float4(x[2].x, x[2].y, x[3].x, x[3].y);
}
__device__ __forceinline__ void ckpt_load(const float *ck, int64_t slot, f2 (&x)[NS / 2]) {
  const float4 *q = reinterpret_cast<const float4 *>(ck + slot);
  const float4 a = q[0], c = q[1];
  x[0] = f2{a.x, a.y}; x[1] = f2{a.z, a.w}; x[2] = f2{c.x, c.y}; x[3] = f2{c.z, c.w};
}

// Checkpoint buffer, d_state > 16 (NW >= 3 waves per workgroup; written by scan_fwd_lds_kernel / scan_seg_kernel,
// read by scan_bwd_kernel): per (b, c, h, w, 64-channel group g) a block of 8 x 64 floats, STATE-major --
// [state n of the wave's slice][column pi(lane)], pi(l) = (l & 7) * 8 + (l >> 3).  The backward kernel keeps state
// k ^ h(lane) in register slot k (scan_bwd.hip, "xor scatter"), h a function of lane & 7: in this layout its load of slot
// k touches 8 whole 32-byte sectors per wave (lanes with equal lane & 7 sit side by side in one row), where a lane-major
// layout made it 64 partial ones -- and the forward's 8 stores per checkpoint are 256 contiguous bytes each instead of
// two interleaved half-sector passes.  The group axis is padded to whole groups (cum_scan_ckpt_elems).
constexpr bool ckpt_is_wide(int NW) { return NW >= 3; }
__device__ __forceinline__ int ckpt_pi(int lane) { return (lane & 7) * 8 + (lane >> 3); }
__device__ __forceinline__ int64_t ckpt_wide_block(int b, int nchunks, int c, int h, int NW, int w, int Dm, int g) {
  const int G = (Dm + 63) >> 6;
  return (((((int64_t)b * nchunks + c) * 2 + h) * NW + w) * G + g) * (64 * NS);
}
__device__ __forceinline__ float ckpt_elem(const f2 (&x)[NS / 2], int n) { return x[n / 2][n % 2]; }
// the state a lane holds in natural order (x[n] = state n of the wave's slice) -> the layout its NW asks for
template <int NW, typename X>
__device__ __forceinline__ void ckpt_put(float *ck, int b, int nchunks, int c, int h, int w, int Dm, int d, const X &x) {
  if constexpr (ckpt_is_wide(NW)) {
    float *q = ck + ckpt_wide_block(b, nchunks, c, h, NW, w, Dm, d >> 6) + ckpt_pi(d & 63);
#pragma unroll
    for (int n = 0; n < NS; ++n) q[n * 64] = ckpt_elem(x, n);
  } else {
    ckpt_store(ck, ckpt_slot(b, nchunks, c, h, NW, w, Dm, d), x);
  }
}

// carry buffer of the time-parallel forms (scan_seg.hip forward, scan_bwd_small.hip backward): [(b, seg, w, d)][NS] f32
// (a segment's end state / leaving dx carry from a zero start), then the per-segment sums of delta' [(b, seg, d)]
__device__ __forceinline__ int64_t carry_slot(int b, int nseg, int seg, int NW, int w, int Dm, int d) {
  return ((((int64_t)b * nseg + seg) * NW + w) * Dm + d) * NS;
}

// cum_scan_shape::delta_softplus is a flag word: bit 0 = softplus on delta + bias; bit 1 (CUM_SCAN_A_IS_LOG) = the `A`
// argument holds A_log and the op uses A = -exp(A_log) (upstream Mamba.forward's `A = -torch.exp(self.A_log.float())`,
// src/network/S4/MambaS4.py mirror); the backward then returns dA_log = dA * A.  One expf per (channel, state) at kernel
// start instead of two elementwise launches per block and step (and a third in the backward).
constexpr int kScanSoftplus = 1, kScanAIsLog = 2;
__device__ __forceinline__ float scan_A(const ScanParams &p, int64_t idx) {
  const float a = p.A[idx];
  return (p.s.delta_softplus & kScanAIsLog) ? -expf(a) : a;
}

int scan_check_shape(const cum_scan_shape *s);
// segment plan of the time-parallel backward (d_state <= 16 only: scan_bwd_small.hip)
void scan_seg_plan_bwd(int batch, int dim, int dstate, int len, int *nseg, int *seg_chunks);
// time-parallel forward for grids that do not fill the chip (scan_seg.hip): plan (nseg == 1: sequential kernels),
// workspace size in f32 elements, launcher
void scan_seg_plan(int batch, int dim, int dstate, int len, int *nseg, int *seg_chunks);
int64_t scan_seg_carry_elems(int batch, int dim, int dstate, int nseg);
int launch_fwd_segmented(const ScanParams &p, hipStream_t st);
// d_state <= 16: wave-specialised backward (scan_bwd_small.hip); the caller runs scan_bwd_finalize_kernel afterwards
int launch_bwd_small(const ScanParams &p, hipStream_t st);

}  // namespace cum
