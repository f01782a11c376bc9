// Teacher / student feature distillation loss for gfx950 (training/distill.py): the teacher branch of the
// reference's loss_fn (src/util/util.py:259-290), per layer  L = kd_p log sum (bn_s(e) - bn_t(t))^4  with both BatchNorms
// in training mode and without affine parameters.
//
// Three streaming passes over e and t, each ONE launch for all layers.  A work item is (layer, chunk of DROWS rows of the
// B * T positions); the table of layers travels in the kernel arguments, so a captured step replays it as it was.
//   stats  a lane keeps 8 neighbouring channels and walks rows: Welford (count, mean, M2) per channel of e and t, on values
//          taken relative to the chunk's first row; the lanes of a workgroup that share a channel group merge through LDS
//          in row-lane order (Chan et al.); the merge launch folds the chunks of a channel in a fixed order in f64, writes
//          the mean (as hi + lo) and rstd, and moves the running statistics.
//   loss   the same walk with s^ = (e - mean) rstd, t^, d = s^ - t^: sum d^4 per chunk, sum d^3 and sum d^3 s^ per channel
//          and chunk; the merge launch adds the chunks in f64 in a fixed order and writes D and L.  Up to the scalar 1 / D
//          the two per-channel sums are the means the BatchNorm backward needs, so the backward reduces nothing.
//   bwd    one read of e and t, one write of de = rstd_e a (d^3 - S3 / n - s^ S3s / n) in e's element type.
// No atomics anywhere.  Pad columns (c >= C) are masked by a select after the load, rows between clips are never addressed.
#include "common.h"

namespace cum {

constexpr int DT = 256;                          // threads per workgroup
constexpr int DROWS = CUM_DISTILL_ROWS;          // rows per work item
constexpr int DV = 8;                            // channels per lane
constexpr int DCB = 16;                          // channels per workgroup of the merge launches
constexpr int DSTRIPES = DT / DCB;               // chunk stripes per workgroup of the merge launches

typedef float float4d __attribute__((ext_vector_type(4)));
typedef unsigned short ushort8d __attribute__((ext_vector_type(8)));

struct DistillPlan {                             // what the launcher derives per layer
  int64_t part0;                                 // first float of the layer's per-chunk partials
  int32_t chunk0, nchunks;                       // its work items on the grids of the three passes
  int32_t cb0, ch0;                              // its first workgroup on the merge grids; its first channel in cst / csum
  int32_t e_vec, t_vec;                          // 16-byte loads are legal on that side
};

struct DistillTable {
  int32_t nl, pad_;
  cum_distill_layer L[CUM_DISTILL_MAX_LAYERS];
  DistillPlan P[CUM_DISTILL_MAX_LAYERS];
};

__device__ __forceinline__ float bf16_to_f32(unsigned short h) { return __builtin_bit_cast(float, (unsigned)h << 16); }
__device__ __forceinline__ unsigned short f32_to_bf16(float f) {          // round to nearest even, NaN kept quiet
  unsigned u = __builtin_bit_cast(unsigned, f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);
  return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ float f16_to_f32(unsigned short h) { return (float)__builtin_bit_cast(f16, h); }
__device__ __forceinline__ unsigned short f32_to_f16(float f) { return __builtin_bit_cast(unsigned short, (f16)f); }

// v[i] = row[c0 + i] for c0 + i < C, else 0 (a select: what sits in a pad column never reaches arithmetic).  `row`: first
// element of the row.  vec: the row holds 8 readable, 16-byte aligned elements at c0 whatever C is.
__device__ __forceinline__ void load8(const void *__restrict__ base, int64_t row, int dt, int vec, int c0, int C,
                                      float (&v)[DV]) {
  if (vec) {
    if (dt == CUM_F32) {
      const float4d *p = reinterpret_cast<const float4d *>(reinterpret_cast<const float *>(base) + row + c0);
      const float4d a = p[0], b = p[1];
      v[0] = a[0], v[1] = a[1], v[2] = a[2], v[3] = a[3], v[4] = b[0], v[5] = b[1], v[6] = b[2], v[7] = b[3];
    } else {
      const ushort8d h = *reinterpret_cast<const ushort8d *>(reinterpret_cast<const unsigned short *>(base) + row + c0);
#pragma unroll
      for (int i = 0; i < DV; ++i) v[i] = dt == CUM_BF16 ? bf16_to_f32(h[i]) : f16_to_f32(h[i]);
    }
#pragma unroll
    for (int i = 0; i < DV; ++i) v[i] = c0 + i < C ? v[i] : 0.f;
  } else {
#pragma unroll
    for (int i = 0; i < DV; ++i) {
      float x = 0.f;
      if (c0 + i < C) {
        if (dt == CUM_F32) {
          x = reinterpret_cast<const float *>(base)[row + c0 + i];
        } else {
          const unsigned short h = reinterpret_cast<const unsigned short *>(base)[row + c0 + i];
          x = dt == CUM_BF16 ? bf16_to_f32(h) : f16_to_f32(h);
        }
      }
      v[i] = x;
    }
  }
}

// The layer of work item `item` (chunk grids: by = 0; merge grids: by = 1) and the item's index inside it.
__device__ __forceinline__ int find_layer(const DistillTable &tab, int item, int by, int &local) {
  int li = 0;
  for (int i = 0; i < tab.nl; ++i) {
    const int first = by ? tab.P[i].cb0 : tab.P[i].chunk0;
    if (item >= first) li = i;
  }
  local = item - (by ? tab.P[li].cb0 : tab.P[li].chunk0);
  return li;
}

// How a workgroup spreads over a chunk: GW lanes across the channel groups, RS row lanes.
struct DistillLanes {
  int CG, GW, RS, g, rsub;
  bool live;
};
__device__ __forceinline__ DistillLanes distill_lanes(int C, int tid) {
  DistillLanes l;
  l.CG = (C + DV - 1) / DV;
  l.GW = l.CG < DT ? l.CG : DT;
  l.RS = DT / l.GW;
  l.g = tid % l.GW;
  l.rsub = tid / l.GW;
  l.live = l.rsub < l.RS;
  return l;
}

// rows of [r0, r1) that row lane rs of RS visits
__device__ __forceinline__ int lane_rows(int r0, int r1, int rs, int RS) {
  const int n = r1 - r0 - rs;
  return n > 0 ? (n + RS - 1) / RS : 0;
}

// ---------------------------------------------------------------------------------------------------------------- stats
constexpr int SW = 4 * DV + 1;                   // floats per lane in LDS (mean_e, M2_e, mean_t, M2_t; odd: no bank conflict)

__global__ __launch_bounds__(DT) void distill_stats_kernel(const DistillTable tab, float *__restrict__ part) {
  __shared__ float sm[DT * SW];
  const int tid = threadIdx.x;
  int ck;
  const int li = find_layer(tab, blockIdx.x, 0, ck);
  const cum_distill_layer &Ly = tab.L[li];
  const DistillPlan &Pl = tab.P[li];
  const int T = Ly.T, C = Ly.C, n = Ly.B * T;
  const int r0 = ck * DROWS, r1 = r0 + DROWS < n ? r0 + DROWS : n;
  const DistillLanes ln = distill_lanes(C, tid);
  const int Cp = ln.CG * DV;
  for (int gt = 0; gt < ln.CG; gt += ln.GW) {                     // (uniform; one trip unless C > 2048)
    const int g = gt + ln.g;
    const bool on = ln.live && g < ln.CG;
    const int c0 = g * DV;
    float me[DV], qe[DV], mt[DV], qt[DV], ke[DV], kt[DV];
#pragma unroll
    for (int i = 0; i < DV; ++i) me[i] = qe[i] = mt[i] = qt[i] = ke[i] = kt[i] = 0.f;
    if (on) {
      // every value is taken relative to the chunk's first row: features far from zero (mean 100, std 0.1) keep their
      // digits through the f32 sums, and the lanes of a channel share one origin for the merge
      load8(Ly.e, (r0 / T) * Ly.e_sb + (r0 % T) * Ly.e_st, Ly.e_dtype, Pl.e_vec, c0, C, ke);
      load8(Ly.t, (r0 / T) * Ly.t_sb + (r0 % T) * Ly.t_st, Ly.t_dtype, Pl.t_vec, c0, C, kt);
      int k = 0;
      for (int r = r0 + ln.rsub; r < r1; r += ln.RS) {
        const int b = r / T, tt = r - b * T;
        float xe[DV], xt[DV];
        load8(Ly.e, b * Ly.e_sb + tt * Ly.e_st, Ly.e_dtype, Pl.e_vec, c0, C, xe);
        load8(Ly.t, b * Ly.t_sb + tt * Ly.t_st, Ly.t_dtype, Pl.t_vec, c0, C, xt);
        ++k;
        const float inv = 1.f / (float)k;
#pragma unroll
        for (int i = 0; i < DV; ++i) {
          const float ve = xe[i] - ke[i], vt = xt[i] - kt[i];
          const float de = ve - me[i];
          me[i] += de * inv;
          qe[i] += de * (ve - me[i]);
          const float dt = vt - mt[i];
          mt[i] += dt * inv;
          qt[i] += dt * (vt - mt[i]);
        }
      }
    }
    __syncthreads();                                              // (the previous trip's readers are done)
    if (on) {
#pragma unroll
      for (int i = 0; i < DV; ++i) {
        sm[tid * SW + i] = me[i], sm[tid * SW + DV + i] = qe[i];
        sm[tid * SW + 2 * DV + i] = mt[i], sm[tid * SW + 3 * DV + i] = qt[i];
      }
    }
    __syncthreads();
    if (on && ln.rsub == 0) {
      float na = (float)lane_rows(r0, r1, 0, ln.RS);
      for (int rs = 1; rs < ln.RS; ++rs) {                        // Chan's merge, row lanes in order
        const float nb = (float)lane_rows(r0, r1, rs, ln.RS);
        if (nb == 0.f) break;
        const float *o = sm + (rs * ln.GW + ln.g) * SW;
        const float nn = na + nb, wb = nb / nn, wq = na * wb;
#pragma unroll
        for (int i = 0; i < DV; ++i) {
          const float de = o[i] - me[i];
          me[i] += de * wb;
          qe[i] += o[DV + i] + de * de * wq;
          const float dt = o[2 * DV + i] - mt[i];
          mt[i] += dt * wb;
          qt[i] += o[3 * DV + i] + dt * dt * wq;
        }
        na = nn;
      }
      float4d *dst = reinterpret_cast<float4d *>(part + Pl.part0 + ((int64_t)ck * Cp + c0) * 8);
#pragma unroll
      for (int i = 0; i < DV; ++i) {
        const float4d ve = {ke[i], me[i], qe[i], 0.f}, vt = {kt[i], mt[i], qt[i], 0.f};
        dst[2 * i] = ve, dst[2 * i + 1] = vt;
      }
    }
  }
}

// One workgroup per (layer, 16 channels): thread (channel, stripe) folds the chunks stripe, stripe + 16, ... in order, the
// stripes are folded in order by stripe 0.  f64 throughout.
__global__ __launch_bounds__(DT) void distill_stats_merge_kernel(const DistillTable tab, const float *__restrict__ part,
                                                                 float *__restrict__ cst) {
  __shared__ double sh[DSTRIPES][DCB][5];
  const int tid = threadIdx.x, cl = tid % DCB, stripe = tid / DCB;
  int cb;
  const int li = find_layer(tab, blockIdx.x, 1, cb);
  const cum_distill_layer &Ly = tab.L[li];
  const DistillPlan &Pl = tab.P[li];
  const int C = Ly.C, n = Ly.B * Ly.T, c = cb * DCB + cl;
  const int Cp = (C + DV - 1) / DV * DV;
  double na = 0.0, me = 0.0, qe = 0.0, mt = 0.0, qt = 0.0;
  if (c < C) {
    for (int k = stripe; k < Pl.nchunks; k += DSTRIPES) {
      const int rows = (k + 1) * DROWS <= n ? DROWS : n - k * DROWS;
      const float4d *src = reinterpret_cast<const float4d *>(part + Pl.part0 + ((int64_t)k * Cp + c) * 8);
      const float4d ve = src[0], vt = src[1];                     // {origin, mean - origin, M2, 0}
      const double nb = (double)rows, nn = na + nb, wb = nb / nn, wq = na * wb;
      const double de = ((double)ve[0] + (double)ve[1]) - me, dt = ((double)vt[0] + (double)vt[1]) - mt;
      me += de * wb, qe += (double)ve[2] + de * de * wq;
      mt += dt * wb, qt += (double)vt[2] + dt * dt * wq;
      na = nn;
    }
  }
  sh[stripe][cl][0] = na, sh[stripe][cl][1] = me, sh[stripe][cl][2] = qe, sh[stripe][cl][3] = mt, sh[stripe][cl][4] = qt;
  __syncthreads();
  if (stripe == 0 && c < C) {
    for (int s = 1; s < DSTRIPES; ++s) {
      const double nb = sh[s][cl][0];
      if (nb == 0.0) continue;
      const double nn = na + nb, wb = nb / nn, wq = na * wb;
      const double de = sh[s][cl][1] - me, dt = sh[s][cl][3] - mt;
      me += de * wb, qe += sh[s][cl][2] + de * de * wq;
      mt += dt * wb, qt += sh[s][cl][4] + dt * dt * wq;
      na = nn;
    }
    const double dn = (double)n, eps = (double)Ly.eps;
    // the mean as hi + lo: x - hi is exact for the values near it, and lo carries what an f32 mean would lose
    float4d oe, ot;
    oe[0] = (float)me, oe[1] = (float)(me - (double)oe[0]), oe[2] = (float)(1.0 / sqrt(qe / dn + eps)), oe[3] = 0.f;
    ot[0] = (float)mt, ot[1] = (float)(mt - (double)ot[0]), ot[2] = (float)(1.0 / sqrt(qt / dn + eps)), ot[3] = 0.f;
    reinterpret_cast<float4d *>(cst + (int64_t)(Pl.ch0 + c) * 8)[0] = oe;
    reinterpret_cast<float4d *>(cst + (int64_t)(Pl.ch0 + c) * 8)[1] = ot;
    const float m = Ly.momentum;
    if (Ly.rm_s) Ly.rm_s[c] = (1.f - m) * Ly.rm_s[c] + m * (float)me;
    if (Ly.rv_s) Ly.rv_s[c] = (1.f - m) * Ly.rv_s[c] + m * (float)(qe / (dn - 1.0));
    if (Ly.rm_t) Ly.rm_t[c] = (1.f - m) * Ly.rm_t[c] + m * (float)mt;
    if (Ly.rv_t) Ly.rv_t[c] = (1.f - m) * Ly.rv_t[c] + m * (float)(qt / (dn - 1.0));
  }
  if (cb == 0 && tid == 0) {
    if (Ly.nbt_s) *Ly.nbt_s += 1;
    if (Ly.nbt_t) *Ly.nbt_t += 1;
  }
}

// ----------------------------------------------------------------------------------------------------------------- loss
constexpr int LW = 2 * DV + 1;                   // floats per lane in LDS: sum d^3, sum d^3 s^ per channel, sum d^4

__global__ __launch_bounds__(DT) void distill_loss_kernel(const DistillTable tab, const float *__restrict__ cst,
                                                          float *__restrict__ part, float *__restrict__ s4) {
  __shared__ float sm[DT * LW];
  __shared__ float red[DT];
  const int tid = threadIdx.x;
  int ck;
  const int li = find_layer(tab, blockIdx.x, 0, ck);
  const cum_distill_layer &Ly = tab.L[li];
  const DistillPlan &Pl = tab.P[li];
  const int T = Ly.T, C = Ly.C, n = Ly.B * T;
  const int r0 = ck * DROWS, r1 = r0 + DROWS < n ? r0 + DROWS : n;
  const DistillLanes ln = distill_lanes(C, tid);
  const int Cp = ln.CG * DV;
  float total = 0.f;                                              // thread 0: the chunk's sum d^4 over all trips
  for (int gt = 0; gt < ln.CG; gt += ln.GW) {
    const int g = gt + ln.g;
    const bool on = ln.live && g < ln.CG;
    const int c0 = g * DV;
    float a3[DV], a3s[DV], a4 = 0.f;
    float mue[DV], loe[DV], rse[DV], mut[DV], lot[DV], rst[DV];
#pragma unroll
    for (int i = 0; i < DV; ++i) a3[i] = a3s[i] = mue[i] = loe[i] = rse[i] = mut[i] = lot[i] = rst[i] = 0.f;
    if (on) {
#pragma unroll
      for (int i = 0; i < DV; ++i) {
        if (c0 + i < C) {
          const float4d *v = reinterpret_cast<const float4d *>(cst + (int64_t)(Pl.ch0 + c0 + i) * 8);
          const float4d ve = v[0], vt = v[1];
          mue[i] = ve[0], loe[i] = ve[1], rse[i] = ve[2], mut[i] = vt[0], lot[i] = vt[1], rst[i] = vt[2];
        }
      }
      for (int r = r0 + ln.rsub; r < r1; r += ln.RS) {
        const int b = r / T, tt = r - b * T;
        float xe[DV], xt[DV];
        load8(Ly.e, b * Ly.e_sb + tt * Ly.e_st, Ly.e_dtype, Pl.e_vec, c0, C, xe);
        load8(Ly.t, b * Ly.t_sb + tt * Ly.t_st, Ly.t_dtype, Pl.t_vec, c0, C, xt);
#pragma unroll
        for (int i = 0; i < DV; ++i) {
          const float sh = ((xe[i] - mue[i]) - loe[i]) * rse[i];  // (pad channels: x = mean = rstd = 0)
          const float d = sh - ((xt[i] - mut[i]) - lot[i]) * rst[i];
          const float d2 = d * d, d3 = d2 * d;
          a3[i] += d3, a3s[i] += d3 * sh, a4 += d2 * d2;
        }
      }
    }
    __syncthreads();
    if (on) {
#pragma unroll
      for (int i = 0; i < DV; ++i) sm[tid * LW + i] = a3[i], sm[tid * LW + DV + i] = a3s[i];
      sm[tid * LW + 2 * DV] = a4;
    }
    __syncthreads();
    float mine = 0.f;
    if (on && ln.rsub == 0) {
      for (int rs = 1; rs < ln.RS; ++rs) {                        // row lanes in order
        const float *o = sm + (rs * ln.GW + ln.g) * LW;
#pragma unroll
        for (int i = 0; i < DV; ++i) a3[i] += o[i], a3s[i] += o[DV + i];
        a4 += o[2 * DV];
      }
      float *dst = part + Pl.part0 + ((int64_t)ck * Cp + c0) * 2;
#pragma unroll
      for (int i = 0; i < DV; ++i) dst[2 * i] = a3[i], dst[2 * i + 1] = a3s[i];
      mine = a4;
    }
    red[tid] = mine;                                              // a fixed tree over the channel groups
    __syncthreads();
    for (int s = DT / 2; s > 0; s >>= 1) {
      if (tid < s) red[tid] += red[tid + s];
      __syncthreads();
    }
    if (tid == 0) total += red[0];
  }
  if (tid == 0) s4[Pl.chunk0 + ck] = total;
}

__global__ __launch_bounds__(DT) void distill_loss_merge_kernel(const DistillTable tab, const float *__restrict__ part,
                                                                const float *__restrict__ s4, float kd_p,
                                                                double *__restrict__ csum, double *__restrict__ D,
                                                                float *__restrict__ L) {
  __shared__ double sh[DSTRIPES][DCB][2];
  __shared__ double red[DT];
  const int tid = threadIdx.x, cl = tid % DCB, stripe = tid / DCB;
  int cb;
  const int li = find_layer(tab, blockIdx.x, 1, cb);
  const cum_distill_layer &Ly = tab.L[li];
  const DistillPlan &Pl = tab.P[li];
  const int C = Ly.C, c = cb * DCB + cl;
  const int Cp = (C + DV - 1) / DV * DV;
  double a3 = 0.0, a3s = 0.0;
  if (c < C) {
    for (int k = stripe; k < Pl.nchunks; k += DSTRIPES) {
      const float *src = part + Pl.part0 + ((int64_t)k * Cp + c) * 2;
      a3 += (double)src[0], a3s += (double)src[1];
    }
  }
  sh[stripe][cl][0] = a3, sh[stripe][cl][1] = a3s;
  __syncthreads();
  if (stripe == 0 && c < C) {
    for (int s = 1; s < DSTRIPES; ++s) a3 += sh[s][cl][0], a3s += sh[s][cl][1];
    csum[(int64_t)(Pl.ch0 + c) * 2] = a3, csum[(int64_t)(Pl.ch0 + c) * 2 + 1] = a3s;
  }
  if (cb == 0) {                                                  // (uniform) the layer's D: chunks in a fixed tree
    double v = 0.0;
    for (int k = tid; k < Pl.nchunks; k += DT) v += (double)s4[Pl.chunk0 + k];
    red[tid] = v;
    __syncthreads();
    for (int s = DT / 2; s > 0; s >>= 1) {
      if (tid < s) red[tid] += red[tid + s];
      __syncthreads();
    }
    if (tid == 0) {
      D[li] = red[0];
      L[li] = (float)((double)kd_p * log(red[0]));
    }
  }
}

// ------------------------------------------------------------------------------------------------------------- backward
__device__ __forceinline__ void store8(void *__restrict__ base, int64_t at, int dt, const float (&v)[DV]) {
  if (dt == CUM_F32) {
    float4d *p = reinterpret_cast<float4d *>(reinterpret_cast<float *>(base) + at);
    const float4d a = {v[0], v[1], v[2], v[3]}, b = {v[4], v[5], v[6], v[7]};
    p[0] = a, p[1] = b;
  } else {
    ushort8d h;
#pragma unroll
    for (int i = 0; i < DV; ++i) h[i] = dt == CUM_BF16 ? f32_to_bf16(v[i]) : f32_to_f16(v[i]);
    *reinterpret_cast<ushort8d *>(reinterpret_cast<unsigned short *>(base) + at) = h;
  }
}

__global__ __launch_bounds__(DT) void distill_bwd_kernel(const DistillTable tab, const float *__restrict__ cst,
                                                         const double *__restrict__ csum, const double *__restrict__ D,
                                                         const float *__restrict__ G, float kd_p) {
  const int tid = threadIdx.x;
  int ck;
  const int li = find_layer(tab, blockIdx.x, 0, ck);
  const cum_distill_layer &Ly = tab.L[li];
  const DistillPlan &Pl = tab.P[li];
  const int T = Ly.T, C = Ly.C, n = Ly.B * T;
  const int r0 = ck * DROWS, r1 = r0 + DROWS < n ? r0 + DROWS : n;
  const DistillLanes ln = distill_lanes(C, tid);
  const float a = (float)(4.0 * (double)kd_p / D[li]) * G[li];    // the upstream scalar joins in f32
  const double inv_n = 1.0 / (double)n;
  const int gap = (int)(Ly.de_sb / Ly.de_st) - T;                 // rows between clips of a row-buffer de (else <= 0)
  for (int gt = 0; gt < ln.CG; gt += ln.GW) {
    const int g = gt + ln.g;
    if (!(ln.live && g < ln.CG)) continue;
    const int c0 = g * DV;
    float mue[DV], loe[DV], rse[DV], mut[DV], lot[DV], rst[DV], m3[DV], m3s[DV];
#pragma unroll
    for (int i = 0; i < DV; ++i) {
      mue[i] = loe[i] = rse[i] = mut[i] = lot[i] = rst[i] = m3[i] = m3s[i] = 0.f;
      if (c0 + i < C) {
        const float4d *v4 = reinterpret_cast<const float4d *>(cst + (int64_t)(Pl.ch0 + c0 + i) * 8);
        const float4d ve = v4[0], vt = v4[1];
        mue[i] = ve[0], loe[i] = ve[1], rse[i] = ve[2], mut[i] = vt[0], lot[i] = vt[1], rst[i] = vt[2];
        m3[i] = (float)(csum[(int64_t)(Pl.ch0 + c0 + i) * 2] * inv_n);
        m3s[i] = (float)(csum[(int64_t)(Pl.ch0 + c0 + i) * 2 + 1] * inv_n);
      }
    }
    for (int r = r0 + ln.rsub; r < r1; r += ln.RS) {
      const int b = r / T, tt = r - b * T;
      float xe[DV], xt[DV], o[DV];
      load8(Ly.e, b * Ly.e_sb + tt * Ly.e_st, Ly.e_dtype, Pl.e_vec, c0, C, xe);
      load8(Ly.t, b * Ly.t_sb + tt * Ly.t_st, Ly.t_dtype, Pl.t_vec, c0, C, xt);
#pragma unroll
      for (int i = 0; i < DV; ++i) {
        const float sh = ((xe[i] - mue[i]) - loe[i]) * rse[i];
        const float d = sh - ((xt[i] - mut[i]) - lot[i]) * rst[i];
        const float v = (rse[i] * a) * (d * d * d - m3[i] - sh * m3s[i]);
        o[i] = c0 + i < C ? v : 0.f;
      }
      const int64_t at = b * Ly.de_sb + tt * Ly.de_st + c0;
      store8(Ly.de, at, Ly.e_dtype, o);
      if (tt == T - 1 && gap > 0 && b < Ly.B - 1) {               // the rows between this clip and the next
        const float z[DV] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int q = 1; q <= gap; ++q) store8(Ly.de, at + q * Ly.de_st, Ly.e_dtype, z);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ host
static bool side_vec(const void *p, int dt, int64_t sb, int64_t st, int C) {
  const int Cp = (C + DV - 1) / DV * DV;
  const int esz = dt == CUM_F32 ? 4 : 2;
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && st >= Cp && (st * esz) % 16 == 0 && (sb * esz) % 16 == 0;
}

// Validates the layers and fills the table; sizes: {floats of part, channels, chunks, merge workgroups}
static int distill_table(const cum_distill_layer *layers, int32_t nl, bool bwd, DistillTable &tab, int64_t sizes[4]) {
  CUM_REQUIRE(layers != nullptr, "distill: null layer table");
  CUM_REQUIRE(nl >= 1 && nl <= CUM_DISTILL_MAX_LAYERS, "distill: between 1 and 16 layers per call");
  int64_t part = 0, chans = 0, chunks = 0, cbs = 0;
  tab.nl = nl, tab.pad_ = 0;
  for (int i = 0; i < nl; ++i) {
    const cum_distill_layer &y = layers[i];
    CUM_REQUIRE(y.B >= 1 && y.T >= 1 && y.C >= 1, "distill: B, T and C must be at least 1");
    const int64_t n = (int64_t)y.B * y.T;
    CUM_REQUIRE(n >= 2, "distill: fewer than 2 values per channel");
    CUM_REQUIRE(n < 0x7fffffffLL, "distill: B * T must stay below 2^31");
    CUM_REQUIRE(dtype_ok(y.e_dtype) && dtype_ok(y.t_dtype), "distill: element types are f32, bf16 or f16");
    CUM_REQUIRE(y.e != nullptr && y.t != nullptr, "distill: null feature pointer");
    CUM_REQUIRE(y.e_st >= y.C && y.t_st >= y.C, "distill: a row stride is below C");
    CUM_REQUIRE(y.B == 1 || (y.e_sb >= (int64_t)(y.T - 1) * y.e_st + y.C && y.t_sb >= (int64_t)(y.T - 1) * y.t_st + y.C),
                "distill: a clip stride is below what T rows need");
    const int Cp = (y.C + DV - 1) / DV * DV;
    if (bwd) {
      const int esz = y.e_dtype == CUM_F32 ? 4 : 2;
      CUM_REQUIRE(y.de != nullptr, "distill: null gradient pointer");
      CUM_REQUIRE((reinterpret_cast<uintptr_t>(y.de) & 15) == 0 && y.de_st >= Cp && (y.de_st * esz) % 16 == 0 &&
                      (y.de_sb * esz) % 16 == 0,
                  "distill: de must be 16-byte aligned with row strides of whole 16-byte groups that cover C rounded up to 8");
      CUM_REQUIRE(y.de_sb >= (int64_t)y.T * y.de_st && y.de_sb % y.de_st == 0,
                  "distill: de's clip stride must be a whole number of rows, at least T");
    }
    tab.L[i] = y;
    DistillPlan &p = tab.P[i];
    p.part0 = part, p.chunk0 = (int32_t)chunks, p.nchunks = (int32_t)cdiv64(n, DROWS);
    p.cb0 = (int32_t)cbs, p.ch0 = (int32_t)chans;
    p.e_vec = side_vec(y.e, y.e_dtype, y.e_sb, y.e_st, y.C);
    p.t_vec = side_vec(y.t, y.t_dtype, y.t_sb, y.t_st, y.C);
    part += (int64_t)p.nchunks * Cp * 8;
    chans += y.C, chunks += p.nchunks, cbs += cdiv64(y.C, DCB);
    CUM_REQUIRE(chunks < 0x7fffffffLL && chans < 0x7fffffffLL, "distill: too many work items");
  }
  sizes[0] = part, sizes[1] = chans, sizes[2] = chunks, sizes[3] = cbs;
  return CUM_OK;
}

}  // namespace cum

using namespace cum;

extern "C" int cum_distill_sizes(const cum_distill_layer *layers, int32_t n_layers, int64_t *sizes) {
  CUM_REQUIRE(sizes != nullptr, "distill_sizes: null sizes");
  DistillTable tab;
  int64_t s[4];
  const int rc = distill_table(layers, n_layers, false, tab, s);
  if (rc != CUM_OK) return rc;
  sizes[0] = s[0], sizes[1] = s[1], sizes[2] = s[2];
  return CUM_OK;
}

extern "C" int cum_distill_fwd(const cum_distill_layer *layers, int32_t n_layers, float kd_p, int32_t passes, float *part,
                               float *cst, double *csum, float *s4, double *D, float *L, void *stream) {
  DistillTable tab;
  int64_t s[4];
  const int rc = distill_table(layers, n_layers, false, tab, s);
  if (rc != CUM_OK) return rc;
  CUM_REQUIRE(part && cst && csum && s4 && D && L, "distill_fwd: null workspace");
  CUM_REQUIRE(((reinterpret_cast<uintptr_t>(part) | reinterpret_cast<uintptr_t>(cst)) & 15) == 0 &&
                  ((reinterpret_cast<uintptr_t>(csum) | reinterpret_cast<uintptr_t>(D)) & 7) == 0,
              "distill_fwd: part and cst must be 16-byte aligned, csum and D 8-byte aligned");
  const dim3 block(DT), chunks((unsigned)s[2]), cbs((unsigned)s[3]);
  if (passes & 1) {
    hipLaunchKernelGGL(distill_stats_kernel, chunks, block, 0, (hipStream_t)stream, tab, part);
    CUM_CHECK_LAUNCH();
    hipLaunchKernelGGL(distill_stats_merge_kernel, cbs, block, 0, (hipStream_t)stream, tab, part, cst);
    CUM_CHECK_LAUNCH();
  }
  if (passes & 2) {
    hipLaunchKernelGGL(distill_loss_kernel, chunks, block, 0, (hipStream_t)stream, tab, cst, part, s4);
    CUM_CHECK_LAUNCH();
    hipLaunchKernelGGL(distill_loss_merge_kernel, cbs, block, 0, (hipStream_t)stream, tab, part, s4, kd_p, csum, D, L);
    CUM_CHECK_LAUNCH();
  }
  return CUM_OK;
}

extern "C" int cum_distill_bwd(const cum_distill_layer *layers, int32_t n_layers, float kd_p, const float *cst,
                               const double *csum, const double *D, const float *G, void *stream) {
  DistillTable tab;
  int64_t s[4];
  const int rc = distill_table(layers, n_layers, true, tab, s);
  if (rc != CUM_OK) return rc;
  CUM_REQUIRE(cst && csum && D && G, "distill_bwd: null workspace");
  CUM_REQUIRE((reinterpret_cast<uintptr_t>(cst) & 15) == 0 &&
                  ((reinterpret_cast<uintptr_t>(csum) | reinterpret_cast<uintptr_t>(D)) & 7) == 0,
              "distill_bwd: cst must be 16-byte aligned, csum and D 8-byte aligned");
  hipLaunchKernelGGL(distill_bwd_kernel, dim3((unsigned)s[2]), dim3(DT), 0, (hipStream_t)stream, tab, cst, csum, D, G, kd_p);
  CUM_CHECK_LAUNCH();
  return CUM_OK;
}
