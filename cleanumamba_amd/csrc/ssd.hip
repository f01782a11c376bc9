// Mamba2 bottleneck (mamba_v2=True): the chunked state-space-duality scan forward and backward, the gated RMSNorm of
// its output forward and backward, and the one-token step of streaming inference.
//
// Replaces mamba-ssm 2.x `mamba_chunk_scan_combined` (ngroups 1, dt_softplus, dt_bias, D per head, no z: the gate goes
// through RMSNormGated), `RMSNormGated(norm_before_gate=False)` and the step path of `Mamba2.step`
// (`selective_state_update` with a scalar decay per head).  Per head h, with dt_t = softplus(dt_raw_t + dt_bias_h),
// A_h = -exp(A_log_h), a_t = exp(dt_t A_h) and the (headdim x d_state) state h_t:
//     h_t = a_t h_{t-1} + dt_t x_t B_t^T,      y_t = h_t C_t + D_h x_t.
//
// Forward (three launches).  The sequence is cut into chunks of kSsdChunk steps.
//   1. ssd_chunk_kernel<LOCAL>: one wave per (batch, head, chunk) runs the recurrence from a zero state and writes the
//      chunk's end state and its total decay exp(sum dt A).
//   2. ssd_carry_fwd_kernel: one workgroup per (batch, head) walks the chunks in order, turning the local end states
//      into chunk-START states in place (h_start[c+1] = decay_c h_start[c] + local_c).  These are the only states kept
//      for the backward.
//   3. ssd_chunk_kernel<OUTPUT>: one wave per chunk reruns the recurrence from its start state and writes y.
//   The grid of 1 and 3 is batch x heads x chunks waves: a single clip still spreads over the chip.
// Backward (three launches + a fixed-order reduce).  With cum_t = sum_{k <= t in chunk} dt_k A and R_c the adjoint of the
// chunk's last state arriving from later chunks, every gradient of a chunk is a closed form in the chunk's own data
// (the SSD "quadratic" form, Q x Q matrices C B^T and dY X^T with the decay mask exp(cum_t - cum_u), u <= t):
//   1. ssd_bwd_local_kernel: L_c = sum_t exp(cum_t) dy_t C_t^T per chunk;
//   2. ssd_carry_bwd_kernel: R_{c-1} = decay_c R_c + L_c from the last chunk down;
//   3. ssd_bwd_chunk_kernel: one 256-thread workgroup per chunk forms the Q x Q matrices in LDS and writes dx, d dt_raw
//      and per-head slabs of dB, dC plus per-chunk partials of dA_log, dD, d dt_bias;
//   4. ssd_reduce_kernel: dB / dC summed over heads and the parameter partials over (batch, chunk), in fixed order.
// No float atomics anywhere: two runs give the same bits.
#include "common.h"

namespace cum {

constexpr int kSsdChunk = 32;

template <typename T>
__device__ __forceinline__ float sld(const void *p, int64_t i) { return (float)static_cast<const T *>(p)[i]; }
template <typename T>
__device__ __forceinline__ void sst(void *p, int64_t i, float v) { static_cast<T *>(p)[i] = (T)v; }

__device__ __forceinline__ float ssd_dt(float raw, float bias) { return softplus20(raw + bias); }

struct SsdArgs {
  cum_ssd_shape s;
  int nchunks;
  const void *x, *dt, *B, *C;
  const float *dt_bias, *A_log, *D;
  void *y;
  float *H, *dec;      // H: [batch][nheads][nchunks + 1][P][N]; dec: [batch][nheads][nchunks]
  float *final_state;  // (batch, nheads, P, N) or null
};

// LOCAL: end state of the chunk from a zero state -> H slot c + 1, decay -> dec.  OUTPUT: y from the start state H[c].
template <typename T, int P, int N, bool OUTPUT>
__global__ __launch_bounds__(64) void ssd_chunk_kernel(const SsdArgs a) {
  constexpr int S = 64 / P;        // lanes sharing one row p of the state
  constexpr int NS = N / S;        // state entries per lane
  __shared__ float sB[kSsdChunk][N], sC[kSsdChunk][N], sdt[kSsdChunk];
  const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int lane = threadIdx.x, p = lane / S, sl = lane % S;
  const cum_ssd_shape &s = a.s;
  const int t0 = c * kSsdChunk, Qc = min(kSsdChunk, s.len - t0);
  const float A = -__expf(a.A_log[h]), bias = a.dt_bias[h];
  for (int e = lane; e < Qc * N; e += 64) {
    const int t = e / N, n = e % N;
    const int64_t r = (int64_t)b * s.B_sb + (int64_t)(t0 + t) * s.B_sl;
    sB[t][n] = sld<T>(a.B, r + n);
    sC[t][n] = sld<T>(a.C, (int64_t)b * s.C_sb + (int64_t)(t0 + t) * s.C_sl + n);
  }
  for (int t = lane; t < Qc; t += 64)
    sdt[t] = ssd_dt(sld<T>(a.dt, (int64_t)b * s.dt_sb + (int64_t)(t0 + t) * s.dt_sl + h), bias);
  __syncthreads();
  const int64_t hb = ((int64_t)b * s.nheads + h) * (a.nchunks + 1);
  float st[NS];
  if (OUTPUT) {
    const float *h0 = a.H + (hb + c) * P * N + p * N + sl * NS;
#pragma unroll
    for (int j = 0; j < NS; ++j) st[j] = h0[j];
  } else {
#pragma unroll
    for (int j = 0; j < NS; ++j) st[j] = 0.f;
  }
  const float Dh = a.D ? a.D[h] : 0.f;
  float lsum = 0.f;
  for (int t = 0; t < Qc; ++t) {
    const float dt = sdt[t];
    const float da = __expf(dt * A);
    lsum += dt * A;
    const int64_t tg = t0 + t;
    const float xv = sld<T>(a.x, (int64_t)b * s.x_sb + tg * s.x_sl + h * P + p);
    const float dx = dt * xv;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      st[j] = fmaf(st[j], da, dx * sB[t][sl * NS + j]);
      if (OUTPUT) acc = fmaf(st[j], sC[t][sl * NS + j], acc);
    }
    if (OUTPUT) {
#pragma unroll
      for (int o = 1; o < S; o <<= 1) acc += __shfl_xor(acc, o, 64);
      if (sl == 0) sst<T>(a.y, (int64_t)b * s.y_sb + tg * s.y_sl + h * P + p, fmaf(Dh, xv, acc));
    }
  }
  if (!OUTPUT) {
    float *dst = a.H + (hb + c + 1) * P * N + p * N + sl * NS;
#pragma unroll
    for (int j = 0; j < NS; ++j) dst[j] = st[j];
    if (lane == 0) a.dec[((int64_t)b * s.nheads + h) * a.nchunks + c] = __expf(lsum);
  }
}

// H[0] = 0; H[c + 1] = dec[c] H[c] + H[c + 1] for c = 0 .. nchunks - 2: slots 0 .. nchunks - 1 end as chunk-start
// states.  Slot nchunks is never rewritten (it keeps the last chunk's LOCAL end state); the final state goes only to
// final_state.
__global__ __launch_bounds__(256) void ssd_carry_fwd_kernel(float *H, const float *dec, int nchunks, int PN,
                                                            float *final_state) {
  const int64_t bh = blockIdx.x;
  float *base = H + bh * (int64_t)(nchunks + 1) * PN;
  const float *d = dec + bh * nchunks;
  for (int e = threadIdx.x; e < PN; e += 256) {
    float run = 0.f;
    base[e] = 0.f;
    for (int c = 0; c < nchunks; ++c) {
      run = fmaf(d[c], run, base[(int64_t)(c + 1) * PN + e]);
      if (c + 1 < nchunks) base[(int64_t)(c + 1) * PN + e] = run;
    }
    if (final_state) final_state[bh * PN + e] = run;
  }
}

struct SsdBwdArgs {
  SsdArgs f;
  const void *dy;
  void *dx, *ddt;
  float *R;                   // [batch][nheads][nchunks][P][N]
  float *slabB, *slabC;       // [nheads][batch][len][N]
  float *part;                // [3][nheads][batch * nchunks]: d A, d D, d dt_bias per chunk
};

// L_c = sum_t exp(cum_t) dy_t C_t^T for chunks c >= 1, into R slot c - 1.
template <typename T, int P, int N>
__global__ __launch_bounds__(64) void ssd_bwd_local_kernel(const SsdBwdArgs g) {
  constexpr int S = 64 / P, NS = N / S;
  __shared__ float sC[kSsdChunk][N], sdt[kSsdChunk];
  const SsdArgs &a = g.f;
  const cum_ssd_shape &s = a.s;
  const int c = blockIdx.x + 1, h = blockIdx.y, b = blockIdx.z;
  const int lane = threadIdx.x, p = lane / S, sl = lane % S;
  const int t0 = c * kSsdChunk, Qc = min(kSsdChunk, s.len - t0);
  const float A = -__expf(a.A_log[h]), bias = a.dt_bias[h];
  for (int e = lane; e < Qc * N; e += 64) {
    const int t = e / N, n = e % N;
    sC[t][n] = sld<T>(a.C, (int64_t)b * s.C_sb + (int64_t)(t0 + t) * s.C_sl + n);
  }
  for (int t = lane; t < Qc; t += 64)
    sdt[t] = ssd_dt(sld<T>(a.dt, (int64_t)b * s.dt_sb + (int64_t)(t0 + t) * s.dt_sl + h), bias);
  __syncthreads();
  float acc[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) acc[j] = 0.f;
  float cum = 0.f;
  for (int t = 0; t < Qc; ++t) {
    cum += sdt[t] * A;
    const float w = __expf(cum) * sld<T>(g.dy, (int64_t)b * s.y_sb + (int64_t)(t0 + t) * s.y_sl + h * P + p);
#pragma unroll
    for (int j = 0; j < NS; ++j) acc[j] = fmaf(w, sC[t][sl * NS + j], acc[j]);
  }
  float *dst = g.R + ((((int64_t)b * s.nheads + h) * a.nchunks + c - 1) * P + p) * N + sl * NS;
#pragma unroll
  for (int j = 0; j < NS; ++j) dst[j] = acc[j];
}

// R[nchunks - 1] = 0; R[c - 1] = dec[c] R[c] + R[c - 1] for c = nchunks - 1 .. 1.
__global__ __launch_bounds__(256) void ssd_carry_bwd_kernel(float *R, const float *dec, int nchunks, int PN) {
  const int64_t bh = blockIdx.x;
  float *base = R + bh * (int64_t)nchunks * PN;
  const float *d = dec + bh * nchunks;
  for (int e = threadIdx.x; e < PN; e += 256) {
    float run = 0.f;
    base[(int64_t)(nchunks - 1) * PN + e] = 0.f;
    for (int c = nchunks - 1; c >= 1; --c) {
      run = fmaf(d[c], run, base[(int64_t)(c - 1) * PN + e]);
      base[(int64_t)(c - 1) * PN + e] = run;
    }
  }
}

__device__ __forceinline__ float block_sum256(float v, float *red) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

template <typename T, int P, int N>
__global__ __launch_bounds__(256) void ssd_bwd_chunk_kernel(const SsdBwdArgs g) {
  constexpr int Q = kSsdChunk;
  __shared__ float sX[Q][P], sDY[Q][P], sRB[Q][P], sHC[Q][P];
  __shared__ float sB[Q][N], sC[Q][N];
  __shared__ float sG1[Q][Q + 1], sG2[Q][Q + 1], sM[Q][Q + 1];
  __shared__ float sdt[Q], scum[Q], sdcum[Q], sdir[Q], sRBx[Q], red[4];
  const SsdArgs &a = g.f;
  const cum_ssd_shape &s = a.s;
  const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const int t0 = c * Q, Qc = min(Q, s.len - t0);
  const float A = -__expf(a.A_log[h]), bias = a.dt_bias[h], Dh = a.D ? a.D[h] : 0.f;
  const int64_t bh = (int64_t)b * s.nheads + h;
  const float *hs = a.H + (bh * (a.nchunks + 1) + c) * P * N;
  const float *R = g.R + (bh * a.nchunks + c) * P * N;
  for (int e = tid; e < Q * P; e += 256) {
    const int t = e / P, p = e % P;
    const bool v = t < Qc;
    const int64_t tg = t0 + t;
    sX[t][p] = v ? sld<T>(a.x, (int64_t)b * s.x_sb + tg * s.x_sl + h * P + p) : 0.f;
    sDY[t][p] = v ? sld<T>(g.dy, (int64_t)b * s.y_sb + tg * s.y_sl + h * P + p) : 0.f;
  }
  for (int e = tid; e < Q * N; e += 256) {
    const int t = e / N, n = e % N;
    const bool v = t < Qc;
    const int64_t tg = t0 + t;
    sB[t][n] = v ? sld<T>(a.B, (int64_t)b * s.B_sb + tg * s.B_sl + n) : 0.f;
    sC[t][n] = v ? sld<T>(a.C, (int64_t)b * s.C_sb + tg * s.C_sl + n) : 0.f;
  }
  if (tid < Q) sdt[tid] = tid < Qc ? ssd_dt(sld<T>(a.dt, (int64_t)b * s.dt_sb + (int64_t)(t0 + tid) * s.dt_sl + h), bias) : 0.f;
  __syncthreads();
  if (tid == 0) {
    float cum = 0.f;
    for (int t = 0; t < Q; ++t) {
      cum += sdt[t] * A;
      scum[t] = cum;
    }
  }
  // R B_u and h_start C_t (rows of the two P x N matrices against the chunk's B / C)
  for (int e = tid; e < Q * P; e += 256) {
    const int t = e / P, p = e % P;
    float rb = 0.f, hc = 0.f;
    for (int n = 0; n < N; ++n) {
      rb = fmaf(R[p * N + n], sB[t][n], rb);
      hc = fmaf(hs[p * N + n], sC[t][n], hc);
    }
    sRB[t][p] = rb;
    sHC[t][p] = hc;
  }
  __syncthreads();
  for (int e = tid; e < Q * Q; e += 256) {
    const int t = e / Q, u = e % Q;
    float g1 = 0.f, g2 = 0.f;
    for (int n = 0; n < N; ++n) g1 = fmaf(sC[t][n], sB[u][n], g1);
    for (int p = 0; p < P; ++p) g2 = fmaf(sDY[t][p], sX[u][p], g2);
    sG1[t][u] = g1;
    sG2[t][u] = g2;
    sM[t][u] = u <= t ? __expf(scum[t] - scum[u]) : 0.f;
  }
  float rh = 0.f;
  for (int e = tid; e < P * N; e += 256) rh = fmaf(R[e], hs[e], rh);
  rh = block_sum256(rh, red);           // <R, h_start> (its barriers also publish sG1 / sG2 / sM)
  const float clast = scum[Qc - 1];
  if (tid < Q) {
    const int t = tid;
    float rbx = 0.f, hcdy = 0.f;
    for (int p = 0; p < P; ++p) {
      rbx = fmaf(sX[t][p], sRB[t][p], rbx);
      hcdy = fmaf(sDY[t][p], sHC[t][p], hcdy);
    }
    sRBx[t] = rbx;
    // d cum_t: via exp(cum_t) h_start, via M[t][.] (t as row) and M[.][t] (t as column), via the carried-out state
    float dc = t < Qc ? __expf(scum[t]) * hcdy : 0.f;
    float dir = 0.f;
    // (the u = t terms of the two sums cancel exactly: both are left out)
    for (int u = 0; u < t; ++u) dc += sM[t][u] * sdt[u] * sG1[t][u] * sG2[t][u];
    dir += sG1[t][t] * sG2[t][t];
    for (int t2 = t + 1; t2 < Q; ++t2) {
      const float m = sM[t2][t] * sG1[t2][t] * sG2[t2][t];
      dc -= m * sdt[t];
      dir += m;
    }
    const float et = t < Qc ? __expf(clast - scum[t]) : 0.f;
    dir += et * rbx;
    dc -= et * sdt[t] * rbx;
    sdcum[t] = dc;
    sdir[t] = dir;
  }
  __syncthreads();
  if (tid == 0) {
    float esum = 0.f;
    for (int u = 0; u < Qc; ++u) esum += __expf(clast - scum[u]) * sdt[u] * sRBx[u];
    sdcum[Qc - 1] += __expf(clast) * rh + esum;
    float rc = 0.f, dA = 0.f, dbias = 0.f, dD = 0.f;
    for (int k = Qc - 1; k >= 0; --k) {
      rc += sdcum[k];
      dA = fmaf(sdt[k], rc, dA);
      const float raw = sld<T>(a.dt, (int64_t)b * s.dt_sb + (int64_t)(t0 + k) * s.dt_sl + h);
      const float ddt = (sdir[k] + A * rc) * sigmoidf_(raw + bias);
      sst<T>(g.ddt, (int64_t)b * s.dt_sb + (int64_t)(t0 + k) * s.dt_sl + h, ddt);
      dbias += ddt;
      dD += sG2[k][k];
    }
    const int64_t np = (int64_t)s.batch * a.nchunks, slot = (int64_t)b * a.nchunks + c;
    g.part[(int64_t)h * np + slot] = dA * A;                       // d A_log = d A * A
    g.part[((int64_t)s.nheads + h) * np + slot] = dD;
    g.part[((int64_t)2 * s.nheads + h) * np + slot] = dbias;
  }
  // dx[u][p] = sum_{t >= u} M[t][u] dt_u G1[t][u] dy_t[p] + D dy_u[p] + exp(cum_last - cum_u) dt_u (R B_u)[p]
  for (int e = tid; e < Qc * P; e += 256) {
    const int u = e / P, p = e % P;
    float acc = 0.f;
    for (int t = u; t < Qc; ++t) acc = fmaf(sM[t][u] * sG1[t][u], sDY[t][p], acc);
    const float v = sdt[u] * (acc + __expf(clast - scum[u]) * sRB[u][p]) + Dh * sDY[u][p];
    sst<T>(g.dx, (int64_t)b * s.x_sb + (int64_t)(t0 + u) * s.x_sl + h * P + p, v);
  }
  // dB[u][n] = dt_u (sum_{t >= u} M[t][u] G2[t][u] C_t[n] + exp(cum_last - cum_u) (x_u^T R)[n])
  // dC[t][n] = exp(cum_t) (dy_t^T h_start)[n] + sum_{u <= t} M[t][u] dt_u G2[t][u] B_u[n]
  float *slB = g.slabB + ((int64_t)h * s.batch + b) * s.len * N;
  float *slC = g.slabC + ((int64_t)h * s.batch + b) * s.len * N;
  for (int e = tid; e < Qc * N; e += 256) {
    const int u = e / N, n = e % N;
    float accB = 0.f, accC = 0.f, xr = 0.f, dyh = 0.f;
    for (int t = u; t < Qc; ++t) accB = fmaf(sM[t][u] * sG2[t][u], sC[t][n], accB);
    for (int v = 0; v <= u; ++v) accC = fmaf(sM[u][v] * sdt[v] * sG2[u][v], sB[v][n], accC);
    for (int p = 0; p < P; ++p) {
      xr = fmaf(sX[u][p], R[p * N + n], xr);
      dyh = fmaf(sDY[u][p], hs[p * N + n], dyh);
    }
    slB[(int64_t)(t0 + u) * N + n] = sdt[u] * (accB + __expf(clast - scum[u]) * xr);
    slC[(int64_t)(t0 + u) * N + n] = __expf(scum[u]) * dyh + accC;
  }
}

// dB, dC: sum over heads in head order (rows of batch x len, N columns).  Parameter partials: sum over (batch, chunk).
template <typename T>
__global__ __launch_bounds__(256) void ssd_reduce_kernel(const SsdBwdArgs g, void *dB, int64_t dB_sb, int64_t dB_sl,
                                                         void *dC, int64_t dC_sb, int64_t dC_sl, float *dA_log,
                                                         float *dD, float *ddt_bias) {
  const cum_ssd_shape &s = g.f.s;
  const int N = s.dstate;
  const int64_t total = (int64_t)s.batch * s.len * N;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < total) {
    const int64_t row = e / N, n = e % N, b = row / s.len, t = row % s.len;
    float sb = 0.f, sc = 0.f;
    for (int h = 0; h < s.nheads; ++h) {
      sb += g.slabB[(int64_t)h * total + e];
      sc += g.slabC[(int64_t)h * total + e];
    }
    sst<T>(dB, b * dB_sb + t * dB_sl + n, sb);
    sst<T>(dC, b * dC_sb + t * dC_sl + n, sc);
  }
  if (blockIdx.x == 0) {
    const int64_t np = (int64_t)s.batch * g.f.nchunks;
    for (int i = threadIdx.x; i < 3 * s.nheads; i += 256) {
      const float *src = g.part + (int64_t)i * np;
      float acc = 0.f;
      for (int64_t j = 0; j < np; ++j) acc += src[j];
      const int k = i / s.nheads, h = i % s.nheads;
      (k == 0 ? dA_log : k == 1 ? dD : ddt_bias)[h] = acc;
    }
  }
}

// ---------------------------------------------------------------- gated RMSNorm: out = rmsnorm(y * silu(z)) * w
__device__ __forceinline__ float silu_(float z) { return z * sigmoidf_(z); }

template <typename T>
__global__ __launch_bounds__(256) void gnorm_fwd_kernel(int64_t rows, int dim, const void *y, int64_t y_ld,
                                                        const void *z, int64_t z_ld, const float *w, float eps, void *out,
                                                        int64_t o_ld, float *rstd) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float q = 0.f;
  for (int e = lane; e < dim; e += 64) {
    const float gv = sld<T>(y, row * y_ld + e) * silu_(sld<T>(z, row * z_ld + e));
    q = fmaf(gv, gv, q);
  }
  for (int o = 32; o >= 1; o >>= 1) q += __shfl_xor(q, o, 64);
  const float r = rsqrtf(q / dim + eps);
  if (lane == 0 && rstd) rstd[row] = r;
  for (int e = lane; e < dim; e += 64) {
    const float gv = sld<T>(y, row * y_ld + e) * silu_(sld<T>(z, row * z_ld + e));
    sst<T>(out, row * o_ld + e, gv * r * w[e]);
  }
}

// One workgroup (4 waves) per `rows_per_block` rows; dw partials per workgroup -> slab [gridDim.x][dim].
template <typename T>
__global__ __launch_bounds__(256) void gnorm_bwd_kernel(int64_t rows, int dim, int64_t rows_per_block, const void *y,
                                                        int64_t y_ld, const void *z, int64_t z_ld, const float *w,
                                                        const float *rstd, const void *dout, int64_t d_ld, void *dy,
                                                        int64_t dy_ld, void *dz, int64_t dz_ld, float *slab) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block, r1 = min(rows, r0 + rows_per_block);
  extern __shared__ float sdw[];     // [4][dim]
  for (int e = lane; e < dim; e += 64) sdw[wv * dim + e] = 0.f;
  for (int64_t row = r0 + wv; row < r1; row += 4) {
    const float r = rstd[row];
    float dot = 0.f;
    for (int e = lane; e < dim; e += 64) {
      const float gv = sld<T>(y, row * y_ld + e) * silu_(sld<T>(z, row * z_ld + e));
      const float go = sld<T>(dout, row * d_ld + e);
      dot = fmaf(go * w[e], gv, dot);
      sdw[wv * dim + e] = fmaf(go, gv * r, sdw[wv * dim + e]);
    }
    for (int o = 32; o >= 1; o >>= 1) dot += __shfl_xor(dot, o, 64);
    const float k = dot * r * r * r / dim;
    for (int e = lane; e < dim; e += 64) {
      const float yv = sld<T>(y, row * y_ld + e), zv = sld<T>(z, row * z_ld + e);
      const float sg = sigmoidf_(zv), sz = zv * sg;
      const float gv = yv * sz;
      const float dg = sld<T>(dout, row * d_ld + e) * w[e] * r - gv * k;
      sst<T>(dy, row * dy_ld + e, dg * sz);
      sst<T>(dz, row * dz_ld + e, dg * yv * sg * (1.f + zv * (1.f - sg)));
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < dim; e += 256)
    slab[(int64_t)blockIdx.x * dim + e] = sdw[e] + sdw[dim + e] + sdw[2 * dim + e] + sdw[3 * dim + e];
}

__global__ __launch_bounds__(256) void gnorm_dw_reduce_kernel(const float *slab, int nblocks, int dim, float *dw) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= dim) return;
  float acc = 0.f;
  for (int i = 0; i < nblocks; ++i) acc += slab[(int64_t)i * dim + e];
  dw[e] = acc;
}

// ---------------------------------------------------------------- one token of every stream
struct Ssd2StepArgs {
  int streams, d_ssm, nheads, headdim, dstate, width;
  float eps;
  const float *zxbcdt;
  int64_t ld;
  float *conv_state;           // (streams, conv_dim, width)
  const float *conv_w, *conv_b, *dt_bias, *A_log, *D, *norm_w;
  float *ssm_state;            // (streams, nheads, headdim, dstate)
  float *out;                  // (streams, d_ssm)
  int64_t out_ld;
};

constexpr int kStepMaxConv = 2048 + 2 * 64;
constexpr int kStepMaxSsm = 2048;

__global__ __launch_bounds__(256) void ssd_step_kernel(const Ssd2StepArgs a) {
  __shared__ float sx[kStepMaxConv], sy[kStepMaxSsm], red[4];
  const int sidx = blockIdx.x, tid = threadIdx.x;
  const int conv_dim = a.d_ssm + 2 * a.dstate, W = a.width;
  const float *row = a.zxbcdt + (int64_t)sidx * a.ld;
  const float *z = row, *xbc = row + a.d_ssm, *dtr = row + a.d_ssm + conv_dim;
  for (int ch = tid; ch < conv_dim; ch += 256) {
    float *cs = a.conv_state + ((int64_t)sidx * conv_dim + ch) * W;
    float acc = a.conv_b ? a.conv_b[ch] : 0.f;
    for (int k = 0; k < W - 1; ++k) {
      cs[k] = cs[k + 1];
      acc = fmaf(cs[k], a.conv_w[ch * W + k], acc);
    }
    const float v = xbc[ch];
    cs[W - 1] = v;
    acc = fmaf(v, a.conv_w[ch * W + W - 1], acc);
    sx[ch] = silu_(acc);
  }
  __syncthreads();
  const float *Bv = sx + a.d_ssm, *Cv = sx + a.d_ssm + a.dstate;
  for (int i = tid; i < a.d_ssm; i += 256) {
    const int h = i / a.headdim;
    const float dt = ssd_dt(dtr[h], a.dt_bias[h]);
    const float da = __expf(-__expf(a.A_log[h]) * dt);
    const float xv = sx[i], dx = dt * xv;
    float *st = a.ssm_state + ((int64_t)sidx * a.d_ssm + i) * a.dstate;
    float acc = 0.f;
    for (int n = 0; n < a.dstate; ++n) {
      const float v = fmaf(st[n], da, dx * Bv[n]);
      st[n] = v;
      acc = fmaf(v, Cv[n], acc);
    }
    sy[i] = (acc + a.D[h] * xv) * silu_(z[i]);
  }
  __syncthreads();
  float q = 0.f;
  for (int i = tid; i < a.d_ssm; i += 256) q = fmaf(sy[i], sy[i], q);
  for (int o = 32; o >= 1; o >>= 1) q += __shfl_xor(q, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = q;
  __syncthreads();
  const float r = rsqrtf((red[0] + red[1] + red[2] + red[3]) / a.d_ssm + a.eps);
  for (int i = tid; i < a.d_ssm; i += 256) a.out[(int64_t)sidx * a.out_ld + i] = sy[i] * r * a.norm_w[i];
}

}  // namespace cum

using namespace cum;

static bool ssd_shape_ok(const cum_ssd_shape *s) {
  if (!s || s->batch < 0 || s->len < 0 || s->nheads < 1 || s->nheads > 256 || !dtype_ok(s->io_dtype)) return false;
  const bool pd = s->headdim == 16 || s->headdim == 32 || s->headdim == 64;
  const bool nd = s->dstate == 16 || s->dstate == 32 || s->dstate == 64;
  return pd && nd;
}

static int ssd_nchunks(int32_t len) { return (int)cdiv64(len, kSsdChunk); }

extern "C" int cum_ssd_chunk(void) { return kSsdChunk; }

extern "C" int64_t cum_ssd_states_elems(int32_t batch, int32_t len, int32_t nheads, int32_t headdim, int32_t dstate) {
  const int64_t nc = ssd_nchunks(len);
  return (int64_t)batch * nheads * ((nc + 1) * headdim * dstate + nc);
}

extern "C" int64_t cum_ssd_bwd_workspace_elems(int32_t batch, int32_t len, int32_t nheads, int32_t headdim,
                                               int32_t dstate) {
  const int64_t nc = ssd_nchunks(len);
  return (int64_t)batch * nheads * nc * headdim * dstate + 2 * (int64_t)nheads * batch * len * dstate +
         3 * (int64_t)nheads * batch * nc;
}

template <typename T, int P, int N>
static void ssd_fwd_launch(const SsdArgs &a, hipStream_t st) {
  const dim3 grid(a.nchunks, a.s.nheads, a.s.batch);
  ssd_chunk_kernel<T, P, N, false><<<grid, 64, 0, st>>>(a);
  ssd_carry_fwd_kernel<<<a.s.batch * a.s.nheads, 256, 0, st>>>(a.H, a.dec, a.nchunks, P * N, a.final_state);
  ssd_chunk_kernel<T, P, N, true><<<grid, 64, 0, st>>>(a);
}

template <typename T, int P, int N>
static void ssd_bwd_launch(const SsdBwdArgs &g, hipStream_t st) {
  const SsdArgs &a = g.f;
  if (a.nchunks > 1)
    ssd_bwd_local_kernel<T, P, N><<<dim3(a.nchunks - 1, a.s.nheads, a.s.batch), 64, 0, st>>>(g);
  ssd_carry_bwd_kernel<<<a.s.batch * a.s.nheads, 256, 0, st>>>(g.R, a.dec, a.nchunks, P * N);
  ssd_bwd_chunk_kernel<T, P, N><<<dim3(a.nchunks, a.s.nheads, a.s.batch), 256, 0, st>>>(g);
}

#define SSD_DISPATCH_PN(FN, T, ARGS, ST)                                              \
  switch (s->headdim * 1000 + s->dstate) {                                            \
    case 16016: FN<T, 16, 16>(ARGS, ST); break;                                       \
    case 16032: FN<T, 16, 32>(ARGS, ST); break;                                       \
    case 16064: FN<T, 16, 64>(ARGS, ST); break;                                       \
    case 32016: FN<T, 32, 16>(ARGS, ST); break;                                       \
    case 32032: FN<T, 32, 32>(ARGS, ST); break;                                       \
    case 32064: FN<T, 32, 64>(ARGS, ST); break;                                       \
    case 64016: FN<T, 64, 16>(ARGS, ST); break;                                       \
    case 64032: FN<T, 64, 32>(ARGS, ST); break;                                       \
    default: FN<T, 64, 64>(ARGS, ST); break;                                          \
  }

#define SSD_DISPATCH(FN, ARGS, ST)                                                    \
  if (s->io_dtype == CUM_F32) {                                                       \
    SSD_DISPATCH_PN(FN, float, ARGS, ST)                                              \
  } else if (s->io_dtype == CUM_BF16) {                                               \
    SSD_DISPATCH_PN(FN, __bf16, ARGS, ST)                                             \
  } else {                                                                            \
    SSD_DISPATCH_PN(FN, f16, ARGS, ST)                                                \
  }

static SsdArgs ssd_args(const cum_ssd_shape *s, const void *x, const void *dt, const float *dt_bias,
                        const float *A_log, const float *D, const void *B, const void *C, void *y, float *states,
                        float *final_state) {
  SsdArgs a;
  a.s = *s;
  a.nchunks = ssd_nchunks(s->len);
  a.x = x; a.dt = dt; a.B = B; a.C = C;
  a.dt_bias = dt_bias; a.A_log = A_log; a.D = D;
  a.y = y;
  a.H = states;
  a.dec = states + (int64_t)s->batch * s->nheads * (a.nchunks + 1) * s->headdim * s->dstate;
  a.final_state = final_state;
  return a;
}

extern "C" int cum_ssd_fwd(const cum_ssd_shape *s, const void *x, const void *dt, const float *dt_bias,
                           const float *A_log, const float *D, const void *B, const void *C, void *y, float *states,
                           float *final_state, void *stream) {
  CUM_REQUIRE(ssd_shape_ok(s), "cum_ssd_fwd: unsupported shape (ngroups 1, headdim and dstate in {16, 32, 64})");
  CUM_REQUIRE(x && dt && dt_bias && A_log && B && C && y && states, "cum_ssd_fwd: null pointer");
  if (s->batch == 0 || s->len == 0) return 0;
  const SsdArgs a = ssd_args(s, x, dt, dt_bias, A_log, D, B, C, y, states, final_state);
  hipStream_t st = (hipStream_t)stream;
  SSD_DISPATCH(ssd_fwd_launch, a, st)
  CUM_CHECK_LAUNCH();
  return 0;
}

extern "C" int cum_ssd_bwd(const cum_ssd_shape *s, const void *x, const void *dt, const float *dt_bias,
                           const float *A_log, const float *D, const void *B, const void *C, const void *dy,
                           const float *states, void *dx, void *ddt, void *dB, int64_t dB_sb, int64_t dB_sl, void *dC,
                           int64_t dC_sb, int64_t dC_sl, float *dA_log, float *dD, float *ddt_bias, float *workspace,
                           void *stream) {
  CUM_REQUIRE(ssd_shape_ok(s), "cum_ssd_bwd: unsupported shape (ngroups 1, headdim and dstate in {16, 32, 64})");
  CUM_REQUIRE(x && dt && dt_bias && A_log && D && B && C && dy && states && dx && ddt && dB && dC && dA_log && dD &&
                  ddt_bias && workspace,
              "cum_ssd_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (s->batch == 0 || s->len == 0) {
    hipMemsetAsync(dA_log, 0, s->nheads * sizeof(float), st);
    hipMemsetAsync(dD, 0, s->nheads * sizeof(float), st);
    hipMemsetAsync(ddt_bias, 0, s->nheads * sizeof(float), st);
    CUM_CHECK_LAUNCH();
    return 0;
  }
  SsdBwdArgs g;
  g.f = ssd_args(s, x, dt, dt_bias, A_log, D, B, C, nullptr, const_cast<float *>(states), nullptr);
  g.dy = dy; g.dx = dx; g.ddt = ddt;
  const int64_t nc = g.f.nchunks;
  g.R = workspace;
  g.slabB = g.R + (int64_t)s->batch * s->nheads * nc * s->headdim * s->dstate;
  g.slabC = g.slabB + (int64_t)s->nheads * s->batch * s->len * s->dstate;
  g.part = g.slabC + (int64_t)s->nheads * s->batch * s->len * s->dstate;
  SSD_DISPATCH(ssd_bwd_launch, g, st)
  const int64_t total = (int64_t)s->batch * s->len * s->dstate;
  const int blocks = (int)cdiv64(total, 256);
  if (s->io_dtype == CUM_F32)
    ssd_reduce_kernel<float><<<blocks, 256, 0, st>>>(g, dB, dB_sb, dB_sl, dC, dC_sb, dC_sl, dA_log, dD, ddt_bias);
  else if (s->io_dtype == CUM_BF16)
    ssd_reduce_kernel<__bf16><<<blocks, 256, 0, st>>>(g, dB, dB_sb, dB_sl, dC, dC_sb, dC_sl, dA_log, dD, ddt_bias);
  else
    ssd_reduce_kernel<f16><<<blocks, 256, 0, st>>>(g, dB, dB_sb, dB_sl, dC, dC_sb, dC_sl, dA_log, dD, ddt_bias);
  CUM_CHECK_LAUNCH();
  return 0;
}

extern "C" int cum_gated_rmsnorm_fwd(int32_t dtype, int64_t rows, int32_t dim, const void *y, int64_t y_ld,
                                     const void *z, int64_t z_ld, const float *w, float eps, void *out, int64_t out_ld,
                                     float *rstd, void *stream) {
  CUM_REQUIRE(dtype_ok(dtype) && rows >= 0 && dim >= 1 && dim <= 8192, "cum_gated_rmsnorm_fwd: bad shape / dtype");
  CUM_REQUIRE(y && z && w && out, "cum_gated_rmsnorm_fwd: null pointer");
  if (rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int blocks = (int)cdiv64(rows, 4);
  if (dtype == CUM_F32)
    gnorm_fwd_kernel<float><<<blocks, 256, 0, st>>>(rows, dim, y, y_ld, z, z_ld, w, eps, out, out_ld, rstd);
  else if (dtype == CUM_BF16)
    gnorm_fwd_kernel<__bf16><<<blocks, 256, 0, st>>>(rows, dim, y, y_ld, z, z_ld, w, eps, out, out_ld, rstd);
  else
    gnorm_fwd_kernel<f16><<<blocks, 256, 0, st>>>(rows, dim, y, y_ld, z, z_ld, w, eps, out, out_ld, rstd);
  CUM_CHECK_LAUNCH();
  return 0;
}

static constexpr int kGnormBwdBlocks = 256;

extern "C" int64_t cum_gated_rmsnorm_bwd_workspace_elems(int32_t dim) { return (int64_t)kGnormBwdBlocks * dim; }

extern "C" int cum_gated_rmsnorm_bwd(int32_t dtype, int64_t rows, int32_t dim, const void *y, int64_t y_ld,
                                     const void *z, int64_t z_ld, const float *w, const float *rstd, const void *dout,
                                     int64_t d_ld, void *dy, int64_t dy_ld, void *dz, int64_t dz_ld, float *dw,
                                     float *workspace, void *stream) {
  CUM_REQUIRE(dtype_ok(dtype) && rows >= 0 && dim >= 1 && dim <= 4096, "cum_gated_rmsnorm_bwd: bad shape / dtype");
  CUM_REQUIRE(y && z && w && rstd && dout && dy && dz && dw && workspace, "cum_gated_rmsnorm_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int64_t per = rows == 0 ? 1 : cdiv64(rows, kGnormBwdBlocks);
  const int blocks = rows == 0 ? 0 : (int)cdiv64(rows, per);
  const size_t lds = 4 * (size_t)dim * sizeof(float);
  if (blocks > 0) {
    if (dtype == CUM_F32)
      gnorm_bwd_kernel<float><<<blocks, 256, lds, st>>>(rows, dim, per, y, y_ld, z, z_ld, w, rstd, dout, d_ld, dy, dy_ld,
                                                        dz, dz_ld, workspace);
    else if (dtype == CUM_BF16)
      gnorm_bwd_kernel<__bf16><<<blocks, 256, lds, st>>>(rows, dim, per, y, y_ld, z, z_ld, w, rstd, dout, d_ld, dy,
                                                         dy_ld, dz, dz_ld, workspace);
    else
      gnorm_bwd_kernel<f16><<<blocks, 256, lds, st>>>(rows, dim, per, y, y_ld, z, z_ld, w, rstd, dout, d_ld, dy, dy_ld,
                                                      dz, dz_ld, workspace);
  }
  gnorm_dw_reduce_kernel<<<(int)cdiv64(dim, 256), 256, 0, st>>>(workspace, blocks, dim, dw);
  CUM_CHECK_LAUNCH();
  return 0;
}

extern "C" int cum_ssd_step(int32_t streams, int32_t d_ssm, int32_t nheads, int32_t dstate, int32_t width, float eps,
                            const float *zxbcdt, int64_t ld, float *conv_state, const float *conv_w,
                            const float *conv_b, const float *dt_bias, const float *A_log, const float *D,
                            const float *norm_w, float *ssm_state, float *out, int64_t out_ld, void *stream) {
  CUM_REQUIRE(streams >= 0 && nheads >= 1 && d_ssm % nheads == 0 && d_ssm <= kStepMaxSsm &&
                  (dstate == 16 || dstate == 32 || dstate == 64) && width >= 1 && width <= 8,
              "cum_ssd_step: unsupported shape");
  const int headdim = d_ssm / nheads;
  CUM_REQUIRE(headdim == 16 || headdim == 32 || headdim == 64, "cum_ssd_step: headdim must be 16, 32 or 64");
  CUM_REQUIRE(ld >= d_ssm + (d_ssm + 2 * dstate) + nheads && out_ld >= d_ssm, "cum_ssd_step: row pitch too small");
  CUM_REQUIRE(zxbcdt && conv_state && conv_w && dt_bias && A_log && D && norm_w && ssm_state && out,
              "cum_ssd_step: null pointer");
  if (streams == 0) return 0;
  Ssd2StepArgs a;
  a.streams = streams; a.d_ssm = d_ssm; a.nheads = nheads; a.headdim = headdim; a.dstate = dstate; a.width = width;
  a.eps = eps; a.zxbcdt = zxbcdt; a.ld = ld; a.conv_state = conv_state; a.conv_w = conv_w; a.conv_b = conv_b;
  a.dt_bias = dt_bias; a.A_log = A_log; a.D = D; a.norm_w = norm_w; a.ssm_state = ssm_state; a.out = out;
  a.out_ld = out_ld;
  ssd_step_kernel<<<streams, 256, 0, (hipStream_t)stream>>>(a);
  CUM_CHECK_LAUNCH();
  return 0;
}
