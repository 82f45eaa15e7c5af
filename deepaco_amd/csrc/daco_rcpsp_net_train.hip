// daco_rcpsp_net_train.hip -- the heuristic network of rcpsp/net.py in TRAINING mode (gnn.BatchNorm on the statistics of each
// project), forward and backward, on the dense relation form of daco_rcpsp_net.hip: B projects of equal n, one workgroup of
// 512 threads per project, ONE launch per direction (+ one small launch that adds the B per-project gradient blocks in ascending
// b).  No cooperative launch, no grid barrier, no atomics.  This file holds the `saved` and workspace layouts, the reductions,
// the training layer, the backward and the entry points; the parameter block's layout, the LDS carve (with its float64
// reduction block and row counts), the device helpers that the forward shares with the eval-mode kernel (input linears, row and
// column compaction, node linears, head) and the host side's refusals are in daco_rcpsp_net.h.
//
// ---- parameter block: the layout of daco_rcpsp_net.h with gamma | beta in the BatchNorm slots (bn_v, then bn_e).  The
// gradient block has the same layout, d/dgamma and d/dbeta in those slots.
//
// ---- `saved`, per project (floats; the per-project stride is rounded up to 256 bytes), written by the forward, read-only to
// the backward:
//   w  [13][n][n][32]   the edge state entering layer l (l = 12: the head's input); slots off the graph are never touched
//   ze [12][n][n][32]   the edge BatchNorm's input  We w + be + x3[i] + x4[j]
//   xs [12][n][32]      the node state entering layer l
//   zv [12][n][32]      the node BatchNorm's input  x1[i] + mean_j sigmoid(w_ij) x2[j]
//   bn [12][2 (edge, node)][32][2 (mean, rstd)]
// = (25 n^2 + 24 n) * 128 B + 6 KB: 50.4 MB at n = 128, 2.8 MB at n = 30.  Nothing is recomputed but X = xs WvT + bv (a
// 64 KB LDS block per layer) and the head's two hidden layers.
//
// ---- forward, a layer = two walks over the rows with a workgroup reduction between them
//   walk 1: ze (stored), the gate sums, zv (stored); per (wavefront, half) float64 partial sums of ze, ze^2 (and zv, zv^2)
//   reduction: the 16 partials of a channel through LDS, added in slot order 0..15 in float64 by every thread; mean = S1 / E,
//     biased var = S2 / E - mean^2, rstd = 1 / sqrt(var + 1e-5), rounded to float32 once
//   walk 2: w' = w + silu(gamma (ze - mean) rstd + beta); x' = x + silu(the same of zv)
// A partial is a sequential sum over the slot's rows and edges in ascending order, so every sum depends on the project alone.
//
// ---- backward: head, then the layers in reverse.  State in the workspace (per project): gw [n][n][32] (in place), gze
// [n][n][32], gX [n][128], gxs [n][32], the 16 slots' partial weight gradients, and the project's gradient block.
//   node A : g_y = gxs silu'(y); S1 = sum g_y, S2 = sum g_y zhat (float64, slot order); g_zv -> gX[:, 0:32]
//   edge 1 : row walk, g_y = gw silu'(y): S1, S2 as above over the E edges
//   edge 2 : row walk, g_ze = gamma rstd (g_y - S1/E - zhat S2/E) -> gze; gw <- gw + We^T g_ze + g_agg[i] x2[j] sigmoid'(w) /
//            count_i; gWe (a lane holds row o: 32 accumulators), gbe, row sums -> gX[:, 64:96]
//   edge 3 : COLUMN walk (a wavefront owns a column, rows ascending, even + odd): sum_i gze -> gX[:, 96:128], sum_i g_agg[i]
//            sigmoid(w_ij) / count_i -> gX[:, 32:64].  No atomics: the order is fixed.
//   node B : gWvT = xs^T gX, gbv, gxs += gX WvT^T
// then v_lin0, e_lin0 (three per-code sums of gw through silu') -- plain f32 FMAs, a lane per channel, as the forward.
#include "daco_rcpsp_net.h"

namespace daco {
namespace {

constexpr double RT_BN_EPS = 1e-5;

// per-project pieces of `saved` and of the backward's workspace (floats)
struct RtSaved {
  size_t n2, nu;
  __host__ __device__ explicit RtSaved(int n) : n2((size_t)n * n * 32), nu((size_t)n * 32) {}
  __host__ __device__ size_t w(int l) const { return (size_t)l * n2; }
  __host__ __device__ size_t ze(int l) const { return (size_t)(RN_DEPTH + 1 + l) * n2; }
  __host__ __device__ size_t xs(int l) const { return (2 * RN_DEPTH + 1) * n2 + (size_t)l * nu; }
  __host__ __device__ size_t zv(int l) const { return (2 * RN_DEPTH + 1) * n2 + (size_t)(RN_DEPTH + l) * nu; }
  __host__ __device__ size_t bn(int l) const { return (2 * RN_DEPTH + 1) * n2 + 2 * RN_DEPTH * nu + (size_t)l * 128; }
  __host__ __device__ size_t floats() const { return bn(RN_DEPTH); }
  __host__ __device__ size_t stride_bytes() const { return align256(floats() * sizeof(float)); }
};
struct RtWork {
  size_t n2, n;
  __host__ __device__ explicit RtWork(int n_) : n2((size_t)n_ * n_ * 32), n((size_t)n_) {}
  __host__ __device__ size_t gw() const { return 0; }
  __host__ __device__ size_t gze() const { return n2; }
  __host__ __device__ size_t gX() const { return 2 * n2; }
  __host__ __device__ size_t gxs() const { return 2 * n2 + n * 128; }
  __host__ __device__ size_t part() const { return 2 * n2 + n * 160; }                  // [2][16][1024]
  __host__ __device__ size_t block() const { return part() + 2 * RN_SLOTS * 1024; }
  __host__ __device__ size_t floats() const { return block() + RN_PARAM_FLOATS; }
  __host__ __device__ size_t stride_bytes() const { return align256(floats() * sizeof(float)); }
};

// acc[c] += g * st[c]: the outer product row this lane owns
__device__ inline void rt_outer32(const float *st, float g, float (&acc)[32]) {
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float4 v = *reinterpret_cast<const float4 *>(st + q * 4);
    acc[q * 4 + 0] = fmaf(g, v.x, acc[q * 4 + 0]);
    acc[q * 4 + 1] = fmaf(g, v.y, acc[q * 4 + 1]);
    acc[q * 4 + 2] = fmaf(g, v.z, acc[q * 4 + 2]);
    acc[q * 4 + 3] = fmaf(g, v.w, acc[q * 4 + 3]);
  }
}

// Two sums over the workgroup per channel o = tid & 31: the partials of the 16 slots (tid >> 5), added in slot order by every
// thread.  Called by all 512 threads.
__device__ inline void rt_reduce2(double *red, double &a, double &b) {
  const int slot = threadIdx.x >> 5, o = threadIdx.x & 31;
  red[(slot * 32 + o) * 2 + 0] = a;
  red[(slot * 32 + o) * 2 + 1] = b;
  __syncthreads();
  double sa = 0.0, sb = 0.0;
  for (int s = 0; s < RN_SLOTS; ++s) {
    sa += red[(s * 32 + o) * 2 + 0];
    sb += red[(s * 32 + o) * 2 + 1];
  }
  __syncthreads();
  a = sa;
  b = sb;
}

// the 16 slots' partial [32][32] matrices (part [16][1024], global) added in slot order into dst [1024]; between barriers
__device__ inline void rt_reduce_matrix(const float *part, float *dst) {
  for (int e = threadIdx.x; e < 1024; e += RN_THREADS) {
    float acc = 0.0f;
    for (int s = 0; s < RN_SLOTS; ++s) acc += part[s * 1024 + e];
    dst[e] = acc;
  }
}

// relation codes, the rows' edge counts, silu(e_lin0(attr)) for the three attribute rows; returns E.  Ends behind a barrier.
__device__ inline int rt_load_graph(const RnLds &s, int n, const uint8_t *relation, const float *params) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  rn_load_relation(s, n, relation);
  rn_edge_init(s, params);
  __syncthreads();
  for (int i = wave; i < n; i += RN_WAVES) {
    const uint8_t *rrow = s.rel + i * n;
    const int c0 = lane < n ? rrow[lane] : 0, c1 = lane + 64 < n ? rrow[lane + 64] : 0;
    const int cnt = __popcll(__ballot(c0 != 0)) + __popcll(__ballot(c1 != 0));
    if (lane == 0) s.rowcnt[i] = cnt;
  }
  __syncthreads();
  int E = 0;
  for (int i = 0; i < n; ++i) E += s.rowcnt[i];
  return E;
}

// ------------------------------------------------------------------------------------------------ forward
__device__ inline void rt_fwd_layer(const RnLds &s, int n, int E, const float *__restrict__ wl, float *__restrict__ wnext,
                                    float *__restrict__ ze, float *__restrict__ xs_save, float *__restrict__ zv_save,
                                    float *__restrict__ bn_save, float *__restrict__ stats_e, float *__restrict__ stats_v) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, o = lane & 31;
  const float *We = s.W + RN_L_WE;
  float wr[32];
#pragma unroll
  for (int c = 0; c < 32; ++c) wr[c] = We[o * 32 + c];
  const float beo = s.W[RN_L_BE + o];
  const float gv = s.W[RN_L_BNV + o], bv = s.W[RN_L_BNV + 32 + o], ge = s.W[RN_L_BNE + o], bbe = s.W[RN_L_BNE + 32 + o];
  float *st = s.stage + (wave * 2 + h) * 96;
  uint8_t *cols = s.cols + wave * 128;
  for (int t = tid; t < n * 32; t += RN_THREADS) xs_save[t] = s.xs[t];
  double s1 = 0.0, s2 = 0.0, v1 = 0.0, v2 = 0.0;
  for (int i = wave; i < n; i += RN_WAVES) {
    const uint8_t *rrow = s.rel + i * n;
    const int cnt = rn_compact(rrow, 1, n, cols, lane);
    const float *wrow = wl + (size_t)i * n * 32;
    float *zrow = ze + (size_t)i * n * 32;
    const float x3 = s.X[i * 128 + 64 + o];
    float part = 0.0f;
    for (int k0 = h; k0 < cnt; k0 += 8) {                 // four edges of this half per step, their loads issued together
      float w0[4];
      int jj[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = k0 + 2 * q;
        jj[q] = k < cnt ? cols[k] : -1;
        w0[q] = jj[q] >= 0 ? wrow[jj[q] * 32 + o] : 0.0f;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (jj[q] >= 0) {
          const int j = jj[q];
          st[o] = w0[q];
          const float g = rn_dot32(st, wr);
          part = fmaf(sigmoidf(w0[q]), s.X[j * 128 + 32 + o], part);
          const float z = g + beo + x3 + s.X[j * 128 + 96 + o];
          zrow[j * 32 + o] = z;
          s1 += (double)z;
          s2 += (double)z * (double)z;
        }
      }
    }
    const float agg = (part + __shfl_xor(part, 32)) / (float)max(cnt, 1);
    if (h == 0) {
      const float zv = s.X[i * 128 + o] + agg;
      zv_save[i * 32 + o] = zv;
      v1 += (double)zv;
      v2 += (double)zv * (double)zv;
    }
  }
  rt_reduce2(s.red, s1, s2);
  rt_reduce2(s.red, v1, v2);
  const double me = s1 / (double)max(E, 1), vare = fmax(s2 / (double)max(E, 1) - me * me, 0.0);
  const double mv = v1 / (double)n, varv = fmax(v2 / (double)n - mv * mv, 0.0);
  const float mean_e = (float)me, rstd_e = (float)(1.0 / sqrt(vare + RT_BN_EPS));
  const float mean_v = (float)mv, rstd_v = (float)(1.0 / sqrt(varv + RT_BN_EPS));
  if (tid < 32) {
    stats_e[o * 2 + 0] = mean_e; stats_e[o * 2 + 1] = (float)vare;
    stats_v[o * 2 + 0] = mean_v; stats_v[o * 2 + 1] = (float)varv;
    bn_save[o * 2 + 0] = mean_e; bn_save[o * 2 + 1] = rstd_e;
    bn_save[64 + o * 2 + 0] = mean_v; bn_save[64 + o * 2 + 1] = rstd_v;
  }
  // walk 2 (the barriers of the reductions made every ze and zv of walk 1 visible)
  for (int i = wave; i < n; i += RN_WAVES) {
    const uint8_t *rrow = s.rel + i * n;
    const int cnt = rn_compact(rrow, 1, n, cols, lane);
    const size_t row = (size_t)i * n * 32;
#pragma unroll 4
    for (int k = h; k < cnt; k += 2) {
      const size_t at = row + cols[k] * 32 + o;
      const float y = fmaf((ze[at] - mean_e) * rstd_e, ge, bbe);
      wnext[at] = wl[at] + silu(y);
    }
  }
  for (int t = tid; t < n * 32; t += RN_THREADS) {          // t & 31 == o
    const float y = fmaf((zv_save[t] - mean_v) * rstd_v, gv, bv);
    s.xs[t] += silu(y);
  }
}

__global__ void __launch_bounds__(RN_THREADS)
rcpsp_net_train_forward_kernel(int B, int n, const float *x, const uint8_t *relation, const float *params, float eps, float *heu,
                               float *logit, float *stats, float *saved_base, size_t saved_stride) {
  extern __shared__ __attribute__((aligned(16))) float rt_lds[];
  const RnLds s = RnLds::carve(rt_lds, n, true);
  const RtSaved sv(n);
  const int b = blockIdx.x, tid = threadIdx.x;
  x += (size_t)b * n * RN_FEATS;
  relation += (size_t)b * n * n;
  heu += (size_t)b * n * n;
  if (logit) logit += (size_t)b * n * n;
  float *saved = saved_base + (size_t)b * saved_stride;

  const int E = rt_load_graph(s, n, relation, params);
  rn_load_floats(s.W, params + RN_OFF_LAYER0, LAYER_FLOATS);
  rn_input_nodes(s, n, x, params);
  {                                                     // w of layer 0: one of the three initial vectors
    float *w0 = saved + sv.w(0);
    const int o = tid & 31;
    for (int t = tid >> 5; t < n * n; t += RN_THREADS / 32) {
      const int c = s.rel[t];
      if (c) w0[(size_t)t * 32 + o] = s.e0[(c - 1) * 32 + o];
    }
  }
  __syncthreads();
  rn_node_linears(s, n);
  __syncthreads();
  for (int l = 0; l < RN_DEPTH; ++l) {
    float *st_e = stats + ((((size_t)l * 2 + 0) * B + b) * 32) * 2, *st_v = stats + ((((size_t)l * 2 + 1) * B + b) * 32) * 2;
    rt_fwd_layer(s, n, E, saved + sv.w(l), saved + sv.w(l + 1), saved + sv.ze(l), saved + sv.xs(l), saved + sv.zv(l),
                 saved + sv.bn(l), st_e, st_v);
    __syncthreads();
    if (l < RN_DEPTH - 1) {
      rn_load_floats(s.W, params + RN_OFF_LAYER0 + (size_t)(l + 1) * LAYER_FLOATS, LAYER_FLOATS);
      __syncthreads();
      rn_node_linears(s, n);
    } else {
      rn_load_floats(s.W, params + RN_OFF_HEAD, HEAD_FLOATS);
    }
    __syncthreads();
  }
  rn_head(s, n, saved + sv.w(RN_DEPTH), eps, heu, logit, nullptr);
}

// ------------------------------------------------------------------------------------------------ backward
// head, in two row walks so that neither holds more than four 32-float register arrays:
//   A: recompute the two hidden layers per edge; gW2, gb2, gW3, gb3, gb1; g_h1 (the gradient at the first layer's
//      pre-activation) -> gh1 [n][n][32] (the gze block, free until the first layer of the reverse walk)
//   B: gW1 += g_h1 (x) w, gw <- W1^T g_h1
__device__ inline void rt_bwd_head(const RnLds &s, int n, const float *__restrict__ w, const float *__restrict__ gheu,
                                   float *__restrict__ gw, float *__restrict__ gh1buf, float *__restrict__ part,
                                   float *__restrict__ gblock) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, o = lane & 31, slot = tid >> 5;
  const float *W1 = s.W, *W2 = s.W + RN_H_W2, *W3 = s.W + RN_H_W3;
  float *st = s.stage + slot * 96;
  uint8_t *cols = s.cols + wave * 128;
  double gb1 = 0.0, gb2 = 0.0, gw3 = 0.0, gb3 = 0.0;
  {
    float w1r[32], w2r[32], w2c[32], acc[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) {
      w1r[c] = W1[o * 32 + c]; w2r[c] = W2[o * 32 + c]; w2c[c] = W2[c * 32 + o];
      acc[c] = 0.0f;
    }
    const float b1o = s.W[RN_H_B1 + o], b2o = s.W[RN_H_B2 + o], b3v = s.W[RN_H_B3], w3o = W3[o];
    for (int i = wave; i < n; i += RN_WAVES) {
      const uint8_t *rrow = s.rel + i * n;
      const int cnt = rn_compact(rrow, 1, n, cols, lane);
      const size_t row = (size_t)i * n * 32;
      for (int k = h; k < cnt; k += 2) {
        const int j = cols[k];
        const float wv = w[row + j * 32 + o];
        const float gh = gheu[i * n + j];
        st[o] = wv;
        const float h1 = rn_dot32(st, w1r) + b1o;
        const float a1 = silu(h1);
        st[32 + o] = a1;
        const float h2 = rn_dot32(st + 32, w2r) + b2o;
        const float a2 = silu(h2);
        st[64 + o] = a2;
        float sum = 0.0f;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const float4 v = *reinterpret_cast<const float4 *>(st + 64 + q * 4);
          const float4 u = *reinterpret_cast<const float4 *>(W3 + q * 4);
          sum = fmaf(v.x, u.x, sum); sum = fmaf(v.y, u.y, sum); sum = fmaf(v.z, u.z, sum); sum = fmaf(v.w, u.w, sum);
        }
        const float sz = sigmoidf(sum + b3v);
        const float gz = gh * (sz * (1.0f - sz));
        gw3 += (double)(gz * a2);
        gb3 += (double)gz;
        const float gh2 = gz * w3o * dsilu(h2);
        gb2 += (double)gh2;
        rt_outer32(st + 32, gh2, acc);                   // gW2[o][c] += gh2[o] a1[c]
        st[64 + o] = gh2;
        const float ga1 = rn_dot32(st + 64, w2c);         // sum_o' gh2[o'] W2[o'][o]
        const float gh1 = ga1 * dsilu(h1);
        gb1 += (double)gh1;
        gh1buf[row + j * 32 + o] = gh1;
      }
    }
#pragma unroll
    for (int c = 0; c < 32; ++c) part[(RN_SLOTS + slot) * 1024 + o * 32 + c] = acc[c];
  }
  {
    float w1c[32], acc[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) { w1c[c] = W1[c * 32 + o]; acc[c] = 0.0f; }
    for (int i = wave; i < n; i += RN_WAVES) {           // the rows this wavefront wrote in walk A
      const uint8_t *rrow = s.rel + i * n;
      const int cnt = rn_compact(rrow, 1, n, cols, lane);
      const size_t row = (size_t)i * n * 32;
#pragma unroll 2
      for (int k = h; k < cnt; k += 2) {
        const size_t at = row + cols[k] * 32 + o;
        const float gh1 = gh1buf[at];
        st[o] = w[at];
        rt_outer32(st, gh1, acc);                        // gW1[o][c] += gh1[o] w[c]
        st[32 + o] = gh1;
        gw[at] = rn_dot32(st + 32, w1c);
      }
    }
#pragma unroll
    for (int c = 0; c < 32; ++c) part[slot * 1024 + o * 32 + c] = acc[c];
  }
  rt_reduce2(s.red, gb1, gb2);
  rt_reduce2(s.red, gw3, gb3);
  float *gh = gblock + RN_OFF_HEAD;
  rt_reduce_matrix(part, gh);
  rt_reduce_matrix(part + RN_SLOTS * 1024, gh + RN_H_W2);
  if (tid < 32) {
    gh[RN_H_B1 + o] = (float)gb1;
    gh[RN_H_B2 + o] = (float)gb2;
    gh[RN_H_W3 + o] = (float)gw3;
    if (o == 0) gh[RN_H_B3] = (float)gb3;
  }
}

__device__ inline void rt_bwd_layer(const RnLds &s, int n, int E, const float *__restrict__ wl, const float *__restrict__ ze,
                                    const float *__restrict__ zv, const float *__restrict__ bn, float *__restrict__ gw,
                                    float *__restrict__ gze, float *gX, float *gxs, float *__restrict__ part,
                                    float *__restrict__ gl) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, o = lane & 31, slot = tid >> 5;
  const float gv = s.W[RN_L_BNV + o], bv = s.W[RN_L_BNV + 32 + o], ge = s.W[RN_L_BNE + o], bbe = s.W[RN_L_BNE + 32 + o];
  const float mean_e = bn[o * 2], rstd_e = bn[o * 2 + 1], mean_v = bn[64 + o * 2], rstd_v = bn[64 + o * 2 + 1];
  float *st = s.stage + slot * 96;
  uint8_t *cols = s.cols + wave * 128;

  // ---- node A
  {
    double a = 0.0, c = 0.0;
    for (int t = tid; t < n * 32; t += RN_THREADS) {
      const float zh = (zv[t] - mean_v) * rstd_v;
      const float gy = gxs[t] * dsilu(fmaf(zh, gv, bv));
      a += (double)gy;
      c += (double)gy * (double)zh;
    }
    rt_reduce2(s.red, a, c);
    const float m1 = (float)(a / (double)n), m2 = (float)(c / (double)n);
    if (tid < 32) { gl[RN_L_BNV + o] = (float)c; gl[RN_L_BNV + 32 + o] = (float)a; }
    for (int t = tid; t < n * 32; t += RN_THREADS) {
      const float zh = (zv[t] - mean_v) * rstd_v;
      const float gy = gxs[t] * dsilu(fmaf(zh, gv, bv));
      gX[(t >> 5) * 128 + o] = gv * rstd_v * (gy - m1 - zh * m2);
    }
  }
  // ---- edge 1: the two sums of the edge BatchNorm
  double e1 = 0.0, e2 = 0.0;
  for (int i = wave; i < n; i += RN_WAVES) {
    const int cnt = rn_compact(s.rel + i * n, 1, n, cols, lane);
    const size_t row = (size_t)i * n * 32;
#pragma unroll 4
    for (int k = h; k < cnt; k += 2) {
      const size_t at = row + cols[k] * 32 + o;
      const float zh = (ze[at] - mean_e) * rstd_e;
      const float gy = gw[at] * dsilu(fmaf(zh, ge, bbe));
      e1 += (double)gy;
      e2 += (double)gy * (double)zh;
    }
  }
  rt_reduce2(s.red, e1, e2);                              // (its barriers also publish node A's gX)
  const float m1 = (float)(e1 / (double)max(E, 1)), m2 = (float)(e2 / (double)max(E, 1));
  if (tid < 32) { gl[RN_L_BNE + o] = (float)e2; gl[RN_L_BNE + 32 + o] = (float)e1; }
  // ---- edge 2
  {
    const float *We = s.W + RN_L_WE;
    float wcol[32], acc[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) { wcol[c] = We[c * 32 + o]; acc[c] = 0.0f; }
    double gbe = 0.0, unused = 0.0;
    const float scale = ge * rstd_e;
    for (int i = wave; i < n; i += RN_WAVES) {
      const int cnt = rn_compact(s.rel + i * n, 1, n, cols, lane);
      const size_t row = (size_t)i * n * 32;
      const float gagg = gX[i * 128 + o] / (float)max(cnt, 1);
      float rows = 0.0f;
      for (int k0 = h; k0 < cnt; k0 += 8) {
        float zq[4], gq[4], wq[4];
        int jj[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int k = k0 + 2 * q;
          jj[q] = k < cnt ? cols[k] : -1;
          const size_t at = row + (jj[q] >= 0 ? jj[q] : 0) * 32 + o;
          zq[q] = jj[q] >= 0 ? ze[at] : 0.0f;
          gq[q] = jj[q] >= 0 ? gw[at] : 0.0f;
          wq[q] = jj[q] >= 0 ? wl[at] : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (jj[q] >= 0) {
            const int j = jj[q];
            const size_t at = row + j * 32 + o;
            const float zh = (zq[q] - mean_e) * rstd_e;
            const float gy = gq[q] * dsilu(fmaf(zh, ge, bbe));
            const float gz = scale * (gy - m1 - zh * m2);
            gze[at] = gz;
            gbe += (double)gz;
            rows += gz;
            st[o] = gz;
            const float back = rn_dot32(st, wcol);        // sum_o' gz[o'] We[o'][o]
            st[32 + o] = wq[q];
            rt_outer32(st + 32, gz, acc);                 // gWe[o][c] += gz[o] w[c]
            const float sg = sigmoidf(wq[q]);
            gw[at] = gq[q] + back + gagg * s.X[j * 128 + 32 + o] * (sg * (1.0f - sg));
          }
        }
      }
      const float tot = rows + __shfl_xor(rows, 32);
      if (h == 0) gX[i * 128 + 64 + o] = tot;
    }
#pragma unroll
    for (int c = 0; c < 32; ++c) part[slot * 1024 + o * 32 + c] = acc[c];
    rt_reduce2(s.red, gbe, unused);
    if (tid < 32) gl[RN_L_BE + o] = (float)gbe;
    rt_reduce_matrix(part, gl + RN_L_WE);
  }
  // ---- edge 3: the column sums (gze and gX[:, 0:32] are complete behind the barriers above)
  for (int j = wave; j < n; j += RN_WAVES) {
    const int cnt = rn_compact(s.rel + j, n, n, cols, lane);
    float a4 = 0.0f, a2 = 0.0f;
#pragma unroll 4
    for (int k = h; k < cnt; k += 2) {
      const int i = cols[k];
      const size_t at = ((size_t)i * n + j) * 32 + o;
      a4 += gze[at];
      a2 = fmaf(gX[i * 128 + o] / (float)max(s.rowcnt[i], 1), sigmoidf(wl[at]), a2);
    }
    a4 += __shfl_xor(a4, 32);
    a2 += __shfl_xor(a2, 32);
    if (h == 0) { gX[j * 128 + 96 + o] = a4; gX[j * 128 + 32 + o] = a2; }
  }
  __syncthreads();
  // ---- node B
  {
    const int col = tid & 127, cg = tid >> 7;
    float acc[8], sum = 0.0f;
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.0f;
    for (int i = 0; i < n; ++i) {
      const float g = gX[i * 128 + col];
      sum += g;
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[q] = fmaf(s.xs[i * 32 + cg * 8 + q], g, acc[q]);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) gl[(cg * 8 + q) * 128 + col] = acc[q];
    if (cg == 0) gl[RN_L_BV + col] = sum;
    for (int t = tid; t < n * 32; t += RN_THREADS) {
      const int i = t >> 5;
      float a = 0.0f;
      for (int k = 0; k < 128; ++k) {
        const int c2 = (k + o) & 127;                     // rotated by the channel: the lanes of a row read 32 different banks
        a = fmaf(gX[i * 128 + c2], s.W[o * 128 + c2], a);
      }
      gxs[t] += a;
    }
  }
}

__global__ void __launch_bounds__(RN_THREADS)
rcpsp_net_train_backward_kernel(int n, const float *x, const uint8_t *relation, const float *params, const float *saved_base,
                                size_t saved_stride, const float *gheu, float *work_base, size_t work_stride) {
  extern __shared__ __attribute__((aligned(16))) float rt_lds[];
  const RnLds s = RnLds::carve(rt_lds, n, true);
  const RtSaved sv(n);
  const RtWork wk(n);
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, o = lane & 31, slot = tid >> 5;
  x += (size_t)b * n * RN_FEATS;
  relation += (size_t)b * n * n;
  gheu += (size_t)b * n * n;
  const float *saved = saved_base + (size_t)b * saved_stride;
  float *work = work_base + (size_t)b * work_stride;
  float *gw = work + wk.gw(), *gze = work + wk.gze(), *gX = work + wk.gX(), *gxs = work + wk.gxs(), *part = work + wk.part();
  float *gblock = work + wk.block();

  const int E = rt_load_graph(s, n, relation, params);
  rn_load_floats(s.W, params + RN_OFF_HEAD, HEAD_FLOATS);
  for (int t = tid; t < n * 32; t += RN_THREADS) gxs[t] = 0.0f;          // nothing reads the node state after the last layer
  __syncthreads();
  rt_bwd_head(s, n, saved + sv.w(RN_DEPTH), gheu, gw, gze, part, gblock);
  __syncthreads();
  for (int l = RN_DEPTH - 1; l >= 0; --l) {
    rn_load_floats(s.W, params + RN_OFF_LAYER0 + (size_t)l * LAYER_FLOATS, LAYER_FLOATS);
    rn_load_floats(s.xs, saved + sv.xs(l), n * 32);
    __syncthreads();
    rn_node_linears(s, n);
    __syncthreads();
    rt_bwd_layer(s, n, E, saved + sv.w(l), saved + sv.ze(l), saved + sv.zv(l), saved + sv.bn(l), gw, gze, gX, gxs, part,
                 gblock + RN_OFF_LAYER0 + (size_t)l * LAYER_FLOATS);
    __syncthreads();
  }
  // ---- v_lin0: x0 = silu(W x + b)
  {
    const float *W = params, *bb = params + 32 * RN_FEATS;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = slot; i < n; i += RN_SLOTS) {
      float v = bb[o];
#pragma unroll
      for (int f = 0; f < RN_FEATS; ++f) v = fmaf(x[i * RN_FEATS + f], W[o * RN_FEATS + f], v);
      const float gp = gxs[i * 32 + o] * dsilu(v);
#pragma unroll
      for (int f = 0; f < RN_FEATS; ++f) acc[f] += (double)(gp * x[i * RN_FEATS + f]);
      acc[5] += (double)gp;
    }
    rt_reduce2(s.red, acc[0], acc[1]);
    rt_reduce2(s.red, acc[2], acc[3]);
    rt_reduce2(s.red, acc[4], acc[5]);
    if (tid < 32) {
#pragma unroll
      for (int f = 0; f < RN_FEATS; ++f) gblock[o * RN_FEATS + f] = (float)acc[f];
      gblock[32 * RN_FEATS + o] = (float)acc[5];
    }
  }
  // ---- e_lin0: w0 = silu(e_lin0(attr of the code)): three per-code sums of gw
  {
    double c0 = 0.0, c1 = 0.0, c2 = 0.0, unused = 0.0;
    uint8_t *cols = s.cols + wave * 128;
    for (int i = wave; i < n; i += RN_WAVES) {
      const uint8_t *rrow = s.rel + i * n;
      const int cnt = rn_compact(rrow, 1, n, cols, lane);
      const size_t row = (size_t)i * n * 32;
#pragma unroll 4
      for (int k = h; k < cnt; k += 2) {
        const int j = cols[k], code = rrow[j];
        const double g = (double)gw[row + j * 32 + o];
        c0 += code == 1 ? g : 0.0;
        c1 += code == 2 ? g : 0.0;
        c2 += code == 3 ? g : 0.0;
      }
    }
    rt_reduce2(s.red, c0, c1);
    rt_reduce2(s.red, c2, unused);
    if (tid < 32) {
      const float *W = params + RN_OFF_ELIN, *bb = W + 64;
      const float p0 = fmaf(0.0f, W[o * 2 + 1], fmaf(1.0f, W[o * 2 + 0], bb[o]));
      const float p1 = fmaf(1.0f, W[o * 2 + 1], fmaf(0.0f, W[o * 2 + 0], bb[o]));
      const float p2 = bb[o];
      const float g0 = (float)c0 * dsilu(p0), g1 = (float)c1 * dsilu(p1), g2 = (float)c2 * dsilu(p2);
      float *ge0 = gblock + RN_OFF_ELIN;
      ge0[o * 2 + 0] = g0;
      ge0[o * 2 + 1] = g1;
      ge0[64 + o] = g0 + g1 + g2;
    }
  }
}

// grad[p] = sum over b ascending of the per-project blocks
__global__ void rcpsp_net_train_sum_kernel(int B, const float *work_base, size_t work_stride, size_t block_off, float *grad,
                                           float *blocks) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= RN_PARAM_FLOATS) return;
  float acc = 0.0f;
  for (int b = 0; b < B; ++b) {
    const float v = work_base[(size_t)b * work_stride + block_off + p];
    if (blocks) blocks[(size_t)b * RN_PARAM_FLOATS + p] = v;
    acc += v;
  }
  grad[p] = acc;
}

}  // namespace
}  // namespace daco

using namespace daco;

extern "C" size_t daco_rcpsp_net_train_saved_bytes(int B, int n) {
  if (!rn_sizes_ok(B, n)) return 0;
  return (size_t)B * RtSaved(n).stride_bytes();
}

extern "C" size_t daco_rcpsp_net_train_workspace_bytes(int B, int n) {
  if (!rn_sizes_ok(B, n)) return 0;
  return (size_t)B * RtWork(n).stride_bytes();
}

extern "C" long daco_rcpsp_net_train_forward(void *stream, int B, int n, int feats, const float *x, const uint8_t *relation,
                                             const float *params, float eps, float *heu, float *logit, float *stats,
                                             void *saved, size_t saved_bytes) {
  const char *who = "daco_rcpsp_net_train_forward";
  if (const long rc = rn_check(who, B, n, feats, x && relation && params && heu && stats && saved, true)) return rc;
  const size_t need = daco_rcpsp_net_train_saved_bytes(B, n);
  if (saved_bytes < need) {
    set_error("%s: saved %zu < %zu bytes", who, saved_bytes, need);
    return DACO_E_WORKSPACE;
  }
  const size_t dyn = RnLds::bytes(n, true);
  if (const long rc = rn_lds_attr(rcpsp_net_train_forward_kernel, dyn, "rcpsp_net_train_forward_kernel (dynamic LDS)")) return rc;
  hipLaunchKernelGGL(rcpsp_net_train_forward_kernel, dim3((unsigned)B), dim3(RN_THREADS), dyn, (hipStream_t)stream, B, n, x,
                     relation, params, eps, heu, logit, stats, (float *)saved, need / B / sizeof(float));
  return launch_status("rcpsp_net_train_forward_kernel");
}

extern "C" long daco_rcpsp_net_train_backward(void *stream, int B, int n, int feats, const float *x, const uint8_t *relation,
                                              const float *params, const void *saved, size_t saved_bytes, const float *grad_heu,
                                              float *grad_params, float *grad_blocks, void *workspace, size_t workspace_bytes) {
  const char *who = "daco_rcpsp_net_train_backward";
  if (const long rc = rn_check(who, B, n, feats, x && relation && params && saved && grad_heu && grad_params && workspace, true)) return rc;
  const size_t need_s = daco_rcpsp_net_train_saved_bytes(B, n), need_w = daco_rcpsp_net_train_workspace_bytes(B, n);
  if (saved_bytes < need_s) {
    set_error("%s: saved %zu < %zu bytes", who, saved_bytes, need_s);
    return DACO_E_WORKSPACE;
  }
  if (workspace_bytes < need_w) {
    set_error("%s: workspace %zu < %zu bytes", who, workspace_bytes, need_w);
    return DACO_E_WORKSPACE;
  }
  const size_t dyn = RnLds::bytes(n, true);
  if (const long rc = rn_lds_attr(rcpsp_net_train_backward_kernel, dyn, "rcpsp_net_train_backward_kernel (dynamic LDS)")) return rc;
  const size_t wstride = need_w / B / sizeof(float);
  hipLaunchKernelGGL(rcpsp_net_train_backward_kernel, dim3((unsigned)B), dim3(RN_THREADS), dyn, (hipStream_t)stream, n, x, relation,
                     params, (const float *)saved, need_s / B / sizeof(float), grad_heu, (float *)workspace, wstride);
  if (const long rc = launch_status("rcpsp_net_train_backward_kernel")) return rc;
  hipLaunchKernelGGL(rcpsp_net_train_sum_kernel, dim3((RN_PARAM_FLOATS + 255) / 256), dim3(256), 0, (hipStream_t)stream, B,
                     (const float *)workspace, wstride, RtWork(n).block(), grad_params, grad_blocks);
  return launch_status("rcpsp_net_train_sum_kernel");
}
