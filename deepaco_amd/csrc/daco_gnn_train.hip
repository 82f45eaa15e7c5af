// daco_gnn_train.hip -- heuristic network, TRAINING mode: forward with per-graph batch statistics and the full
// backward, both as HIP kernels (no library GEMM anywhere).
//
// Reference behaviour replaced: EmbNet.forward tsp/net.py:27-45 with BatchNorm in training mode (the statistics
// of the ONE graph being trained on, :21,24,43-44), MLP/ParNet.forward :59-75, and what autograd derives from
// them for tsp_nls/train.py:15-44 (loss.backward()).  G equal-sized graphs may be laid side by side (n = G*n_g
// nodes, E = G*E_g edges, node ids offset per graph): every graph normalises with its own statistics, exactly as G
// separate reference forwards would.  The *_ragged entries take G graphs of equal node count whose edge counts differ (sop/:
// the graph is nonzero(adj)): graph g owns edges [edge_off[g], edge_off[g+1]) and normalises over its own count.
//
// Per layer (x [n,32], w [E,32]):
//   X = x Wv^T + bv = (x1|x2|x3|x4)                     node_post of the previous layer (MFMA-free: n is small)
//   ze = w We^T + be + x3[src] + x4[dst]                edge_pre   (MFMA 32x32x2 f32 tile GEMM) + sum, sum^2 per channel
//   zv = x1 + mean_{e: src=i} sigmoid(w_e) * x2[dst_e]  node_pre   (CSR gather, no atomics)   + sum, sum^2 per channel
//   w' = w + silu(bn_e(ze)),  x' = x + silu(bn_v(zv))   edge_post / node_post (batch statistics, biased variance)
// The channel sums are accumulated in f64 (tile-wise partial sums, then one hardware f64 atomic per channel), so the
// mean/variance do not depend on the summation order beyond f64 rounding.
// Saved for the backward: x, X, w, ze, zv of every layer (n, E are training-sized: TSP-500, k = 50 is 3.2 MB per
// edge tensor).  The backward walks the layers in reverse:
//   edge_bwd_stats / node_bwd_stats   sum(g_y), sum(g_y * zhat) per channel (the two BatchNorm reductions)
//   node_bwd_apply                    g_zv -> gX[:, x1 block], g_msg = g_zv / degree
//   edge_bwd_main                     g_ze -> gw (in place: residual + g_ze We + gate path), scatter-adds into gX
//                                     (x2, x3, x4 blocks; hardware f32 atomics), gWe += g_ze^T w (MFMA outer products
//                                     accumulated over the tiles a wave walks), gbe
//   node_lin_bwd                      gx (in place: residual + gX Wv), gWv += gX^T x (MFMA), gbv
// Parameter gradients land in a flat block with the layout of the parameter block (see daco_gnn.hip), BatchNorm
// slots holding d/dgamma, d/dbeta.
#include <cstdlib>

#include "daco_gnn.h"
#include "daco_host.h"

namespace daco {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int TU = 32;
constexpr float BN_EPS = 1e-5f;

__device__ inline float t_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + expf(-x)); }
__device__ inline float t_silu(float x) { return x * t_sigmoid(x); }
__device__ inline float t_dsilu(float x) { const float s = t_sigmoid(x); return s * (1.0f + x * (1.0f - s)); }

// D[i][j] += sum_k A[i][k] * B[k][j] over k = 0..31 with v_mfma_f32_32x32x2_f32; lane l supplies A[l%32][k] and
// B[k][l%32] for k = (l/32)*16 + kk.  a(kk) / b(kk) are functors returning those elements.
template <class FA, class FB>
__device__ inline f32x16 mfma32(f32x16 acc, FA a, FB b) {
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a(kk), b(kk), acc, 0, 0, 0);
  return acc;
}
constexpr f32x16 ZERO16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// per-channel batch statistics of graph g: (mean, 1/sqrt(var + eps)), tabulated once per BatchNorm from the f64 sums by
// gnn_t_stat_table (the consumers read two floats per element instead of redoing an f64 divide and square root)
struct Stat { float mean, rstd; };
__device__ inline Stat load_stat(const float2 *tab, int g, int c, int /*count*/) {
  const float2 t = tab[(size_t)g * 32 + c];
  return Stat{t.x, t.y};
}
// Which graph a row (an edge, or a node) belongs to.  The kernels below are templates over one of these two; `of(r)` is the
// graph of row r, `of(r, s)` the same for a caller that holds the edge's source node s in a register already.
//   EqualGraphs   graphs of `per` rows each, listed graph after graph: r / per.  One int, passed where the kernels used to take
//                 `Eg` / `Rg`: these instantiations are the kernels as they were.
//   RaggedGraphs  graphs of n_g nodes each whose edge counts differ (graph g owns edges [edge_off[g], edge_off[g + 1]), in any
//                 order inside the graph): the graph of an edge is that of its source node, src[e] / n_g -- the register the
//                 kernel holds, or one 4-byte load where it holds none.  Always in [0, G) for node ids in [0, n).
struct EqualGraphs {
  int per;
  __device__ int of(int r) const { return r / per; }
  __device__ int of(int r, int /*s*/) const { return r / per; }
};
struct RaggedGraphs {
  const int *src;
  int ng;
  __device__ int of(int e) const { return src[e] / ng; }
  __device__ int of(int /*e*/, int s) const { return s / ng; }
};

// the rows behind an edge statistic of graph g: `count_e`, or the graph's own edge_off[g + 1] - edge_off[g] (ragged; a graph
// without edges -- nothing reads its entries -- counts one row, so that no table entry is a 0 / 0)
__device__ inline int edge_count(const int *edge_off, int g, int count_e) {
  return edge_off ? max(edge_off[g + 1] - edge_off[g], 1) : count_e;
}

// forward table: (mean, rstd); backward table: (sum(g_y) / count, sum(g_y * zhat) / count)
// (the edge and the node BatchNorm of a layer in one launch: their sums and their tables are neighbours in memory; the first
// G * 32 entries count `count_e` rows each -- edge_off: see edge_count --, the next G * 32 `count_v`)
__global__ void gnn_t_stat_table(int G, int count_e, int count_v, const int *edge_off, const double *sums, float2 *tab, int backward) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 2 * G * 32) return;
  const int count = idx < G * 32 ? edge_count(edge_off, idx >> 5, count_e) : count_v;
  const double s = sums[(size_t)idx * 2], q = sums[(size_t)idx * 2 + 1];
  if (backward) { tab[idx] = make_float2((float)(s / count), (float)(q / count)); return; }
  const double m = s / count;
  double v = q / count - m * m;
  v = v < 0.0 ? 0.0 : v;
  tab[idx] = make_float2((float)m, (float)(1.0 / sqrt(v + (double)BN_EPS)));
}

// BatchNorm in evaluation mode (running statistics, the same for every graph): (mean, 1 / sqrt(var + eps)) from the caller's
// [32][2] (mean, var) block into the table of all G graphs
// (both BatchNorms of a layer: fixed = [2 (e, v)][32][2])
__global__ void gnn_t_fixed_table(int G, const float *fixed, float2 *tab) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 2 * G * 32) return;
  const int c = (idx & 31) + (idx >= G * 32 ? 32 : 0);
  tab[idx] = make_float2(fixed[c * 2], (float)(1.0 / sqrt((double)fixed[c * 2 + 1] + (double)BN_EPS)));
}

// ------------------------------------------------------------------ forward
// ze = w We^T + be + x3[src] + x4[dst] for one 32-edge tile per wave; channel sums of the tile -> f64 atomics
template <class GR>
__global__ void __launch_bounds__(256)
gnn_t_edge_pre(int E, GR gr, const int *src, const int *dst, const float *We, const float *be, const float *X,
               const float *w0, float *ze, double *sums) {
  __shared__ __attribute__((aligned(16))) float tile_s[4][32][36];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float (*tile)[36] = tile_s[wave];
  __shared__ double red[4][64];                             // (one add per channel, statistic and workgroup: see gnn_t_bwd_stats)
  const int e0 = (blockIdx.x * 4 + wave) * 32;
  const int o = lane & 31, h = lane >> 5, c0 = (lane & 7) * 4;
  // the workgroup's 128 edges in one graph (uniform): the four waves' sums are added in LDS and flushed once
  const int wg0 = blockIdx.x * 128, wg1 = min(wg0 + 127, E - 1);
  const bool one_graph = gr.of(wg0) == gr.of(wg1);
  if (e0 >= E) {                                            // (a wave past the end: nothing to do but the workgroup's barrier)
    if (one_graph) { red[wave][lane] = 0.0; __syncthreads(); }
    return;
  }
  // (Round 6, last session: the tile's rows, the edge ids, the lane's sixteen entries of We and -- once the ids are back -- the
  // eight gathered node rows are all in flight before the matrix product; the gathers used to sit in each pass's `if (e < E)`
  // block behind its own id loads: eight dependent memory round trips per tile after the product.)
  float4 wrow[4], wev[4], a3q[4], a4q[4];
  int sq[4], dq[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int el = q * 8 + (lane >> 3), e = min(e0 + el, E - 1);
    wrow[q] = *reinterpret_cast<const float4 *>(w0 + (size_t)e * TU + c0);
    sq[q] = src[e]; dq[q] = dst[e];
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) wev[v] = *reinterpret_cast<const float4 *>(We + o * TU + h * 16 + 4 * v);
  const float4 bb = *reinterpret_cast<const float4 *>(be + c0);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    a3q[q] = *reinterpret_cast<const float4 *>(X + (size_t)sq[q] * 128 + 64 + c0);
    a4q[q] = *reinterpret_cast<const float4 *>(X + (size_t)dq[q] * 128 + 96 + c0);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) *reinterpret_cast<float4 *>(&tile[q * 8 + (lane >> 3)][c0]) = wrow[q];
  __builtin_amdgcn_wave_barrier();
  const f32x16 acc = mfma32(ZERO16, [&](int kk) { return tile[o][h * 16 + kk]; },
                            [&](int kk) { const float4 w4 = wev[kk >> 2]; return (kk & 3) == 0 ? w4.x : (kk & 3) == 1 ? w4.y : (kk & 3) == 2 ? w4.z : w4.w; });
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int r = 0; r < 16; ++r) tile[drow(r, lane)][o] = acc[r];
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int el = q * 8 + (lane >> 3), e = e0 + el;
    float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e < E) {
      const float4 g = *reinterpret_cast<const float4 *>(&tile[el][c0]);
      const float4 a3 = a3q[q], a4 = a4q[q];
      z = make_float4(g.x + bb.x + a3.x + a4.x, g.y + bb.y + a3.y + a4.y, g.z + bb.z + a3.z + a4.z, g.w + bb.w + a3.w + a4.w);
      *reinterpret_cast<float4 *>(ze + (size_t)e * TU + c0) = z;
    }
    *reinterpret_cast<float4 *>(&tile[el][c0]) = z;
  }
  __builtin_amdgcn_wave_barrier();
  // lanes 0..31: sum of channel o over the tile's edges, lanes 32..63: sum of squares; flushed per graph
  double accd = 0.0;
  int gcur = gr.of(e0);
  for (int el = 0; el < 32 && e0 + el < E; ++el) {
    const int g = gr.of(e0 + el);
    if (g != gcur) { unsafeAtomicAdd(sums + ((size_t)gcur * 32 + o) * 2 + h, accd); accd = 0.0; gcur = g; }
    const float v = tile[el][o];
    accd += h ? (double)v * (double)v : (double)v;
  }
  if (one_graph) {
    red[wave][lane] = accd;
    __syncthreads();
    if (wave == 0) unsafeAtomicAdd(sums + ((size_t)gcur * 32 + o) * 2 + h, red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane]);
  } else unsafeAtomicAdd(sums + ((size_t)gcur * 32 + o) * 2 + h, accd);
}

// zv = x1 + mean over out-edges of sigmoid(w) * x2[dst]; 8 nodes per workgroup, 32 lanes per node
__global__ void __launch_bounds__(256)
gnn_t_node_pre(int n, int ng, const int *dst, const int *rowptr, const int *perm, const float *X, const float *w0,
               float *zv, double *sums) {
  __shared__ double red[8][32][2];                          // (one add per channel and workgroup: see gnn_t_bwd_stats)
  const int il = threadIdx.x >> 5, o = threadIdx.x & 31;
  const int i = blockIdx.x * 8 + il;
  const bool live = i < n;
  float z = 0.0f;
  if (live) {
    const int lo = rowptr[i], hi = rowptr[i + 1];
    float agg = 0.0f;
    // (four incident edges at a time: their ids, then their rows and endpoints, then the endpoints' rows are each in flight
    // together -- one edge at a time the loop was perm -> dst -> X, three dependent memory round trips per edge; the sum keeps
    // its order)
    for (int q0 = lo; q0 < hi; q0 += 4) {
      int ee[4], dd[4];
      float ww[4], xx[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) { const int qq = min(q0 + j, hi - 1); ee[j] = perm ? perm[qq] : qq; }
#pragma unroll
      for (int j = 0; j < 4; ++j) { dd[j] = dst[ee[j]]; ww[j] = w0[(size_t)ee[j] * TU + o]; }
#pragma unroll
      for (int j = 0; j < 4; ++j) xx[j] = X[(size_t)dd[j] * 128 + 32 + o];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (q0 + j < hi) agg = fmaf(t_sigmoid(ww[j]), xx[j], agg);
    }
    agg = agg / (float)max(hi - lo, 1);
    z = X[(size_t)i * 128 + o] + agg;
    zv[(size_t)i * TU + o] = z;
  }
  const int i0 = blockIdx.x * 8, i1 = min(i0 + 7, n - 1);
  if (i0 / ng == i1 / ng) {                                 // the workgroup's nodes lie in one graph (uniform)
    red[il][o][0] = live ? (double)z : 0.0; red[il][o][1] = live ? (double)z * (double)z : 0.0;
    __syncthreads();
    if (threadIdx.x < 64) {
      const int oo = threadIdx.x >> 1, k = threadIdx.x & 1;
      double t = 0.0;
#pragma unroll
      for (int j = 0; j < 8; ++j) t += red[j][oo][k];
      unsafeAtomicAdd(sums + ((size_t)(i0 / ng) * 32 + oo) * 2 + k, t);
    }
  } else if (live) {
    const int g = i / ng;
    unsafeAtomicAdd(sums + ((size_t)g * 32 + o) * 2, (double)z);
    unsafeAtomicAdd(sums + ((size_t)g * 32 + o) * 2 + 1, (double)z * (double)z);
  }
}

// w' = w + silu(gamma * (ze - mean) * rstd + beta)
template <class GR>
__global__ void __launch_bounds__(256)
gnn_t_edge_post(int E, GR gr, const float *gamma, const float *beta, const float2 *sums, const float *w0, const float *ze,
                float *w1) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)E * TU) return;
  const int e = (int)(idx >> 5), c = (int)(idx & 31);
  const Stat st = load_stat(sums, gr.of(e), c, 0);
  const float y = fmaf((ze[idx] - st.mean) * st.rstd, gamma[c], beta[c]);
  w1[idx] = w0[idx] + t_silu(y);
}

// x' = x + silu(bn_v(zv)); then the NEXT layer's node linears X' = x' Wv^T + bv (WT/bv = next layer's, or null)
__global__ void __launch_bounds__(256)
gnn_t_node_post(int n, int ng, const float *gamma, const float *beta, const float2 *sums, const float *x0, const float *zv,
                float *x1, const float *WTnext, const float *bvnext, float *Xnext) {
  __shared__ float xs[8][TU];
  const int il = threadIdx.x >> 5, o = threadIdx.x & 31;
  const int i = blockIdx.x * 8 + il;
  float xn = 0.0f;
  if (i < n) {
    const Stat st = load_stat(sums, i / ng, o, ng);
    const float y = fmaf((zv[(size_t)i * TU + o] - st.mean) * st.rstd, gamma[o], beta[o]);
    xn = x0[(size_t)i * TU + o] + t_silu(y);
    x1[(size_t)i * TU + o] = xn;
  }
  if (!WTnext) return;
  xs[il][o] = xn;
  __syncthreads();
  if (i >= n) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float acc = bvnext[q * 32 + o];
    for (int c = 0; c < TU; ++c) acc = fmaf(xs[il][c], WTnext[c * 128 + q * 32 + o], acc);
    Xnext[(size_t)i * 128 + q * 32 + o] = acc;
  }
}

// x0 = silu(v_lin0 xin), pre-activation a0 saved; X(0) = layer-0 node linears
__global__ void __launch_bounds__(256)
gnn_t_node_init(int n, int feats, const float *xin, const float *params, float *a0, float *x, float *X) {
  __shared__ float xs[8][TU];
  const int il = threadIdx.x >> 5, o = threadIdx.x & 31;
  const int i = blockIdx.x * 8 + il;
  const float *W = params, *b = params + 32 * feats;
  float v = 0.0f;
  if (i < n) {
    v = b[o];
    for (int f = 0; f < feats; ++f) v = fmaf(xin[(size_t)i * feats + f], W[o * feats + f], v);
    a0[(size_t)i * TU + o] = v;
    v = t_silu(v);
    x[(size_t)i * TU + o] = v;
  }
  xs[il][o] = v;
  __syncthreads();
  if (i >= n) return;
  const float *WT = params + off_layer(feats, 0), *bv = WT + 32 * 128;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float acc = bv[q * 32 + o];
    for (int c = 0; c < TU; ++c) acc = fmaf(xs[il][c], WT[c * 128 + q * 32 + o], acc);
    X[(size_t)i * 128 + q * 32 + o] = acc;
  }
}
__global__ void __launch_bounds__(256)
gnn_t_edge_init(int E, int feats, const float *attr, const float *params, float *w) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)E * TU) return;
  const int e = (int)(idx >> 5), c = (int)(idx & 31);
  const float *W = params + 32 * feats + 32, *b = W + 32;
  w[idx] = t_silu(fmaf(attr[e], W[c], b[c]));
}

// head forward (sigmoid(W3 silu(W2 silu(W1 w + b1) + b2) + b3)), one 32-edge tile per wave
__global__ void __launch_bounds__(256)
gnn_t_head_fwd(int E, const float *hp, const float *w, float *heu) {
  __shared__ __attribute__((aligned(16))) float tile_s[4][32][36];
  const float *W1 = hp, *b1 = W1 + 1024, *W2 = b1 + 32, *b2 = W2 + 1024, *W3 = b2 + 32, *b3 = W3 + 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int e0 = (blockIdx.x * 4 + wave) * 32;
  if (e0 >= E) return;
  const int o = lane & 31, h = lane >> 5, c0 = (lane & 7) * 4;
  float (*t)[36] = tile_s[wave];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int el = q * 8 + (lane >> 3), e = min(e0 + el, E - 1);
    *reinterpret_cast<float4 *>(&t[el][c0]) = *reinterpret_cast<const float4 *>(w + (size_t)e * TU + c0);
  }
  __builtin_amdgcn_wave_barrier();
  f32x16 acc = mfma32(ZERO16, [&](int kk) { return t[o][h * 16 + kk]; }, [&](int kk) { return W1[o * TU + h * 16 + kk]; });
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int r = 0; r < 16; ++r) t[drow(r, lane)][o] = t_silu(acc[r] + b1[o]);
  __builtin_amdgcn_wave_barrier();
  acc = mfma32(ZERO16, [&](int kk) { return t[o][h * 16 + kk]; }, [&](int kk) { return W2[o * TU + h * 16 + kk]; });
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int r = 0; r < 16; ++r) t[drow(r, lane)][o] = t_silu(acc[r] + b2[o]) * W3[o];
  __builtin_amdgcn_wave_barrier();
  if (lane < 32) {
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < TU; ++c) s = s + t[lane][c];
    const int e = e0 + lane;
    if (e < E) heu[e] = t_sigmoid(s + b3[0]);
  }
}

// ------------------------------------------------------------------ backward
// flush a wave's 32x32 accumulator (MFMA output layout) and a per-channel vector into global memory
__device__ inline void flush_acc(float *dstM, const f32x16 &acc, int lane) {
  const int j = lane & 31;
#ifdef DACO_ABLATE_FLUSH   // (measurement build: one atomic per lane instead of sixteen -- what the contended flush costs)
  float t = 0.0f;
#pragma unroll
  for (int r = 0; r < 16; ++r) t += acc[r];
  unsafeAtomicAdd(dstM + drow(0, lane) * TU + j, t);
#else
#pragma unroll
  for (int r = 0; r < 16; ++r) unsafeAtomicAdd(dstM + drow(r, lane) * TU + j, acc[r]);
#endif
}

// Round 6: one flush per WORKGROUP.  Every wave used to add its 32x32 accumulator to the same 1 024 words of the flat gradient: an
// address's atomic adds execute one after the other in the L2 (~75 ns apiece), so a launch of W wavefronts took W x 75 ns whatever
// else it did -- gnn_t_edge_bwd 300 us at 200 k edges (4 096 wavefronts), 70 us at 20 k (625), gnn_t_head_bwd 329 us; making the
// flush sixteen times smaller changed nothing (profiles/r06_gnn_train_flush_ablation.txt: it is the number of adds PER ADDRESS).
// The four waves of a workgroup now add their accumulators in LDS first (ds_add_f32: four adds per word), a launch has at most one
// workgroup per CU (waves walk more tiles), and the workgroup's 256 threads flush four words each.
// `red`: >= 1 024 floats of LDS no wave uses any more (callers put a barrier before; all 256 threads call this).
__device__ inline void flush_acc_wg(float *dstM, const f32x16 &acc, float *red) {
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31;
  for (int i = tid; i < 1024; i += 256) red[i] = 0.0f;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 16; ++r) atomicAdd(&red[drow(r, lane) * TU + j], acc[r]);
  __syncthreads();
  for (int i = tid; i < 1024; i += 256) unsafeAtomicAdd(dstM + i, red[i]);
  __syncthreads();
}
// the same for per-channel vectors: every lane holds a partial sum for channel `o` (two lanes per wave and channel)
__device__ inline void flush_vec_wg(float *dst, float v, int o, float *red /* >= 32 floats */, int words = 32) {
  const int tid = threadIdx.x;
  if (tid < 32) red[tid] = 0.0f;
  __syncthreads();
  atomicAdd(&red[o], v);
  __syncthreads();
  if (tid < words) unsafeAtomicAdd(dst + tid, red[tid]);
  __syncthreads();
}

// head backward: waves walk tiles (grid-stride), recompute a1, a2, accumulate gW1/gW2/gW3/gb in registers
__global__ void __launch_bounds__(256)
gnn_t_head_bwd(int E, const float *hp, const float *w, const float *heu, const float *gheu, float *gw, float *ghp) {
  __shared__ __attribute__((aligned(16))) float tin_s[4][32][36], ta_s[4][32][36], tg_s[4][32][36];
  const float *W1 = hp, *b1 = W1 + 1024, *W2 = b1 + 32, *b2 = W2 + 1024, *W3 = b2 + 32;
  float *gW1 = ghp, *gb1 = gW1 + 1024, *gW2 = gb1 + 32, *gb2 = gW2 + 1024, *gW3 = gb2 + 32, *gb3 = gW3 + 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int o = lane & 31, h = lane >> 5, c0 = (lane & 7) * 4;
  float (*tin)[36] = tin_s[wave], (*ta)[36] = ta_s[wave], (*tg)[36] = tg_s[wave];
  f32x16 aW1 = ZERO16, aW2 = ZERO16;
  float aW3 = 0.f, ab1 = 0.f, ab2 = 0.f, ab3 = 0.f;
  const int ntiles = (E + 31) / 32;
  // (Round 6, last session: the lane's entries of W1 / W2 -- rows for the forward products, columns for the backward ones -- and
  // b1, b2, W3 are read once, and a tile's rows and its 16 + 16 per-edge scalars are in flight together; read where they are used
  // they were some eighty dependent memory round trips per tile.)
  float w1r[16], w2r[16], w1c[16], w2c[16];
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) {
    w1r[kk] = W1[o * TU + h * 16 + kk]; w2r[kk] = W2[o * TU + h * 16 + kk];
    w1c[kk] = W1[(h * 16 + kk) * TU + o]; w2c[kk] = W2[(h * 16 + kk) * TU + o];
  }
  const float b1o = b1[o], b2o = b2[o], w3o = W3[o];
  for (int tix = blockIdx.x * 4 + wave; tix < ntiles; tix += gridDim.x * 4) {
    const int e0 = tix * 32;
    float4 win[4];
    float hvr[16], ghr[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int el = q * 8 + (lane >> 3), e = min(e0 + el, E - 1);
      win[q] = *reinterpret_cast<const float4 *>(w + (size_t)e * TU + c0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) { const int e = min(e0 + drow(r, lane), E - 1); hvr[r] = heu[e]; ghr[r] = gheu[e]; }
#pragma unroll
    for (int q = 0; q < 4; ++q) *reinterpret_cast<float4 *>(&tin[q * 8 + (lane >> 3)][c0]) = win[q];
    __builtin_amdgcn_wave_barrier();
    // a1 = w W1^T + b1 -> ta (pre-activation), h1 = silu(a1) -> tg (temporarily)
    f32x16 acc = mfma32(ZERO16, [&](int kk) { return tin[o][h * 16 + kk]; }, [&](int kk) { return w1r[kk]; });
#pragma unroll
    for (int r = 0; r < 16; ++r) { const float a = acc[r] + b1o; ta[drow(r, lane)][o] = a; tg[drow(r, lane)][o] = t_silu(a); }
    __builtin_amdgcn_wave_barrier();
    // a2 = h1 W2^T + b2; h2 = silu(a2); gs = gheu * heu * (1 - heu) per edge
    acc = mfma32(ZERO16, [&](int kk) { return tg[o][h * 16 + kk]; }, [&](int kk) { return w2r[kk]; });
    // per-edge scalar gs for the 16 rows this lane holds
    float a2r[16], gsr[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int e = e0 + drow(r, lane);
      float gs = 0.0f;
      if (e < E) { const float hv = hvr[r]; gs = ghr[r] * hv * (1.0f - hv); }
      a2r[r] = acc[r] + b2o; gsr[r] = gs;
    }
    // gW3[o] += sum_e gs * h2[e][o]; gb3 += sum_e gs (lane o = 0 of half 0 only, below); g_a2 = gs * W3[o] * dsilu(a2)
    float ga2[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      aW3 += gsr[r] * t_silu(a2r[r]);
      ga2[r] = gsr[r] * w3o * t_dsilu(a2r[r]);
      ab2 += ga2[r];
      if (o == 0) ab3 += gsr[r];
    }
    // gW2 += g_a2^T h1 (h1 is in tg); then g_h1 = g_a2 W2 -> needs g_a2 as a tile: reuse tin after saving nothing
    // (w tile is still needed for gW1: keep tin, put g_a2 into a second use of tg AFTER the outer product)
    // stage g_a2 in registers -> write to tin? no: use ta for a1 (needed), so write g_a2 over tg after reading h1.
    // 1) outer product needs A = g_a2^T (from a tile) and B = h1 (tg): put g_a2 into tin's place temporarily is not
    //    possible (w needed later), so spill w tile to registers first.
    float4 wsave[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) wsave[q] = *reinterpret_cast<const float4 *>(&tin[q * 8 + (lane >> 3)][c0]);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < 16; ++r) tin[drow(r, lane)][o] = ga2[r];                 // tin := g_a2 [edge][ch]
    __builtin_amdgcn_wave_barrier();
    aW2 = mfma32(aW2, [&](int kk) { return tin[h * 16 + kk][o]; }, [&](int kk) { return tg[h * 16 + kk][o]; });
    // g_h1 = g_a2 W2 : D[e][c] = sum_o g_a2[e][o] W2[o][c]
    acc = mfma32(ZERO16, [&](int kk) { return tin[o][h * 16 + kk]; }, [&](int kk) { return w2c[kk]; });
    __builtin_amdgcn_wave_barrier();
    // g_a1 = g_h1 * dsilu(a1) -> tg
#pragma unroll
    for (int r = 0; r < 16; ++r) { const float g = acc[r] * t_dsilu(ta[drow(r, lane)][o]); tg[drow(r, lane)][o] = g; ab1 += g; }
    __builtin_amdgcn_wave_barrier();
    // restore the w tile, gW1 += g_a1^T w, gw = g_a1 W1
#pragma unroll
    for (int q = 0; q < 4; ++q) *reinterpret_cast<float4 *>(&tin[q * 8 + (lane >> 3)][c0]) = wsave[q];
    __builtin_amdgcn_wave_barrier();
    aW1 = mfma32(aW1, [&](int kk) { return tg[h * 16 + kk][o]; }, [&](int kk) { return tin[h * 16 + kk][o]; });
    acc = mfma32(ZERO16, [&](int kk) { return tg[o][h * 16 + kk]; }, [&](int kk) { return w1c[kk]; });
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < 16; ++r) ta[drow(r, lane)][o] = acc[r];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int el = q * 8 + (lane >> 3), e = e0 + el;
      if (e < E) *reinterpret_cast<float4 *>(gw + (size_t)e * TU + c0) = *reinterpret_cast<const float4 *>(&ta[el][c0]);
    }
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();                                         // (the tiles in LDS are dead: the reduction area)
  float *red = &tin_s[0][0][0];
  flush_acc_wg(gW1, aW1, red);
  flush_acc_wg(gW2, aW2, red);
  // per-channel vectors: both halves hold partial sums for channel o
  flush_vec_wg(gW3, aW3, o, red);
  flush_vec_wg(gb1, ab1, o, red);
  flush_vec_wg(gb2, ab2, o, red);
  flush_vec_wg(gb3, o == 0 ? ab3 : 0.0f, 0, red, 1);       // (a scalar: the lanes of channel 0 hold its partial sums)
}

// sum(g_y), sum(g_y * zhat) per channel and graph for an [R,32] tensor (edges or nodes); g_y = gout * dsilu(y)
template <class GR>
__global__ void __launch_bounds__(256)
gnn_t_bwd_stats(int R, GR gr, const float *gamma, const float *beta, const float2 *fsums, const float *z, const float *gout,
                double *bsums) {
  // 8 rows per pass and workgroup-pass; thread = (row slot, channel); rows of one workgroup: a contiguous chunk
  // (round 6: the adds to one word of `bsums` execute one after the other in the L2 -- ~75 ns apiece -- and every thread used to
  // add its own partial sums: 8 x (workgroups per graph) adds per word, 43 us per launch at 200 k edges.  A workgroup whose rows
  // lie in one graph now sums its eight row slots in LDS first and adds once per channel.)
  __shared__ double red[8][32][2];
  const int il = threadIdx.x >> 5, o = threadIdx.x & 31;
  const int rows_per_wg = 256;
  const int r0 = blockIdx.x * rows_per_wg, r1 = min(R, r0 + rows_per_wg);
  const bool one_graph = r0 < r1 && gr.of(r0) == gr.of(r1 - 1);         // uniform
  double s1 = 0.0, s2 = 0.0;
  int gcur = -1;
  // (Round 6, last session: eight of a thread's rows at a time, their loads issued together.  One row per iteration -- with the
  // flush of a finished graph inside the loop, which keeps the compiler from moving loads across iterations -- the launch was 32
  // dependent memory round trips per thread: 15.3 us at 40 k edges for 10 MB.  The sums keep their order.)
  const float gam = gamma[o], bet = beta[o];
  Stat st = {0.f, 0.f};
  constexpr int UN = 8;
  for (int rb = r0 + il; rb < r1; rb += 8 * UN) {
    float zz[UN], gg[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int rc = min(rb + 8 * u, r1 - 1);
      zz[u] = z[(size_t)rc * TU + o]; gg[u] = gout[(size_t)rc * TU + o];
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int r = rb + 8 * u;
      if (r < r1) {
        const int g = gr.of(r);
        if (g != gcur) {
          if (gcur >= 0) { unsafeAtomicAdd(bsums + ((size_t)gcur * 32 + o) * 2, s1); unsafeAtomicAdd(bsums + ((size_t)gcur * 32 + o) * 2 + 1, s2); }
          s1 = s2 = 0.0; gcur = g;
          st = load_stat(fsums, g, o, 0);
        }
        const float zh = (zz[u] - st.mean) * st.rstd;
        const float gy = gg[u] * t_dsilu(fmaf(zh, gam, bet));
        s1 += (double)gy; s2 += (double)gy * (double)zh;
      }
    }
  }
  if (one_graph) {
    red[il][o][0] = s1; red[il][o][1] = s2;
    __syncthreads();
    if (threadIdx.x < 64) {
      const int oo = threadIdx.x >> 1, k = threadIdx.x & 1;
      double t = 0.0;
#pragma unroll
      for (int j = 0; j < 8; ++j) t += red[j][oo][k];
      unsafeAtomicAdd(bsums + ((size_t)gr.of(r0) * 32 + oo) * 2 + k, t);
    }
  } else if (gcur >= 0) { unsafeAtomicAdd(bsums + ((size_t)gcur * 32 + o) * 2, s1); unsafeAtomicAdd(bsums + ((size_t)gcur * 32 + o) * 2 + 1, s2); }
}

// g_z of a BatchNorm'd row element: (gamma * rstd) * (g_y - mean(g_y) - zhat * mean(g_y * zhat))
__device__ inline float bn_bwd(float gout, float z, const Stat &st, float gamma, float beta, const float2 *btab, int g, int c,
                               int /*count*/) {
  const float zh = (z - st.mean) * st.rstd;
  const float gy = gout * t_dsilu(fmaf(zh, gamma, beta));
  const float2 m = btab[(size_t)g * 32 + c];
  return gamma * st.rstd * (gy - m.x - zh * m.y);
}

// (the same with the backward table's entry already in hand)
__device__ inline float bn_bwd_m(float gout, float z, const Stat &st, float gamma, float beta, const float2 m) {
  const float zh = (z - st.mean) * st.rstd;
  const float gy = gout * t_dsilu(fmaf(zh, gamma, beta));
  return gamma * st.rstd * (gy - m.x - zh * m.y);
}

// node side: g_zv -> gX[:, 0:32] (x1 block) and g_msg = g_zv / degree; BatchNorm parameter gradients
__global__ void __launch_bounds__(256)
gnn_t_node_bwd_apply(int n, int ng, const int *rowptr, const float *gamma, const float *beta, const float2 *fsums,
                     const float2 *bsums, const float *zv, const float *gx, float *gX, float *gmsg, int clear_rest) {
  const int il = threadIdx.x >> 5, o = threadIdx.x & 31;
  const int i = blockIdx.x * 8 + il;
  if (i >= n) return;
  const int g = i / ng;
  const Stat st = load_stat(fsums, g, o, ng);
  const float gz = bn_bwd(gx[(size_t)i * TU + o], zv[(size_t)i * TU + o], st, gamma[o], beta[o], bsums, g, o, ng);
  gX[(size_t)i * 128 + o] = gz;
  if (clear_rest) { gX[(size_t)i * 128 + 32 + o] = 0.0f; gX[(size_t)i * 128 + 64 + o] = 0.0f; gX[(size_t)i * 128 + 96 + o] = 0.0f; }
  gmsg[(size_t)i * TU + o] = gz / (float)max(rowptr[i + 1] - rowptr[i], 1);
}

// edge side of a layer's backward, waves walk 32-edge tiles
template <class GR>
__global__ void __launch_bounds__(256)
gnn_t_edge_bwd(int E, GR gr, const int *src, const int *dst, const float *We, const float *gamma, const float *beta,
               const float2 *fsums, const float2 *bsums, const float *X, const float *w0, const float *ze, const float *gmsg,
               float *gw /* in: grad wrt w', out: grad wrt w */, float *gX, float *gWe, float *gbe,
               float *c2buf /* [E][32] d/d x2[dst] per edge, or null */, float *gzbuf /* [E][32] g_ze per edge */) {
  __shared__ __attribute__((aligned(16))) float tw_s[4][32][36], tg_s[4][32][36];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int o = lane & 31, h = lane >> 5, c0 = (lane & 7) * 4;
  float (*tw)[36] = tw_s[wave], (*tg)[36] = tg_s[wave];
  f32x16 aW = ZERO16;
  float ab = 0.0f;
  const int ntiles = (E + 31) / 32;
  // (a lane serves the same four channels c0 .. c0 + 3 of every edge it touches: their BatchNorm scale / shift are read once)
  float gam[4], bet[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { gam[k] = gamma[c0 + k]; bet[k] = beta[c0 + k]; }
  float wecol[16];                                            // We[h * 16 + kk][o]: the B operand of g_w = g_ze We, the same for every tile
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) wecol[kk] = We[(h * 16 + kk) * TU + o];
  for (int tix = blockIdx.x * 4 + wave; tix < ntiles; tix += gridDim.x * 4) {
    const int e0 = tix * 32;
    // the statistics of the lane's four channels, once per tile when the tile lies inside one graph (32 edges, graphs of Eg edges:
    // almost always) instead of once per element: sixteen 8-byte loads per lane and tile instead of thirty-two per pass
    const int g_first = gr.of(e0), g_last = gr.of(min(e0 + 31, E - 1));
    const bool one_graph = g_first == g_last;
    Stat st_t[4];
    float2 bs_t[4];
    if (one_graph) {
#pragma unroll
      for (int k = 0; k < 4; ++k) { st_t[k] = load_stat(fsums, g_first, c0 + k, 0); bs_t[k] = bsums[(size_t)g_first * 32 + c0 + k]; }
    }
    // edge-major pass: g_ze per element, scatter-adds, gate path; tiles tw = w, tg = g_ze
    // (Round 6, last session: the four passes' loads are issued together -- ids and rows first, then the two gathers that need the
    // ids -- instead of inside each pass's `if (e < E)` block, where every pass waited for its own two memory round trips: eight
    // dependent trips per tile; a pass past the end reads edge E - 1 and drops it.)
    float4 gres[4], gate_term[4];
    int sq[4], dq[4];
    float4 wvq[4], zzq[4], gmq[4], x2q[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = e0 + q * 8 + (lane >> 3), ec = e < E ? e : E - 1;
      sq[q] = src[ec]; dq[q] = dst[ec];
      wvq[q] = *reinterpret_cast<const float4 *>(w0 + (size_t)ec * TU + c0);
      zzq[q] = *reinterpret_cast<const float4 *>(ze + (size_t)ec * TU + c0);
      gres[q] = *reinterpret_cast<const float4 *>(gw + (size_t)ec * TU + c0);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      gmq[q] = *reinterpret_cast<const float4 *>(gmsg + (size_t)sq[q] * TU + c0);
      x2q[q] = *reinterpret_cast<const float4 *>(X + (size_t)dq[q] * 128 + 32 + c0);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int el = q * 8 + (lane >> 3), e = e0 + el;
      float4 wv = make_float4(0.f, 0.f, 0.f, 0.f), gz = wv;
      gate_term[q] = wv;
      if (e < E) {
        const int s = sq[q], d = dq[q], g = gr.of(e, s);
        wv = wvq[q];
        const float4 zz = zzq[q];
        const float4 go = gres[q];
        const float zc[4] = {zz.x, zz.y, zz.z, zz.w}, gc[4] = {go.x, go.y, go.z, go.w}, wc[4] = {wv.x, wv.y, wv.z, wv.w};
        float gzc[4], gt[4], c2c[4];
        const float4 gm = gmq[q];
        const float4 x2 = x2q[q];
        const float gmc[4] = {gm.x, gm.y, gm.z, gm.w}, x2c[4] = {x2.x, x2.y, x2.z, x2.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const Stat st = one_graph ? st_t[k] : load_stat(fsums, g, c0 + k, 0);
          const float2 bm = one_graph ? bs_t[k] : bsums[(size_t)g * 32 + c0 + k];
          gzc[k] = bn_bwd_m(gc[k], zc[k], st, gam[k], bet[k], bm);
          const float gate = t_sigmoid(wc[k]);
          gt[k] = gmc[k] * x2c[k] * gate * (1.0f - gate);                   // d msg / d w through the gate
          c2c[k] = gmc[k] * gate;                                           // d / d x2[dst]
          if (!c2buf) {
            unsafeAtomicAdd(gX + (size_t)d * 128 + 32 + c0 + k, c2c[k]);        // d / d x2[dst]
            unsafeAtomicAdd(gX + (size_t)s * 128 + 64 + c0 + k, gzc[k]);        // d / d x3[src]
            unsafeAtomicAdd(gX + (size_t)d * 128 + 96 + c0 + k, gzc[k]);        // d / d x4[dst]
          }
        }
        gz = make_float4(gzc[0], gzc[1], gzc[2], gzc[3]);
        if (c2buf) {
          // per-edge contributions for gnn_t_gather_bwd (f32 atomics into gX run at ~16 per clock on this chip: 19 M of them
          // were 0.5 ms per layer at 200 k edges; two coalesced row stores here, three CSR row sums there)
          *reinterpret_cast<float4 *>(c2buf + (size_t)e * TU + c0) = make_float4(c2c[0], c2c[1], c2c[2], c2c[3]);
          *reinterpret_cast<float4 *>(gzbuf + (size_t)e * TU + c0) = gz;
        }
        gate_term[q] = make_float4(gt[0], gt[1], gt[2], gt[3]);
      } else {
        gres[q] = wv;
      }
      *reinterpret_cast<float4 *>(&tw[el][c0]) = wv;
      *reinterpret_cast<float4 *>(&tg[el][c0]) = gz;
    }
    __builtin_amdgcn_wave_barrier();
    // gWe[o][c] += sum_e g_ze[e][o] * w[e][c];  gbe[o] += sum_e g_ze[e][o]
    aW = mfma32(aW, [&](int kk) { return tg[h * 16 + kk][o]; }, [&](int kk) { return tw[h * 16 + kk][o]; });
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) ab += tg[h * 16 + kk][o];
    // g_w (through the edge linear) = g_ze We : D[e][c] = sum_o g_ze[e][o] We[o][c]
    const f32x16 acc = mfma32(ZERO16, [&](int kk) { return tg[o][h * 16 + kk]; }, [&](int kk) { return wecol[kk]; });
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < 16; ++r) tw[drow(r, lane)][o] = acc[r];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int el = q * 8 + (lane >> 3), e = e0 + el;
      if (e < E) {
        const float4 a = *reinterpret_cast<const float4 *>(&tw[el][c0]);
        float4 out;
        out.x = gres[q].x + a.x + gate_term[q].x; out.y = gres[q].y + a.y + gate_term[q].y;
        out.z = gres[q].z + a.z + gate_term[q].z; out.w = gres[q].w + a.w + gate_term[q].w;
        *reinterpret_cast<float4 *>(gw + (size_t)e * TU + c0) = out;
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  float *red = &tw_s[0][0][0];
  flush_acc_wg(gWe, aW, red);
  flush_vec_wg(gbe, ab, o, red);
}

// gX[:, x2 | x3 | x4 blocks] as sums over CSR rows of the per-edge contributions edge_bwd stored (no atomics, fixed order):
// x2[i] and x4[i] over the edges entering i (perm_dst / rowptr_dst), x3[i] over the edges leaving it (perm / rowptr).
// 8 nodes per workgroup, lane = channel.
__global__ void __launch_bounds__(256)
gnn_t_gather_bwd(int n, const int *rowptr, const int *perm, const int *rowptr_dst, const int *perm_dst, const float *c2buf,
                 const float *gzbuf, float *gX) {
  const int il = threadIdx.x >> 5, o = threadIdx.x & 31;
  const int i = blockIdx.x * 8 + il;
  if (i >= n) return;
  // edge ids are fetched 32 at a time by the node's lanes and handed round by shuffles: the row loads then depend on a
  // lane exchange, not on a second trip to memory, and several of them are in flight
  float a2 = 0.0f, a3 = 0.0f, a4 = 0.0f;
  // (the four row bounds together, then the first 32 ids of both lists together: read where each loop starts they were four
  // dependent memory round trips before the first row arrived)
  const int dlo = rowptr_dst[i], dhi = rowptr_dst[i + 1], slo = rowptr[i], shi = rowptr[i + 1];
  int ev_d = dlo + o < dhi ? perm_dst[dlo + o] : 0;
  int ev_s = slo + o < shi ? (perm ? perm[slo + o] : slo + o) : 0;
  for (int q0 = dlo; q0 < dhi; q0 += 32) {
    const int m = min(32, dhi - q0);
    const int ev = q0 == dlo ? ev_d : (o < m ? perm_dst[q0 + o] : 0);
    // (eight edges' rows in flight: the compiler does not unroll a loop of run-time length around a lane exchange, and one edge at a
    // time the loop was two loads and a full wait per edge -- a memory round trip per incident edge)
    for (int j0 = 0; j0 < m; j0 += 8) {
      float r2[8], r4[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = __shfl(ev, j0 + u < m ? j0 + u : 0, 32);
        r2[u] = c2buf[(size_t)e * TU + o];
        r4[u] = gzbuf[(size_t)e * TU + o];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (j0 + u < m) { a2 += r2[u]; a4 += r4[u]; }
    }
  }
  for (int q0 = slo; q0 < shi; q0 += 32) {
    const int m = min(32, shi - q0);
    const int ev = q0 == slo ? ev_s : (o < m ? (perm ? perm[q0 + o] : q0 + o) : 0);
    for (int j0 = 0; j0 < m; j0 += 8) {
      float r3[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) r3[u] = gzbuf[(size_t)__shfl(ev, j0 + u < m ? j0 + u : 0, 32) * TU + o];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (j0 + u < m) a3 += r3[u];
    }
  }
  gX[(size_t)i * 128 + 32 + o] = a2;
  gX[(size_t)i * 128 + 64 + o] = a3;
  gX[(size_t)i * 128 + 96 + o] = a4;
}

// The edges grouped by destination, built on the device when the caller has no such CSR: count, scan, fill (cursor order is
// whatever the hardware schedules), then every row's ids are put in ascending order so that the sums have a fixed order.
__global__ void csr_count_kernel(int E, const int *dst, int *cnt) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < E) atomicAdd(cnt + dst[e], 1);
}
__global__ void __launch_bounds__(1024) csr_scan_kernel(int n, const int *cnt, int *rowptr, int *cursor) {
  __shared__ int wsum[16], carry_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < n; base += 1024) {
    const int i = base + tid;
    const int v = i < n ? cnt[i] : 0;
    int inc = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) { const int o = __shfl_up(inc, s, 64); if (lane >= s) inc += o; }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int off = carry_s;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    if (i < n) { rowptr[i] = off + inc - v; cursor[i] = off + inc - v; }
    __syncthreads();
    if (tid == 1023) carry_s = off + inc;
    __syncthreads();
  }
  if (tid == 0) rowptr[n] = carry_s;
}
__global__ void csr_fill_kernel(int E, const int *dst, int *cursor, int *perm) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < E) perm[atomicAdd(cursor + dst[e], 1)] = e;
}
// rank sort of every row's ids (distinct), 32 lanes per row out of LDS; rows longer than CSR_SORT_MAX keep the fill order
constexpr int CSR_SORT_MAX = 512;
__global__ void __launch_bounds__(256) csr_sort_rows_kernel(int n, const int *rowptr, int *perm) {
  __shared__ int ids[8][CSR_SORT_MAX];
  const int il = threadIdx.x >> 5, o = threadIdx.x & 31;
  const int i = blockIdx.x * 8 + il;
  if (i >= n) return;
  const int lo = rowptr[i], L = rowptr[i + 1] - lo;
  if (L > CSR_SORT_MAX) return;
  for (int k = o; k < L; k += 32) ids[il][k] = perm[lo + k];
  __builtin_amdgcn_wave_barrier();                         // (a row belongs to one half-wave: LDS accesses of a wave are in order)
  for (int k = o; k < L; k += 32) {
    const int v = ids[il][k];
    int rank = 0;
    for (int j = 0; j < L; ++j) rank += ids[il][j] < v;
    perm[lo + rank] = v;
  }
}

// node linears backward: gx (in: grad wrt x', out: grad wrt x) += gX Wv; gWvT[c][c'] += sum_i x[i][c] gX[i][c'];
// gbv[c'] += sum_i gX[i][c'].  Waves walk 32-node tiles.
__global__ void __launch_bounds__(256)
gnn_t_node_lin_bwd(int n, const float *WT, const float *x0, const float *gX, float *gx, float *gWT, float *gbv) {
  __shared__ __attribute__((aligned(16))) float tx_s[4][32][36], tG_s[4][32][132];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int o = lane & 31, h = lane >> 5;
  float (*tx)[36] = tx_s[wave], (*tG)[132] = tG_s[wave];
  f32x16 aW[4] = {ZERO16, ZERO16, ZERO16, ZERO16};
  float ab[4] = {0.f, 0.f, 0.f, 0.f};
  const int ntiles = (n + 31) / 32;
  // Round 6 (last session): every global access of a tile is issued before the first one is waited for.  The compiled loops
  // were load -> s_waitcnt vmcnt(0) -> LDS store, one element at a time: 80 dependent memory round trips per tile for the two
  // operand tiles, sixteen more for the rows of WT (re-read per tile) and sixteen for gx's read-modify-write -- 38.7 us per launch
  // at n = 2 000 for 1.3 MB of traffic.  Now: the lane's 64 entries of WT are read once (registers), a tile's rows arrive as
  // 20 independent 16-byte loads per lane, gx's old values are in flight under the matrix products.  Same products, same sums.
  float4 wv[4][4];                                            // WT[o][q * 32 + h * 16 + 4 v ..]: the B operand of the second product
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int v = 0; v < 4; ++v) wv[q][v] = *reinterpret_cast<const float4 *>(WT + o * 128 + q * 32 + h * 16 + 4 * v);
  for (int tix = blockIdx.x * 4 + wave; tix < ntiles; tix += gridDim.x * 4) {
    const int i0 = tix * 32;
    float4 vx[4], vg[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {                             // x0 tile: 32 rows x 8 vectors
      const int f = lane + 64 * j, r = f >> 3;
      vx[j] = *reinterpret_cast<const float4 *>(x0 + (size_t)(i0 + r < n ? i0 + r : n - 1) * TU + 4 * (f & 7));
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {                            // gX tile: 32 rows x 32 vectors
      const int f = lane + 64 * j, r = f >> 5;
      vg[j] = *reinterpret_cast<const float4 *>(gX + (size_t)(i0 + r < n ? i0 + r : n - 1) * 128 + 4 * (f & 31));
    }
    float gold[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { const int i = i0 + drow(r, lane); gold[r] = gx[(size_t)(i < n ? i : n - 1) * TU + o]; }
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int f = lane + 64 * j, r = f >> 3;
      *reinterpret_cast<float4 *>(&tx[r][4 * (f & 7)]) = i0 + r < n ? vx[j] : z4;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int f = lane + 64 * j, r = f >> 5;
      *reinterpret_cast<float4 *>(&tG[r][4 * (f & 31)]) = i0 + r < n ? vg[j] : z4;
    }
    __builtin_amdgcn_wave_barrier();
    // gWT[c][32q + c'] : D_q[c][c'] = sum_i x[i][c] * gX[i][32q + c']
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      aW[q] = mfma32(aW[q], [&](int kk) { return tx[h * 16 + kk][o]; }, [&](int kk) { return tG[h * 16 + kk][q * 32 + o]; });
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) ab[q] += tG[h * 16 + kk][q * 32 + o];
    }
    // gx[i][c] += sum_{c'} gX[i][c'] * W[c'][c] = sum_{c'} gX[i][c'] * WT[c*128 + c']: four K = 32 blocks
    f32x16 acc = ZERO16;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      acc = mfma32(acc, [&](int kk) { return tG[o][q * 32 + h * 16 + kk]; },
                   [&](int kk) { const float4 w4 = wv[q][kk >> 2]; return (kk & 3) == 0 ? w4.x : (kk & 3) == 1 ? w4.y : (kk & 3) == 2 ? w4.z : w4.w; });
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = i0 + drow(r, lane);
      if (i < n) gx[(size_t)i * TU + o] = gold[r] + acc[r];
    }
    __builtin_amdgcn_wave_barrier();
  }
  // (per wave, as before round 6: this launch has a few dozen to ~125 wavefronts -- n / 32 tiles -- so a word of gWT sees that
  // many adds, a few microseconds; combining the waves through LDS first -- flush_acc_wg, four column blocks -- cost more in
  // barriers than it saved: 38.7 -> 57 us at n = 2 000)
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = lane & 31;
#pragma unroll
    for (int r = 0; r < 16; ++r) unsafeAtomicAdd(gWT + drow(r, lane) * 128 + q * 32 + j, aW[q][r]);
    unsafeAtomicAdd(gbv + q * 32 + o, ab[q]);
  }
}

// BatchNorm parameter gradients from the backward sums: d/dgamma = sum(g_y * zhat), d/dbeta = sum(g_y), over graphs
// (block 0: the edge BatchNorm, block 1: the node BatchNorm, whose sums follow the edge's)
__global__ void gnn_t_bn_param_grad(int G, const double *bsums_e, float *ggamma_e, float *gbeta_e, float *ggamma_v, float *gbeta_v) {
  const int c = threadIdx.x;
  if (c >= 32) return;
  const double *bsums = bsums_e + (blockIdx.x ? (size_t)G * 64 : 0);
  float *ggamma = blockIdx.x ? ggamma_v : ggamma_e, *gbeta = blockIdx.x ? gbeta_v : gbeta_e;
  double a = 0.0, b = 0.0;
  for (int g = 0; g < G; ++g) { b += bsums[((size_t)g * 32 + c) * 2]; a += bsums[((size_t)g * 32 + c) * 2 + 1]; }
  ggamma[c] = (float)a; gbeta[c] = (float)b;
}

// first linears: x0 = silu(a0), a0 = xin W^T + b  /  w0 = silu(attr * W + b)
__global__ void __launch_bounds__(256)
gnn_t_node_init_bwd(int n, int feats, const float *xin, const float *a0, const float *gx, float *gW, float *gb) {
  __shared__ float red[8][TU][9];
  const int il = threadIdx.x >> 5, o = threadIdx.x & 31;
  float accW[8] = {0, 0, 0, 0, 0, 0, 0, 0}, accb = 0.0f;
  for (int i = blockIdx.x * 8 + il; i < n; i += gridDim.x * 8) {
    const float g = gx[(size_t)i * TU + o] * t_dsilu(a0[(size_t)i * TU + o]);
    accb += g;
    for (int f = 0; f < feats; ++f) accW[f] = fmaf(g, xin[(size_t)i * feats + f], accW[f]);
  }
  // one atomic per channel and workgroup (not per thread: 64 addresses would serialise a quarter million atomics)
  for (int f = 0; f < 8; ++f) red[il][o][f] = accW[f];
  red[il][o][8] = accb;
  __syncthreads();
  if (il == 0) {
    for (int f = 0; f <= 8; ++f) {
      float v = 0.0f;
      for (int r = 0; r < 8; ++r) v += red[r][o][f];
      if (f == 8) unsafeAtomicAdd(gb + o, v);
      else if (f < feats) unsafeAtomicAdd(gW + o * feats + f, v);
    }
  }
}
__global__ void __launch_bounds__(256)
gnn_t_edge_init_bwd(int E, const float *attr, const float *W, const float *b, const float *gw, float *gW, float *gb) {
  __shared__ float red[8][TU][2];
  const int il = threadIdx.x >> 5, o = threadIdx.x & 31;
  float accW = 0.0f, accb = 0.0f;
  for (int e = blockIdx.x * 8 + il; e < E; e += gridDim.x * 8) {
    const float a = attr[e];
    const float g = gw[(size_t)e * TU + o] * t_dsilu(fmaf(a, W[o], b[o]));
    accb += g; accW = fmaf(g, a, accW);
  }
  red[il][o][0] = accW; red[il][o][1] = accb;
  __syncthreads();
  if (il == 0) {
    float vw = 0.0f, vb = 0.0f;
    for (int r = 0; r < 8; ++r) { vw += red[r][o][0]; vb += red[r][o][1]; }
    unsafeAtomicAdd(gW + o, vw);
    unsafeAtomicAdd(gb + o, vb);
  }
}

// mean / biased variance of every BatchNorm (for the running-statistics update on the host side)
__global__ void gnn_t_export_stats(int G, int count_e, int count_v, const int *edge_off, const double *fsums_all, float *out) {
  // fsums_all: [12][2 (e, v)][G][32][2]; out: [12][2][G][32][2] (mean, biased var)
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 12 * 2 * G * 32) return;
  const int which = (idx / (G * 32)) & 1;
  const int cnt = which == 0 ? edge_count(edge_off, (idx >> 5) % G, count_e) : count_v;
  const double s = fsums_all[(size_t)idx * 2], q = fsums_all[(size_t)idx * 2 + 1];
  const double m = s / cnt;
  double v = q / cnt - m * m;
  out[(size_t)idx * 2] = (float)m;
  out[(size_t)idx * 2 + 1] = (float)(v < 0.0 ? 0.0 : v);
}

struct TrainWs {
  float *a0, *x[13], *X[12], *w[13], *ze[12], *zv[12];
  double *fsums;   // [12][2][G][32][2]
  float2 *ftab;    // [12][2][G][32] (mean, rstd)
  float2 *btab;    // [2][G][32] (mean g_y, mean g_y zhat) of the layer being differentiated
  // backward scratch
  float *gx, *gw, *gX, *gmsg;
  float *c2buf, *gzbuf;   // [E][32] per-edge contributions of the layer being differentiated (gather path)
  int *csr_rowptr, *csr_perm, *csr_cursor;   // destination CSR built by the backward when the caller passes none
  double *bsums;   // [12][2][G][32][2]
  size_t total;
};
static TrainWs carve(void *base, int n, int E, int G) {
  TrainWs t;
  char *p = (char *)base;
  auto take = [&](size_t bytes) { char *r = p; p += align256(bytes); return r; };
  t.a0 = (float *)take((size_t)n * 32 * 4);
  for (int l = 0; l <= 12; ++l) t.x[l] = (float *)take((size_t)n * 32 * 4);
  for (int l = 0; l < 12; ++l) t.X[l] = (float *)take((size_t)n * 128 * 4);
  for (int l = 0; l <= 12; ++l) t.w[l] = (float *)take((size_t)E * 32 * 4);
  for (int l = 0; l < 12; ++l) t.ze[l] = (float *)take((size_t)E * 32 * 4);
  for (int l = 0; l < 12; ++l) t.zv[l] = (float *)take((size_t)n * 32 * 4);
  t.fsums = (double *)take((size_t)12 * 2 * G * 32 * 2 * 8);
  t.ftab = (float2 *)take((size_t)12 * 2 * G * 32 * 8);
  t.btab = (float2 *)take((size_t)2 * G * 32 * 8);
  t.gx = (float *)take((size_t)n * 32 * 4);
  t.gw = (float *)take((size_t)E * 32 * 4);
  t.gX = (float *)take((size_t)n * 128 * 4);
  t.gmsg = (float *)take((size_t)n * 32 * 4);
  t.c2buf = (float *)take((size_t)E * 32 * 4);
  t.gzbuf = (float *)take((size_t)E * 32 * 4);
  t.csr_rowptr = (int *)take((size_t)(n + 1) * 4);
  t.csr_perm = (int *)take((size_t)E * 4);
  t.csr_cursor = (int *)take((size_t)n * 4);
  t.bsums = (double *)take((size_t)12 * 2 * G * 32 * 2 * 8);   // per layer (cleared once per backward)
  t.total = (size_t)(p - (char *)base);
  return t;
}

}  // namespace daco

using namespace daco;

extern "C" size_t daco_gnn_train_workspace_bytes(int n, int E, int G) {
  if (n <= 0 || E <= 0 || G <= 0) return 0;
  return carve(nullptr, n, E, G).total;
}

// (ragged: the graphs' edge counts are the caller's edge_off [G + 1] on the device; E need not be a multiple of G)
static int check_train_args(const char *what, int n, int E, int feats, int G, bool ragged = false) {
  if (n <= 0 || E <= 0 || feats < 1 || feats > 8 || G <= 0 || n % G || (!ragged && E % G)) {
    set_error(ragged ? "%s: bad argument (n=%d E=%d feats=%d G=%d; n must be a multiple of G)"
                     : "%s: bad argument (n=%d E=%d feats=%d G=%d; n and E must be multiples of G)", what, n, E, feats, G);
    return DACO_E_BADARG;
  }
  return DACO_OK;
}

// The body of both forward entries.  gr: how an edge finds its graph (EqualGraphs{E / G} with edge_off = NULL, or
// RaggedGraphs{src, n / G} with the graphs' edge ranges in edge_off); the launch sequence is the same.
template <class GR>
static int train_forward_body(const char *what, void *stream, int n, int E, int feats, int G, GR gr, const int32_t *edge_off,
                              const float *x, const int32_t *src, const int32_t *dst, const int32_t *rowptr, const int32_t *perm,
                              const float *edge_attr, const float *params, float *heu, float *stats_out, const float *fixed_stats,
                              void *workspace, size_t workspace_bytes) {
  if (!x || !src || !dst || !rowptr || !edge_attr || !params || !heu || !workspace) { set_error("%s: null pointer", what); return DACO_E_BADARG; }
  if (workspace_bytes < daco_gnn_train_workspace_bytes(n, E, G)) { set_error("%s: workspace too small", what); return DACO_E_WORKSPACE; }
  hipStream_t s = (hipStream_t)stream;
  TrainWs t = carve(workspace, n, E, G);
  const int ng = n / G, Eg = E / G;                         // (Eg: the count of an edge statistic when edge_off is NULL)
  const int node_blocks = (n + 7) / 8, tile_blocks = (E + 127) / 128;
  const unsigned ew_blocks = (unsigned)(((long)E * 32 + 255) / 256);
  if (zero_async(t.fsums, (size_t)12 * 2 * G * 32 * 2 * 8, s) != hipSuccess) { set_error("zero fill failed"); return DACO_E_HIP; }
  hipLaunchKernelGGL(gnn_t_node_init, dim3(node_blocks), dim3(256), 0, s, n, feats, x, params, t.a0, t.x[0], t.X[0]);
  hipLaunchKernelGGL(gnn_t_edge_init, dim3(ew_blocks), dim3(256), 0, s, E, feats, edge_attr, params, t.w[0]);
  for (int l = 0; l < 12; ++l) {
    const float *lp = params + off_layer(feats, l);
    const float *We = lp + 32 * 128 + 128, *be = We + 1024, *gv = be + 32, *bv_ = gv + 32, *ge = bv_ + 32, *bee = ge + 32;
    double *fe = t.fsums + ((size_t)l * 2 + 0) * G * 64, *fv = t.fsums + ((size_t)l * 2 + 1) * G * 64;
    float2 *fte = t.ftab + ((size_t)l * 2 + 0) * G * 32, *ftv = t.ftab + ((size_t)l * 2 + 1) * G * 32;
    const unsigned tb = (unsigned)((2 * G * 32 + 255) / 256);
    hipLaunchKernelGGL(gnn_t_edge_pre<GR>, dim3(tile_blocks), dim3(256), 0, s, E, gr, src, dst, We, be, t.X[l], t.w[l], t.ze[l], fe);
    hipLaunchKernelGGL(gnn_t_node_pre, dim3(node_blocks), dim3(256), 0, s, n, ng, dst, rowptr, perm, t.X[l], t.w[l], t.zv[l], fv);
    if (fixed_stats) {   // evaluation-mode BatchNorm: the caller's running statistics ([12][2 (e, v)][32][2 (mean, var)])
      hipLaunchKernelGGL(gnn_t_fixed_table, dim3(tb), dim3(256), 0, s, G, fixed_stats + (size_t)l * 2 * 64, fte);
    } else {
      hipLaunchKernelGGL(gnn_t_stat_table, dim3(tb), dim3(256), 0, s, G, Eg, ng, edge_off, fe, fte, 0);      // (fv / ftv follow fe / fte)
    }
    hipLaunchKernelGGL(gnn_t_edge_post<GR>, dim3(ew_blocks), dim3(256), 0, s, E, gr, ge, bee, fte, t.w[l], t.ze[l], t.w[l + 1]);
    const float *WTn = l < 11 ? params + off_layer(feats, l + 1) : nullptr;
    hipLaunchKernelGGL(gnn_t_node_post, dim3(node_blocks), dim3(256), 0, s, n, ng, gv, bv_, ftv, t.x[l], t.zv[l], t.x[l + 1], WTn,
                       WTn ? WTn + 32 * 128 : nullptr, l < 11 ? t.X[l + 1] : nullptr);
  }
  hipLaunchKernelGGL(gnn_t_head_fwd, dim3(tile_blocks), dim3(256), 0, s, E, params + off_head(feats), t.w[12], heu);
  if (stats_out)
    hipLaunchKernelGGL(gnn_t_export_stats, dim3((12 * 2 * G * 32 + 255) / 256), dim3(256), 0, s, G, Eg, ng, edge_off, t.fsums, stats_out);
  return launch_status("gnn train forward");
}

extern "C" int daco_gnn_train_forward(void *stream, int n, int E, int feats, int G, const float *x, const int32_t *src,
                                      const int32_t *dst, const int32_t *rowptr, const int32_t *perm, const float *edge_attr,
                                      const float *params, float *heu, float *stats_out, const float *fixed_stats,
                                      void *workspace, size_t workspace_bytes) {
  if (int rc = check_train_args("daco_gnn_train_forward", n, E, feats, G)) return rc;
  return train_forward_body("daco_gnn_train_forward", stream, n, E, feats, G, EqualGraphs{E / G}, nullptr, x, src, dst, rowptr, perm,
                            edge_attr, params, heu, stats_out, fixed_stats, workspace, workspace_bytes);
}

extern "C" long daco_gnn_train_forward_ragged(void *stream, int n, int E, int feats, int G, const int32_t *edge_off, const float *x,
                                             const int32_t *src, const int32_t *dst, const int32_t *rowptr, const int32_t *perm,
                                             const float *edge_attr, const float *params, float *heu, float *stats_out,
                                             const float *fixed_stats, void *workspace, size_t workspace_bytes) {
  if (int rc = check_train_args("daco_gnn_train_forward_ragged", n, E, feats, G, true)) return rc;
  if (!edge_off || !src) { set_error("daco_gnn_train_forward_ragged: null pointer"); return DACO_E_BADARG; }
  return train_forward_body("daco_gnn_train_forward_ragged", stream, n, E, feats, G, RaggedGraphs{src, n / G}, edge_off, x, src, dst,
                            rowptr, perm, edge_attr, params, heu, stats_out, fixed_stats, workspace, workspace_bytes);
}

// The body of both backward entries (gr, edge_off: see train_forward_body).
template <class GR>
static int train_backward_body(const char *what, void *stream, int n, int E, int feats, int G, GR gr, const int32_t *edge_off,
                               const float *x, const int32_t *src, const int32_t *dst, const int32_t *rowptr, const int32_t *perm,
                               const int32_t *rowptr_dst, const int32_t *perm_dst, const float *edge_attr, const float *params,
                               const float *heu, const float *grad_heu, float *grad_params, int fixed_stats, void *workspace,
                               size_t workspace_bytes) {
  if (!x || !src || !dst || !rowptr || !edge_attr || !params || !heu || !grad_heu || !grad_params || !workspace) { set_error("%s: null pointer", what); return DACO_E_BADARG; }
  if (workspace_bytes < daco_gnn_train_workspace_bytes(n, E, G)) { set_error("%s: workspace too small", what); return DACO_E_WORKSPACE; }
  hipStream_t s = (hipStream_t)stream;
  TrainWs t = carve(workspace, n, E, G);
  const int ng = n / G, Eg = E / G;
  const int node_blocks = (n + 7) / 8;
  const int etiles = (E + 31) / 32, ntiles = (n + 31) / 32;
  // (at most one workgroup per CU: the waves walk more tiles, and fewer workgroups add into the same words of the gradient)
  const int egrid = etiles / 4 + 1 < 256 ? etiles / 4 + 1 : 256, ngrid = ntiles / 4 + 1 < 512 ? ntiles / 4 + 1 : 512;
  const size_t pfloats = off_head(feats) + HEAD_FLOATS;
  // (kernels, not memset nodes: daco_device.h zero_async)
  if (zero_async(grad_params, pfloats * 4, s) != hipSuccess || zero_async(t.gx, (size_t)n * 32 * 4, s) != hipSuccess ||
      zero_async(t.bsums, (size_t)12 * 2 * G * 64 * 8, s) != hipSuccess) { set_error("zero fill failed"); return DACO_E_HIP; }
  const bool caller_csr = rowptr_dst && perm_dst;
  const int force_gather = getenv("DACO_GNN_TRAIN_GATHER") ? atoi(getenv("DACO_GNN_TRAIN_GATHER")) : -1;   // read per call
  // (the threshold was 100 k edges before the kernels' loads were batched; measured again at the end of round 6: 20 k edges -- the
  // TSP-100 training step -- 3.37 ms with atomics, 3.30 with the gather, profiles/r06_train_step_load_batching.txt)
  const bool use_gather = force_gather >= 0 ? force_gather != 0 : (E >= 16000 || caller_csr);
  if (use_gather && !caller_csr) {
    if (zero_async(t.csr_cursor, (size_t)n * 4, s) != hipSuccess) { set_error("zero fill failed"); return DACO_E_HIP; }
    hipLaunchKernelGGL(csr_count_kernel, dim3((E + 255) / 256), dim3(256), 0, s, E, dst, t.csr_cursor);
    hipLaunchKernelGGL(csr_scan_kernel, dim3(1), dim3(1024), 0, s, n, t.csr_cursor, t.csr_rowptr, t.csr_cursor);
    hipLaunchKernelGGL(csr_fill_kernel, dim3((E + 255) / 256), dim3(256), 0, s, E, dst, t.csr_cursor, t.csr_perm);
    hipLaunchKernelGGL(csr_sort_rows_kernel, dim3((n + 7) / 8), dim3(256), 0, s, n, t.csr_rowptr, t.csr_perm);
    rowptr_dst = t.csr_rowptr;
    perm_dst = t.csr_perm;
  }
  hipLaunchKernelGGL(gnn_t_head_bwd, dim3(egrid), dim3(256), 0, s, E, params + off_head(feats), t.w[12], heu, grad_heu, t.gw,
                     grad_params + off_head(feats));
  for (int l = 11; l >= 0; --l) {
    const float *lp = params + off_layer(feats, l);
    const float *WT = lp, *We = lp + 32 * 128 + 128, *gv = We + 1024 + 32, *bv_ = gv + 32, *ge = bv_ + 32, *bee = ge + 32;
    float *glp = grad_params + off_layer(feats, l);
    float *gWT = glp, *gbv = glp + 32 * 128, *gWe = gbv + 128, *gbe = gWe + 1024, *ggv = gbe + 32, *gbv_ = ggv + 32, *gge = gbv_ + 32, *gbee = gge + 32;
    double *be_s = t.bsums + (size_t)l * 2 * G * 64, *bv_s = be_s + (size_t)G * 64;
    // the gather path pays four small CSR kernels per call and one gather launch per layer: it wins from ~100 k edges
    // (8 x TSP-500: edge_bwd 508 -> 303 + 47 us per layer); below, the f32 atomics are cheaper.  DACO_GNN_TRAIN_GATHER=0/1 forces.
    const bool gather = use_gather;
    // (atomics path: node_bwd_apply writes the x1 block of every row of gX and clears the three blocks the edges add into)
    const float2 *fte = t.ftab + ((size_t)l * 2 + 0) * G * 32, *ftv = t.ftab + ((size_t)l * 2 + 1) * G * 32;
    float2 *bte = t.btab, *btv = t.btab + (size_t)G * 32;
    const unsigned tb = (unsigned)((2 * G * 32 + 255) / 256);
    hipLaunchKernelGGL(gnn_t_bwd_stats<GR>, dim3((E + 255) / 256), dim3(256), 0, s, E, gr, ge, bee, fte, t.ze[l], t.gw, be_s);
    hipLaunchKernelGGL(gnn_t_bwd_stats<EqualGraphs>, dim3((n + 255) / 256), dim3(256), 0, s, n, EqualGraphs{ng}, gv, bv_, ftv, t.zv[l], t.gx, bv_s);
    if (fixed_stats) {   // the statistics were constants of the forward: g_z = gamma * rstd * g_y, no batch terms
      if (l == 11 && zero_async(t.btab, (size_t)2 * G * 32 * 8, s) != hipSuccess) { set_error("zero fill failed"); return DACO_E_HIP; }   // (nobody writes it in this mode)
    } else {
      hipLaunchKernelGGL(gnn_t_stat_table, dim3(tb), dim3(256), 0, s, G, Eg, ng, edge_off, be_s, bte, 1);    // (bv_s / btv follow be_s / bte)
    }
    hipLaunchKernelGGL(gnn_t_node_bwd_apply, dim3(node_blocks), dim3(256), 0, s, n, ng, rowptr, gv, bv_, ftv, btv, t.zv[l], t.gx,
                       t.gX, t.gmsg, gather ? 0 : 1);
    hipLaunchKernelGGL(gnn_t_edge_bwd<GR>, dim3(egrid), dim3(256), 0, s, E, gr, src, dst, We, ge, bee, fte, bte, t.X[l], t.w[l], t.ze[l],
                       t.gmsg, t.gw, t.gX, gWe, gbe, gather ? t.c2buf : nullptr, gather ? t.gzbuf : nullptr);
    if (gather)
      hipLaunchKernelGGL(gnn_t_gather_bwd, dim3(node_blocks), dim3(256), 0, s, n, rowptr, perm, rowptr_dst, perm_dst, t.c2buf,
                         t.gzbuf, t.gX);
    hipLaunchKernelGGL(gnn_t_node_lin_bwd, dim3(ngrid), dim3(256), 0, s, n, WT, t.x[l], t.gX, t.gx, gWT, gbv);
    hipLaunchKernelGGL(gnn_t_bn_param_grad, dim3(2), dim3(64), 0, s, G, be_s, gge, gbee, ggv, gbv_);
  }
  hipLaunchKernelGGL(gnn_t_node_init_bwd, dim3(node_blocks < 128 ? node_blocks : 128), dim3(256), 0, s, n, feats, x, t.a0, t.gx,
                     grad_params, grad_params + 32 * feats);
  const float *W0e = params + 32 * feats + 32;
  // (at most 128 workgroups: each adds once into the same 64 words, and the adds to one word are serial)
  hipLaunchKernelGGL(gnn_t_edge_init_bwd, dim3(E / 64 + 1 < 128 ? E / 64 + 1 : 128), dim3(256), 0, s, E, edge_attr, W0e, W0e + 32, t.gw,
                     grad_params + 32 * feats + 32, grad_params + 32 * feats + 64);
  return launch_status("gnn train backward");
}

extern "C" int daco_gnn_train_backward(void *stream, int n, int E, int feats, int G, const float *x, const int32_t *src,
                                       const int32_t *dst, const int32_t *rowptr, const int32_t *perm, const int32_t *rowptr_dst,
                                       const int32_t *perm_dst, const float *edge_attr, const float *params, const float *heu,
                                       const float *grad_heu, float *grad_params, int fixed_stats, void *workspace,
                                       size_t workspace_bytes) {
  if (int rc = check_train_args("daco_gnn_train_backward", n, E, feats, G)) return rc;
  return train_backward_body("daco_gnn_train_backward", stream, n, E, feats, G, EqualGraphs{E / G}, nullptr, x, src, dst, rowptr, perm,
                             rowptr_dst, perm_dst, edge_attr, params, heu, grad_heu, grad_params, fixed_stats, workspace,
                             workspace_bytes);
}

extern "C" long daco_gnn_train_backward_ragged(void *stream, int n, int E, int feats, int G, const int32_t *edge_off, const float *x,
                                              const int32_t *src, const int32_t *dst, const int32_t *rowptr, const int32_t *perm,
                                              const int32_t *rowptr_dst, const int32_t *perm_dst, const float *edge_attr,
                                              const float *params, const float *heu, const float *grad_heu, float *grad_params,
                                              int fixed_stats, void *workspace, size_t workspace_bytes) {
  if (int rc = check_train_args("daco_gnn_train_backward_ragged", n, E, feats, G, true)) return rc;
  if (!edge_off || !src) { set_error("daco_gnn_train_backward_ragged: null pointer"); return DACO_E_BADARG; }
  return train_backward_body("daco_gnn_train_backward_ragged", stream, n, E, feats, G, RaggedGraphs{src, n / G}, edge_off, x, src,
                             dst, rowptr, perm, rowptr_dst, perm_dst, edge_attr, params, heu, grad_heu, grad_params, fixed_stats,
                             workspace, workspace_bytes);
}
