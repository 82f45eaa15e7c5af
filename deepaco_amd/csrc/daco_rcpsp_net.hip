// daco_rcpsp_net.hip -- the heuristic network of rcpsp/net.py (EmbNet(depth=12, feats=5, edge_feats=2, units=32) + ParNet) in
// eval mode, for B projects of equal n, in ONE launch: input linears, 12 layers, head, `+ eps` and the write of the dense
// [B][n][n] heuristic the colony takes.  One workgroup of 512 threads per project; projects are independent, so the only
// barrier a layer needs is __syncthreads().  No cooperative launch, no grid-wide barrier, no atomics.
//
// The graph is not an edge list but a dense relation matrix [B][n][n] of uint8 codes (rcpsp_inst.py:202-222):
//   0 no edge | 1 precedence edge, attribute [1,0] | 2 unrelated pair, attribute [0,1] | 3 the sink's self-loop, attribute [0,0]
// (a code above 3 is read as 0).  Edge (i, j) lives at slot i*n + j, so mean pooling by source is a row mean over the row's
// non-zero codes (count clamped to 1) and the result needs no permutation.
//
// ---- parameter block (floats), built by deepaco_amd/rcpsp/net.py pack_params: the layout of daco_gnn.h with 64 instead of
// 32 floats for e_lin0.weight
// [0]               v_lin0.W [32][5] | v_lin0.b [32]
// then              e_lin0.W [32][2] | e_lin0.b [32]
// then 12 x layer:  WvT [32 c][128 c']  (x1|x2|x3|x4 outputs, transposed) | bv [128]
//                   We [32 o][32 c] | be [32] | bn_v scale[32] shift[32] | bn_e scale[32] shift[32]      (LAYER_FLOATS)
// then head:        W1 [32][32] b1 [32] W2 [32][32] b2 [32] W3 [32] b3 [1]                                (HEAD_FLOATS)
//
// ---- state
// LDS (dynamic, sized by n; 124.5 KB at n = 128): node states x [n][32], the four node linears X [n][128], the current layer's
// parameters (the head's after the last layer), the three initial edge vectors silu(e_lin0(attr_code)), the relation codes,
// and per wavefront a staging tile and the compacted column list of the row it works on.
// Workspace: the edge state w [n][n][32] f32 of each project, private to its workgroup, updated in place.  Layer 0 does not
// read it (its edge state is one of the three initial vectors), so what the workspace holds before the call does not matter.
//
// ---- a layer (tsp/net.py:36-46 with rcpsp's e_lin0)
// A wavefront takes rows i = wave, wave + 8, ...; it compacts the row's non-zero columns into a list (ascending j) and walks
// it two edges at a time, one per half-wavefront, lane o of a half owning channel o.  Per edge, in ONE pass: gate =
// sigmoid(w0) joins the row's aggregate BEFORE w is overwritten, w1 = We w0 on plain f32 FMAs (lane o holds row o of We in
// registers; w0's 32 channels are exchanged through the wavefront's LDS tile), w' = w0 + silu(bn_e(w1 + be + x3[i] + x4[j])).
// After the row: x'[i] = x0[i] + silu(bn_v(x1[i] + (even edges' sum + odd edges' sum) / max(count, 1))).  Then, behind a
// barrier, the next layer's parameters are loaded and X = x' WvT + bv.  The next edges' loads are issued four edges ahead.
// Every sum has a fixed order that depends on the project alone: the output is bit-identical from run to run, and a project
// gives the same bits alone as inside a batch.
#include "daco_gnn.h"
#include "daco_host.h"

namespace daco {

constexpr int RN_U = 32, RN_FEATS = 5, RN_THREADS = 512, RN_WAVES = RN_THREADS / 64, RN_AHEAD = 4;
constexpr int RN_OFF_ELIN = 32 * RN_FEATS + 32;                         // e_lin0.W [32][2] | b [32]
constexpr int RN_OFF_LAYER0 = RN_OFF_ELIN + 64 + 32;
constexpr int RN_OFF_HEAD = RN_OFF_LAYER0 + 12 * LAYER_FLOATS;
constexpr int RN_PARAM_FLOATS = RN_OFF_HEAD + HEAD_FLOATS;
constexpr size_t RN_LDS_PLAIN = 64 * 1024;                              // above: hipFuncSetAttribute

// the activations of daco_gnn.hip (defined again here: that translation unit's device code stays as it is)
constexpr float RN_L2E_HI = 1.44269502162933349609375f, RN_L2E_LO = 1.92596299e-8f, RN_LN2F = 0.693147182464599609375f;
__device__ inline float exp_neg(float x) {
  const float nx = fminf(-x, 87.0f);
  const float t = nx * RN_L2E_HI;
  const float lo = fmaf(nx, RN_L2E_LO, fmaf(nx, RN_L2E_HI, -t));
  const float e = __builtin_amdgcn_exp2f(t);
  return fmaf(e, lo * RN_LN2F, e);
}
__device__ inline float sigmoidf(float x) { return __builtin_amdgcn_rcpf(1.0f + exp_neg(x)); }
__device__ inline float silu(float x) { return x * sigmoidf(x); }

// dynamic LDS, in this order: floats first (16-byte aligned parts), then bytes
struct RnLds {
  float *xs, *X, *W, *e0, *stage;
  uint8_t *rel, *cols;
  __host__ __device__ static size_t floats(int n) { return (size_t)n * 32 + (size_t)n * 128 + LAYER_FLOATS + 96 + RN_WAVES * 2 * 3 * 32; }
  __host__ __device__ static size_t bytes(int n) { return floats(n) * sizeof(float) + (((size_t)n * n + 15) & ~(size_t)15) + RN_WAVES * 128; }
  __device__ static RnLds carve(float *base, int n) {
    RnLds s;
    s.xs = base; s.X = s.xs + n * 32; s.W = s.X + n * 128; s.e0 = s.W + LAYER_FLOATS; s.stage = s.e0 + 96;
    s.rel = reinterpret_cast<uint8_t *>(s.stage + RN_WAVES * 2 * 3 * 32);
    s.cols = s.rel + ((n * n + 15) & ~15);
    return s;
  }
};

// the row's non-zero columns, ascending, into this wavefront's list; returns their number
__device__ inline int rn_compact_row(const uint8_t *rrow, int n, uint8_t *cols, int lane) {
  const int c0 = lane < n ? rrow[lane] : 0, c1 = lane + 64 < n ? rrow[lane + 64] : 0;
  const unsigned long long m0 = __ballot(c0 != 0), m1 = __ballot(c1 != 0);
  const unsigned long long below = (1ull << lane) - 1ull;
  const int cnt0 = __popcll(m0);
  if (c0) cols[__popcll(m0 & below)] = (uint8_t)lane;
  if (c1) cols[cnt0 + __popcll(m1 & below)] = (uint8_t)(lane + 64);
  return cnt0 + __popcll(m1);
}

// dot of this half-wavefront's staged 32 channels with the 32 weights the lane holds, channel order 0..31
__device__ inline float rn_dot32(const float *st, const float (&wr)[32]) {
  float acc = 0.0f;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float4 v = *reinterpret_cast<const float4 *>(st + q * 4);
    acc = fmaf(v.x, wr[q * 4 + 0], acc);
    acc = fmaf(v.y, wr[q * 4 + 1], acc);
    acc = fmaf(v.z, wr[q * 4 + 2], acc);
    acc = fmaf(v.w, wr[q * 4 + 3], acc);
  }
  return acc;
}

// X [n][128] = xs [n][32] WvT + bv, the four linears side by side (an output's fmas in channel order)
__device__ inline void rn_node_linears(const RnLds &s, int n) {
  const int col = threadIdx.x & 127;
  const float *WT = s.W, *bv = s.W + 32 * 128;
  for (int i = threadIdx.x >> 7; i < n; i += RN_THREADS / 128) {
    float acc = bv[col];
#pragma unroll 8
    for (int c = 0; c < RN_U; ++c) acc = fmaf(s.xs[i * 32 + c], WT[c * 128 + col], acc);
    s.X[i * 128 + col] = acc;
  }
}

template <bool FIRST>
__device__ inline void rn_layer(const RnLds &s, int n, float *w) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, o = lane & 31;
  const float *We = s.W + 32 * 128 + 128, *be = We + 32 * 32, *bnv = be + 32, *bne = bnv + 64;
  float wr[32];
#pragma unroll
  for (int c = 0; c < 32; ++c) wr[c] = We[o * 32 + c];
  const float beo = be[o], sv = bnv[o], tv = bnv[32 + o], se = bne[o], te = bne[32 + o];
  float *st = s.stage + (wave * 2 + h) * 96;
  uint8_t *cols = s.cols + wave * 128;
  for (int i = wave; i < n; i += RN_WAVES) {
    const uint8_t *rrow = s.rel + i * n;
    const int cnt = rn_compact_row(rrow, n, cols, lane);
    const int T = (cnt + 1) >> 1;                       // steps: edge k = 2 t + h of the list
    float *wrow = w + (size_t)i * n * 32;
    const float x3 = s.X[i * 128 + 64 + o];
    float part = 0.0f;
    float cur[RN_AHEAD], nxt[RN_AHEAD];
#pragma unroll
    for (int q = 0; q < RN_AHEAD; ++q) {
      const int k = 2 * q + h;
      cur[q] = 0.0f;
      if (k < cnt) cur[q] = FIRST ? s.e0[(rrow[cols[k]] - 1) * 32 + o] : wrow[cols[k] * 32 + o];
    }
    for (int t0 = 0; t0 < T; t0 += RN_AHEAD) {
#pragma unroll
      for (int q = 0; q < RN_AHEAD; ++q) {
        const int k = 2 * (t0 + RN_AHEAD + q) + h;
        nxt[q] = 0.0f;
        if (k < cnt) nxt[q] = FIRST ? s.e0[(rrow[cols[k]] - 1) * 32 + o] : wrow[cols[k] * 32 + o];
      }
#pragma unroll
      for (int q = 0; q < RN_AHEAD; ++q) {
        const int k = 2 * (t0 + q) + h;
        if (k < cnt) {
          const int j = cols[k];
          const float w0 = cur[q];
          st[o] = w0;
          const float g = rn_dot32(st, wr);
          part = fmaf(sigmoidf(w0), s.X[j * 128 + 32 + o], part);
          const float y = fmaf(g + beo + x3 + s.X[j * 128 + 96 + o], se, te);
          wrow[j * 32 + o] = w0 + silu(y);
        }
      }
#pragma unroll
      for (int q = 0; q < RN_AHEAD; ++q) cur[q] = nxt[q];
    }
    // the row's aggregate: even edges' partial + odd edges' partial (the same sum in both halves)
    const float agg = (part + __shfl_xor(part, 32)) / (float)max(cnt, 1);
    if (h == 0) {
      const float y = fmaf(s.X[i * 128 + o] + agg, sv, tv);
      s.xs[i * 32 + o] += silu(y);
    }
  }
}

// head: logit = W3 silu(W2 silu(W1 w + b1) + b2) + b3, heu = sigmoid(logit) + eps; non-edges: heu = eps, logit = -inf
__device__ inline void rn_head(const RnLds &s, int n, const float *w, float eps, float *heu, float *logit, float *emb) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, o = lane & 31;
  const float *W1 = s.W, *b1 = W1 + 1024, *W2 = b1 + 32, *b2 = W2 + 1024, *W3 = b2 + 32, *b3 = W3 + 32;
  float w1r[32], w2r[32];
#pragma unroll
  for (int c = 0; c < 32; ++c) { w1r[c] = W1[o * 32 + c]; w2r[c] = W2[o * 32 + c]; }
  const float b1o = b1[o], b2o = b2[o], b3v = b3[0];
  float *st = s.stage + (wave * 2 + h) * 96;
  uint8_t *cols = s.cols + wave * 128;
  for (int i = wave; i < n; i += RN_WAVES) {
    const uint8_t *rrow = s.rel + i * n;
    for (int j = lane; j < n; j += 64)
      if (!rrow[j]) {
        heu[i * n + j] = eps;
        if (logit) logit[i * n + j] = -__builtin_inff();
      }
    const int cnt = rn_compact_row(rrow, n, cols, lane);
    const float *wrow = w + (size_t)i * n * 32;
    for (int k = h; k < cnt; k += 2) {
      const int j = cols[k];
      const float wv = wrow[j * 32 + o];
      if (emb) emb[((size_t)i * n + j) * 32 + o] = wv;
      st[o] = wv;
      const float a1 = silu(rn_dot32(st, w1r) + b1o);
      st[32 + o] = a1;
      const float a2 = silu(rn_dot32(st + 32, w2r) + b2o);
      st[64 + o] = a2;
      float sum = 0.0f;                                  // every lane of the half: the same 32 terms in channel order
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float4 v = *reinterpret_cast<const float4 *>(st + 64 + q * 4);
        const float4 u = *reinterpret_cast<const float4 *>(W3 + q * 4);
        sum = fmaf(v.x, u.x, sum); sum = fmaf(v.y, u.y, sum); sum = fmaf(v.z, u.z, sum); sum = fmaf(v.w, u.w, sum);
      }
      if (o == 0) {
        const float z = sum + b3v;
        heu[i * n + j] = sigmoidf(z) + eps;
        if (logit) logit[i * n + j] = z;
      }
    }
  }
}

__global__ void __launch_bounds__(RN_THREADS)
rcpsp_net_kernel(int n, const float *x, const uint8_t *relation, const float *params, float eps, float *heu, float *logit,
                 float *emb, float *wbase, size_t wstride) {
  extern __shared__ __attribute__((aligned(16))) float rn_lds[];
  const RnLds s = RnLds::carve(rn_lds, n);
  const int b = blockIdx.x, tid = threadIdx.x;
  x += (size_t)b * n * RN_FEATS;
  relation += (size_t)b * n * n;
  heu += (size_t)b * n * n;
  if (logit) logit += (size_t)b * n * n;
  if (emb) emb += (size_t)b * n * n * 32;
  float *w = wbase + (size_t)b * wstride;

  for (int t = tid; t < n * n; t += RN_THREADS) {
    const uint8_t c = relation[t];
    s.rel[t] = c > 3 ? 0 : c;
  }
  for (int t = tid; t < LAYER_FLOATS; t += RN_THREADS) s.W[t] = params[RN_OFF_LAYER0 + t];
  if (tid < 96) {                                       // silu(e_lin0(attr)) for the attributes [1,0], [0,1], [0,0]
    const int code = tid >> 5, o = tid & 31;
    const float *W = params + RN_OFF_ELIN, *bb = W + 64;
    float v = bb[o];
    v = fmaf(code == 0 ? 1.0f : 0.0f, W[o * 2 + 0], v);
    v = fmaf(code == 1 ? 1.0f : 0.0f, W[o * 2 + 1], v);
    s.e0[tid] = silu(v);
  }
  for (int t = tid; t < n * 32; t += RN_THREADS) {      // x = silu(v_lin0(x))
    const int i = t >> 5, o = t & 31;
    const float *W = params, *bb = params + 32 * RN_FEATS;
    float v = bb[o];
#pragma unroll
    for (int f = 0; f < RN_FEATS; ++f) v = fmaf(x[i * RN_FEATS + f], W[o * RN_FEATS + f], v);
    s.xs[t] = silu(v);
  }
  __syncthreads();
  rn_node_linears(s, n);
  __syncthreads();
  for (int l = 0; l < 12; ++l) {
    if (l == 0) rn_layer<true>(s, n, w);
    else rn_layer<false>(s, n, w);
    __syncthreads();                                    // every row's x' and w' are written; the layer's parameters are free
    if (l < 11) {
      for (int t = tid; t < LAYER_FLOATS; t += RN_THREADS) s.W[t] = params[RN_OFF_LAYER0 + (size_t)(l + 1) * LAYER_FLOATS + t];
      __syncthreads();
      rn_node_linears(s, n);
    } else {
      for (int t = tid; t < HEAD_FLOATS; t += RN_THREADS) s.W[t] = params[RN_OFF_HEAD + t];
    }
    __syncthreads();
  }
  rn_head(s, n, w, eps, heu, logit, emb);
}

}  // namespace daco

using namespace daco;

extern "C" size_t daco_rcpsp_net_param_floats(void) { return RN_PARAM_FLOATS; }

extern "C" size_t daco_rcpsp_net_workspace_bytes(int B, int n) {
  if (B <= 0 || n < 2 || n > DACO_RCPSP_NET_MAX_N) return 0;
  return (size_t)B * align256((size_t)n * n * 32 * sizeof(float));
}

extern "C" long daco_rcpsp_net_forward(void *stream, int B, int n, int feats, const float *x, const uint8_t *relation,
                                       const float *params, float eps, float *heu, float *logit, float *emb, void *workspace,
                                       size_t workspace_bytes) {
  if (B <= 0 || n < 2 || feats != RN_FEATS) {
    set_error("daco_rcpsp_net_forward: bad argument (B=%d n=%d feats=%d; feats must be %d)", B, n, feats, RN_FEATS);
    return DACO_E_BADARG;
  }
  if (!x || !relation || !params || !heu || !workspace) {
    set_error("daco_rcpsp_net_forward: null pointer");
    return DACO_E_BADARG;
  }
  if (n > DACO_RCPSP_NET_MAX_N) {
    set_error("daco_rcpsp_net_forward: n=%d exceeds DACO_RCPSP_NET_MAX_N = %d", n, DACO_RCPSP_NET_MAX_N);
    return DACO_E_TOOLARGE;
  }
  const size_t need = daco_rcpsp_net_workspace_bytes(B, n);
  if (workspace_bytes < need) {
    set_error("daco_rcpsp_net_forward: workspace %zu < %zu bytes", workspace_bytes, need);
    return DACO_E_WORKSPACE;
  }
  const size_t dyn = RnLds::bytes(n);
  if (dyn > RN_LDS_PLAIN) {
    const hipError_t e = hipFuncSetAttribute((const void *)rcpsp_net_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
    if (e != hipSuccess) return launch_status(e, "rcpsp_net_kernel (dynamic LDS)");
  }
  hipLaunchKernelGGL(rcpsp_net_kernel, dim3((unsigned)B), dim3(RN_THREADS), dyn, (hipStream_t)stream, n, x, relation, params, eps,
                     heu, logit, emb, (float *)workspace, need / B / sizeof(float));
  return launch_status("rcpsp_net_kernel");
}
