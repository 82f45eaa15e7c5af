// daco_rcpsp_net.hip -- the heuristic network of rcpsp/net.py (EmbNet(depth=12, feats=5, edge_feats=2, units=32) + ParNet) in
// eval mode, for B projects of equal n, in ONE launch: input linears, 12 layers, head, `+ eps` and the write of the dense
// [B][n][n] heuristic the colony takes.  One workgroup of 512 threads per project; projects are independent, so the only
// barrier a layer needs is __syncthreads().  No cooperative launch, no grid-wide barrier, no atomics.  This file holds the
// eval-mode layer, the kernel and its entry point; the parameter block's layout, the LDS carve, the device helpers (input
// linears, row compaction, node linears, head) and the host side's refusals are in daco_rcpsp_net.h, shared with the training
// kernels of daco_rcpsp_net_train.hip.
//
// The graph is not an edge list but a dense relation matrix [B][n][n] of uint8 codes (rcpsp_inst.py:202-222):
//   0 no edge | 1 precedence edge, attribute [1,0] | 2 unrelated pair, attribute [0,1] | 3 the sink's self-loop, attribute [0,0]
// (a code above 3 is read as 0).  Edge (i, j) lives at slot i*n + j, so mean pooling by source is a row mean over the row's
// non-zero codes (count clamped to 1) and the result needs no permutation.
//
// ---- state
// LDS (RnLds of daco_rcpsp_net.h, without its training parts): 124.5 KB at n = 128.
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
#include "daco_rcpsp_net.h"

namespace daco {

constexpr int RN_AHEAD = 4;                                              // edges whose loads are in flight

template <bool FIRST>
__device__ inline void rn_layer(const RnLds &s, int n, float *w) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, o = lane & 31;
  const float *We = s.W + RN_L_WE, *be = s.W + RN_L_BE, *bnv = s.W + RN_L_BNV, *bne = s.W + RN_L_BNE;
  float wr[32];
#pragma unroll
  for (int c = 0; c < 32; ++c) wr[c] = We[o * 32 + c];
  const float beo = be[o], sv = bnv[o], tv = bnv[32 + o], se = bne[o], te = bne[32 + o];
  float *st = s.stage + (wave * 2 + h) * 96;
  uint8_t *cols = s.cols + wave * 128;
  for (int i = wave; i < n; i += RN_WAVES) {
    const uint8_t *rrow = s.rel + i * n;
    const int cnt = rn_compact(rrow, 1, n, cols, lane);
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


__global__ void __launch_bounds__(RN_THREADS)
rcpsp_net_kernel(int n, const float *x, const uint8_t *relation, const float *params, float eps, float *heu, float *logit,
                 float *emb, float *wbase, size_t wstride) {
  extern __shared__ __attribute__((aligned(16))) float rn_lds[];
  const RnLds s = RnLds::carve(rn_lds, n, false);
  const int b = blockIdx.x;
  x += (size_t)b * n * RN_FEATS;
  relation += (size_t)b * n * n;
  heu += (size_t)b * n * n;
  if (logit) logit += (size_t)b * n * n;
  if (emb) emb += (size_t)b * n * n * 32;
  float *w = wbase + (size_t)b * wstride;

  rn_load_relation(s, n, relation);
  rn_load_floats(s.W, params + RN_OFF_LAYER0, LAYER_FLOATS);
  rn_edge_init(s, params);
  rn_input_nodes(s, n, x, params);
  __syncthreads();
  rn_node_linears(s, n);
  __syncthreads();
  for (int l = 0; l < RN_DEPTH; ++l) {
    if (l == 0) rn_layer<true>(s, n, w);
    else rn_layer<false>(s, n, w);
    __syncthreads();                                    // every row's x' and w' are written; the layer's parameters are free
    if (l < RN_DEPTH - 1) {
      rn_load_floats(s.W, params + RN_OFF_LAYER0 + (size_t)(l + 1) * LAYER_FLOATS, LAYER_FLOATS);
      __syncthreads();
      rn_node_linears(s, n);
    } else {
      rn_load_floats(s.W, params + RN_OFF_HEAD, HEAD_FLOATS);
    }
    __syncthreads();
  }
  rn_head(s, n, w, eps, heu, logit, emb);
}

}  // namespace daco

using namespace daco;

extern "C" size_t daco_rcpsp_net_param_floats(void) { return RN_PARAM_FLOATS; }

extern "C" size_t daco_rcpsp_net_workspace_bytes(int B, int n) {
  if (!rn_sizes_ok(B, n)) return 0;
  return (size_t)B * align256((size_t)n * n * 32 * sizeof(float));
}

extern "C" long daco_rcpsp_net_forward(void *stream, int B, int n, int feats, const float *x, const uint8_t *relation,
                                       const float *params, float eps, float *heu, float *logit, float *emb, void *workspace,
                                       size_t workspace_bytes) {
  const char *who = "daco_rcpsp_net_forward";
  if (const long rc = rn_check(who, B, n, feats, x && relation && params && heu && workspace, false)) return rc;
  const size_t need = daco_rcpsp_net_workspace_bytes(B, n);
  if (workspace_bytes < need) {
    set_error("%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    return DACO_E_WORKSPACE;
  }
  const size_t dyn = RnLds::bytes(n, false);
  if (const long rc = rn_lds_attr(rcpsp_net_kernel, dyn, "rcpsp_net_kernel (dynamic LDS)")) return rc;
  hipLaunchKernelGGL(rcpsp_net_kernel, dim3((unsigned)B), dim3(RN_THREADS), dyn, (hipStream_t)stream, n, x, relation, params, eps,
                     heu, logit, emb, (float *)workspace, need / B / sizeof(float));
  return launch_status("rcpsp_net_kernel");
}
