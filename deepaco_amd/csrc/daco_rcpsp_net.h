// daco_rcpsp_net.h -- what daco_rcpsp_net.hip (eval-mode forward) and daco_rcpsp_net_train.hip (training forward and backward)
// share: the layout of the flat parameter block, the carve of the dynamic LDS, the device helpers that both directions are made
// of, and the host side's refusals.  The two .hip files hold only their kernels and entry points.
#pragma once
#include "daco_gnn.h"
#include "daco_host.h"

namespace daco {

// ---- parameter block (floats), built by the walk of deepaco_amd/net.py (BlockNet._slots, rcpsp.net.Net uses it): the layout of daco_gnn.h
// with 64 instead of 32 floats for e_lin0.weight
// [0]               v_lin0.W [32][5] | v_lin0.b [32]
// then              e_lin0.W [32][2] | e_lin0.b [32]                                                      (RN_OFF_ELIN)
// then 12 x layer:  WvT [32 c][128 c']  (x1|x2|x3|x4 outputs, transposed) | bv [128]                       (RN_OFF_LAYER0)
//                   We [32 o][32 c] | be [32] | bn_v [32][32] | bn_e [32][32]                              (LAYER_FLOATS)
// then head:        W1 [32][32] b1 [32] W2 [32][32] b2 [32] W3 [32] b3 [1]                                 (RN_OFF_HEAD, HEAD_FLOATS)
// A BatchNorm slot holds the folded scale | shift in eval mode and gamma | beta in training mode.  The gradient block of the
// backward has the same layout, d/dgamma and d/dbeta in those slots.
constexpr int RN_FEATS = 5, RN_THREADS = 512, RN_WAVES = RN_THREADS / 64, RN_SLOTS = RN_THREADS / 32, RN_DEPTH = 12;
constexpr int RN_OFF_ELIN = 32 * RN_FEATS + 32;
constexpr int RN_OFF_LAYER0 = RN_OFF_ELIN + 64 + 32;
constexpr int RN_OFF_HEAD = RN_OFF_LAYER0 + RN_DEPTH * LAYER_FLOATS;
constexpr int RN_PARAM_FLOATS = RN_OFF_HEAD + HEAD_FLOATS;
constexpr int RN_L_BV = 32 * 128, RN_L_WE = RN_L_BV + 128, RN_L_BE = RN_L_WE + 1024, RN_L_BNV = RN_L_BE + 32, RN_L_BNE = RN_L_BNV + 64;
constexpr int RN_H_B1 = 1024, RN_H_W2 = 1056, RN_H_B2 = 2080, RN_H_W3 = 2112, RN_H_B3 = 2144;
constexpr size_t RN_LDS_PLAIN = 64 * 1024, RN_LDS_MAX = 160 * 1024;     // above PLAIN: hipFuncSetAttribute; MAX: a workgroup's

// ---- dynamic LDS, sized by n (124.5 KB at n = 128, 133 KB with the training parts): node states xs [n][32], the four node
// linears X [n][128], the current layer's parameters W (the head's after the last layer), the three initial edge vectors
// e0 = silu(e_lin0(attr_code)), per (wavefront, half) a staging tile; the training kernels' float64 reduction block and row
// counts; the relation codes, and per wavefront the compacted list of the row or column it works on.  Floats first (16-byte
// aligned parts), then float64, ints, bytes.
struct RnLds {
  float *xs, *X, *W, *e0, *stage;
  double *red;                                                          // training only
  int *rowcnt;                                                          // training only
  uint8_t *rel, *cols;
  __host__ __device__ static size_t floats(int n) { return (size_t)n * 160 + LAYER_FLOATS + 96 + RN_WAVES * 2 * 96; }
  __host__ __device__ static size_t bytes(int n, bool train) {
    return floats(n) * sizeof(float) + (train ? RN_SLOTS * 32 * 2 * sizeof(double) + 128 * sizeof(int) : 0) +
           (((size_t)n * n + 15) & ~(size_t)15) + RN_WAVES * 128;
  }
  __device__ static RnLds carve(float *base, int n, bool train) {
    RnLds s;
    s.xs = base; s.X = s.xs + n * 32; s.W = s.X + n * 128; s.e0 = s.W + LAYER_FLOATS; s.stage = s.e0 + 96;
    float *end = s.stage + RN_WAVES * 2 * 96;
    s.red = train ? reinterpret_cast<double *>(end) : nullptr;
    s.rowcnt = train ? reinterpret_cast<int *>(s.red + RN_SLOTS * 32 * 2) : nullptr;
    s.rel = train ? reinterpret_cast<uint8_t *>(s.rowcnt + 128) : reinterpret_cast<uint8_t *>(end);
    s.cols = s.rel + ((n * n + 15) & ~15);
    return s;
  }
};
static_assert((LAYER_FLOATS + 96 + RN_WAVES * 2 * 96) % 2 == 0, "the float64 block must be 8-byte aligned");

// ---- device helpers
__device__ inline void rn_load_floats(float *dst, const float *src, int count) {
  for (int t = threadIdx.x; t < count; t += RN_THREADS) dst[t] = src[t];
}

// the relation codes into LDS, a code above 3 read as 0
__device__ inline void rn_load_relation(const RnLds &s, int n, const uint8_t *relation) {
  for (int t = threadIdx.x; t < n * n; t += RN_THREADS) {
    const uint8_t c = relation[t];
    s.rel[t] = c > 3 ? 0 : c;
  }
}

// e0 = silu(e_lin0(attr)) for the attributes [1,0], [0,1], [0,0] of the codes 1, 2, 3
__device__ inline void rn_edge_init(const RnLds &s, const float *params) {
  const int tid = threadIdx.x;
  if (tid < 96) {
    const int code = tid >> 5, o = tid & 31;
    const float *W = params + RN_OFF_ELIN, *bb = W + 64;
    float v = bb[o];
    v = fmaf(code == 0 ? 1.0f : 0.0f, W[o * 2 + 0], v);
    v = fmaf(code == 1 ? 1.0f : 0.0f, W[o * 2 + 1], v);
    s.e0[tid] = silu(v);
  }
}

// xs = silu(v_lin0(x))
__device__ inline void rn_input_nodes(const RnLds &s, int n, const float *x, const float *params) {
  for (int t = threadIdx.x; t < n * 32; t += RN_THREADS) {
    const int i = t >> 5, o = t & 31;
    const float *W = params, *bb = params + 32 * RN_FEATS;
    float v = bb[o];
#pragma unroll
    for (int f = 0; f < RN_FEATS; ++f) v = fmaf(x[i * RN_FEATS + f], W[o * RN_FEATS + f], v);
    s.xs[t] = silu(v);
  }
}

// the non-zero entries of a row (stride 1) or a column (stride n), ascending, into this wavefront's list; returns their number
__device__ inline int rn_compact(const uint8_t *first, int stride, int n, uint8_t *list, int lane) {
  const int c0 = lane < n ? first[lane * stride] : 0, c1 = lane + 64 < n ? first[(lane + 64) * stride] : 0;
  const unsigned long long m0 = __ballot(c0 != 0), m1 = __ballot(c1 != 0);
  const unsigned long long below = (1ull << lane) - 1ull;
  const int cnt0 = __popcll(m0);
  if (c0) list[__popcll(m0 & below)] = (uint8_t)lane;
  if (c1) list[cnt0 + __popcll(m1 & below)] = (uint8_t)(lane + 64);
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
  const float *WT = s.W, *bv = s.W + RN_L_BV;
  for (int i = threadIdx.x >> 7; i < n; i += RN_THREADS / 128) {
    float acc = bv[col];
#pragma unroll 8
    for (int c = 0; c < 32; ++c) acc = fmaf(s.xs[i * 32 + c], WT[c * 128 + col], acc);
    s.X[i * 128 + col] = acc;
  }
}

// head: logit = W3 silu(W2 silu(W1 w + b1) + b2) + b3, heu = sigmoid(logit) + eps; non-edges: heu = eps, logit = -inf.
// `logit` and `emb` (the head's input, [n][n][32]) are optional.
__device__ inline void rn_head(const RnLds &s, int n, const float *w, float eps, float *heu, float *logit, float *emb) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, o = lane & 31;
  const float *W1 = s.W, *b1 = s.W + RN_H_B1, *W2 = s.W + RN_H_W2, *b2 = s.W + RN_H_B2, *W3 = s.W + RN_H_W3, *b3 = s.W + RN_H_B3;
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
    const int cnt = rn_compact(rrow, 1, n, cols, lane);
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

// ---- host side
// the size functions' guard: 0 bytes for a batch no entry point takes
inline bool rn_sizes_ok(int B, int n) { return B > 0 && n >= 2 && n <= DACO_RCPSP_NET_MAX_N; }

// an entry point's refusals, in this order; `pointers`: every required pointer is there
inline long rn_check(const char *who, int B, int n, int feats, bool pointers, bool train) {
  if (B <= 0 || n < 2 || feats != RN_FEATS) {
    set_error("%s: bad argument (B=%d n=%d feats=%d; feats must be %d)", who, B, n, feats, RN_FEATS);
    return DACO_E_BADARG;
  }
  if (!pointers) {
    set_error("%s: null pointer", who);
    return DACO_E_BADARG;
  }
  if (n > DACO_RCPSP_NET_MAX_N) {
    set_error("%s: n=%d exceeds DACO_RCPSP_NET_MAX_N = %d", who, n, DACO_RCPSP_NET_MAX_N);
    return DACO_E_TOOLARGE;
  }
  if (RnLds::bytes(n, train) > RN_LDS_MAX) {              // (cannot happen for n <= 128: 133 KB at n = 128)
    set_error("%s: n=%d needs %zu bytes of LDS, a workgroup has %zu", who, n, RnLds::bytes(n, train), RN_LDS_MAX);
    return DACO_E_TOOLARGE;
  }
  return DACO_OK;
}

// a kernel whose dynamic LDS exceeds 64 KB has to be told so before its launch
template <typename K>
inline long rn_lds_attr(K kernel, size_t dyn, const char *what) {
  if (dyn > RN_LDS_PLAIN) {
    const hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
    if (e != hipSuccess) return launch_status(e, what);
  }
  return DACO_OK;
}

}  // namespace daco
