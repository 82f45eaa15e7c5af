// daco_gnn.h -- the heuristic network's parameter block, shared by the inference kernels (daco_gnn.hip) and the training
// kernels (daco_gnn_train.hip, whose gradient block has the same layout).
#pragma once
#include "daco_device.h"

namespace daco {

// ---- parameter block layout (floats), built by the host: the one walk deepaco_amd/net.py BlockNet._slots
// [0]               v_lin0.W [32][feats] | v_lin0.b [32]
// then              e_lin0.W [32]        | e_lin0.b [32]
// then 12 x layer:  WvT [32 c][128 c']  (x1|x2|x3|x4 outputs, transposed) | bv [128]
//                   We [32 o][32 c] | be [32] | bn_v scale[32] shift[32] | bn_e scale[32] shift[32]
// then head:        W1 [32][32] b1 [32] W2 [32][32] b2 [32] W3 [32] b3 [1]
constexpr int LAYER_FLOATS = 32 * 128 + 128 + 32 * 32 + 32 + 4 * 32;
__host__ __device__ inline size_t off_layer(int feats, int l) { return (size_t)32 * feats + 32 + 64 + (size_t)l * LAYER_FLOATS; }
__host__ __device__ inline size_t off_head(int feats) { return off_layer(feats, 12); }
constexpr int HEAD_FLOATS = 2 * (32 * 32 + 32) + 32 + 1;

// ---- activations of the inference kernels and of the RCPSP network (daco_gnn_train.hip keeps its own expf-based family:
// different arithmetic).  e^-x in six full-rate instructions instead of libm's twelve (the two activations are evaluated
// 2*E*32 times per layer and were most of a layer's VALU work): t = -x*log2(e) as the rounded product plus its exact residual
// (two fmas, the second adds the low word of log2 e), 2^t on the hardware exponential (its range reduction is exact),
// first-order correction for the residual: ~1 ulp, like libm.  1/(1+e^-x) with the hardware reciprocal (1 ulp).
constexpr float L2E_HI = 1.44269502162933349609375f, L2E_LO = 1.92596299e-8f, LN2F = 0.693147182464599609375f;
__device__ inline float exp_neg(float x) {
  const float nx = fminf(-x, 87.0f);                      // beyond: e^-x > 1e37, sigmoid and silu are 0 to f32 either way
  const float t = nx * L2E_HI;
  const float lo = fmaf(nx, L2E_LO, fmaf(nx, L2E_HI, -t));
  const float e = __builtin_amdgcn_exp2f(t);
  return fmaf(e, lo * LN2F, e);
}
__device__ inline float sigmoidf(float x) { return __builtin_amdgcn_rcpf(1.0f + exp_neg(x)); }
__device__ inline float silu(float x) { return x * sigmoidf(x); }
__device__ inline float dsilu(float x) {                  // d silu / dx
  const float s = sigmoidf(x);
  return s * fmaf(x, 1.0f - s, 1.0f);
}

// row of a 32 x 32 MFMA output tile that accumulator register r of `lane` holds
__device__ inline int drow(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

}  // namespace daco
