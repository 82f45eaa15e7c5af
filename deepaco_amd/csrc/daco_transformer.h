// daco_transformer.h -- what daco_transformer.hip (forward, training forward) and daco_transformer_train.hip (backward) share:
// the layout of the flat parameter block, the layout of the `saved` buffer of the training forward, the per-token helpers.
#pragma once
#include "daco_host.h"

namespace daco {

constexpr int TH = 2, THD = 16, TLAYERS = 3, TTILE = 128;
// per layer: in_w 3072, in_b 96, out_w 1024, out_b 32, l1_w 1024, l1_b 32, l2_w 1024, l2_b 32, 4 x 32 norm = 6464
constexpr int OFF_IN_W = 0, OFF_IN_B = 3072, OFF_OUT_W = 3168, OFF_OUT_B = 4192, OFF_L1_W = 4224, OFF_L1_B = 5248,
              OFF_L2_W = 5280, OFF_L2_B = 6304, OFF_N1_W = 6336, OFF_N1_B = 6368, OFF_N2_W = 6400, OFF_N2_B = 6432,
              LAYER_FLOATS = 6464;
constexpr int HEAD_FLOATS = 1024 + 32 + 1024 + 32 + 32 + 1;
constexpr int TF_MAX_FEATS = 16, TF_MAX_TOKENS = 4096;

__host__ __device__ inline size_t t_layer_off(int feats, int l) { return (size_t)32 * feats + 32 + (size_t)l * LAYER_FLOATS; }

// The `saved` buffer of daco_transformer_forward_train, N = G * n tokens, in floats.  Per layer l (SV_LAYER * N floats each,
// every array [N][width]): the layer's input X_l, q/k/v, the attention output O (both heads, before out_proj), r1 = X_l +
// out_proj(O) (the input of LayerNorm 1), the ReLU input of the FFN, r2 (the input of LayerNorm 2).  Then the encoder's
// output X_3, ParNet's two hidden rows before their ReLU, the raw sigmoid; then per layer and (token, head) the
// log-sum-exp of the scores; then per sequence the maximum and the first index attaining it (an int32 in a float's place).
// 3 * 256 + 97 + 3 * 2 = 871 floats per token, + 2 per sequence; every array that is read as float4 starts at a multiple
// of 32 N floats.  Recomputed by the backward instead of saved: LayerNorm's mean and rstd and its output (from r1 / r2, by
// the forward's own code), the ReLU outputs, the softmax probabilities (from q, k and the log-sum-exp).
constexpr int SV_X = 0, SV_QKV = 32, SV_O = 128, SV_R1 = 160, SV_HPRE = 192, SV_R2 = 224, SV_LAYER = 256;
constexpr int SV_HX = 0, SV_H1 = 32, SV_H2 = 64, SV_RAW = 96, SV_HEAD = 97;
constexpr int SV_TOKEN = TLAYERS * (SV_LAYER + 2) + SV_HEAD;

struct SavedLayer { float *X, *QKV, *O, *R1, *HPRE, *R2, *LSE; };
__host__ __device__ inline SavedLayer saved_layer(float *saved, size_t N, int l) {
  float *b = saved + (size_t)l * SV_LAYER * N;
  float *lse = saved + ((size_t)TLAYERS * SV_LAYER + SV_HEAD + 2 * (size_t)l) * N;
  return SavedLayer{b + SV_X * N, b + SV_QKV * N, b + SV_O * N, b + SV_R1 * N, b + SV_HPRE * N, b + SV_R2 * N, lse};
}
struct SavedHead { float *X, *H1, *H2, *RAW, *MX; int *AMAX; };
__host__ __device__ inline SavedHead saved_head(float *saved, size_t N, int G) {
  float *b = saved + (size_t)TLAYERS * SV_LAYER * N;
  float *mx = saved + (size_t)SV_TOKEN * N;
  return SavedHead{b + SV_HX * N, b + SV_H1 * N, b + SV_H2 * N, b + SV_RAW * N, mx, reinterpret_cast<int *>(mx + G)};
}

// y[0..NO) = W x + b, W [NO][32] row-major
template <int NO>
__device__ inline void linear32(const float *__restrict__ W, const float *__restrict__ b, const float (&x)[32], float *y) {
#pragma unroll 4
  for (int o = 0; o < NO; ++o) {
    float acc = b[o];
#pragma unroll
    for (int i = 0; i < 32; ++i) acc = __builtin_fmaf(W[o * 32 + i], x[i], acc);
    y[o] = acc;
  }
}

// LayerNorm over 32 values in place: mean, biased variance, (x - mean) / sqrt(var + 1e-5) * w + b
__device__ inline void layer_norm32(float (&x)[32], const float *__restrict__ w, const float *__restrict__ b) {
  float mean = 0.0f;
#pragma unroll
  for (int i = 0; i < 32; ++i) mean = mean + x[i];
  mean = mean * (1.0f / 32.0f);
  float var = 0.0f;
#pragma unroll
  for (int i = 0; i < 32; ++i) { const float d = x[i] - mean; var = __builtin_fmaf(d, d, var); }
  const float rstd = 1.0f / sqrtf(var * (1.0f / 32.0f) + 1e-5f);
#pragma unroll
  for (int i = 0; i < 32; ++i) x[i] = __builtin_fmaf((x[i] - mean) * rstd, w[i], b[i]);
}

}  // namespace daco

// the argument checks daco_transformer_forward_train and daco_transformer_backward share (daco_transformer.hip)
int tf_check_train_args(const char *who, int G, int n, int feats, size_t param_floats, size_t saved_floats,
                        bool needs_workspace, size_t workspace_bytes);
