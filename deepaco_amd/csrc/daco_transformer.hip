// daco_transformer.hip -- forward of the heuristic network of mkp_transformer/net.py:9-45 for G sequences of n tokens.
//
// Reference behaviour replaced: TransformerModel.forward in eval / no-grad use (mkp_transformer/test.py:14-18):
//   x = Linear(feats, 32)(src) * sqrt(32); three post-norm nn.TransformerEncoderLayer(d_model 32, 2 heads, d_hid 32, relu,
//   dropout 0): x = LN1(x + out_proj(MHA(x))), x = LN2(x + linear2(relu(linear1(x)))) (LayerNorm eps 1e-5, biased
//   variance); ParNet 32-32-32-1 (relu, relu, sigmoid); heu / heu.max() per sequence.  float32 throughout, no library GEMM.
//
// Parameters: ONE flat float block (daco_transformer_param_floats(feats) floats), every matrix in torch's [out][in]
// row-major layout, in this order:
//   encoder.weight [32][feats], encoder.bias [32];
//   per layer l = 0, 1, 2:  self_attn.in_proj_weight [96][32] (rows 0-31 q, 32-63 k, 64-95 v), in_proj_bias [96],
//     self_attn.out_proj.weight [32][32], .bias [32], linear1.weight [32][32], .bias [32], linear2.weight [32][32],
//     .bias [32], norm1.weight [32], norm1.bias [32], norm2.weight [32], norm2.bias [32];
//   decoder_heu.lins.0.weight [32][32], .bias [32], lins.1.weight [32][32], .bias [32], lins.2.weight [1][32], .bias [1].
//
// Split into launches.  Everything except attention is per token, and a layer needs every token's K and V before any query
// finishes, so a layer is two launches: (a) one thread per token forms q, k, v (layer 0: the input projection first);
// (b) one thread per token does both heads' attention with an online softmax -- the workgroup streams K and V of the
// (sequence, head) through LDS in tiles of 128 keys (16 KB static LDS; every lane reads the same key at a time, a
// broadcast), the n x n scores are never written; every tile is summed on its own and merged into the totals, so no
// float32 chain is longer than a tile -- and then, still in registers, out_proj, residual + LayerNorm, the FFN,
// residual + LayerNorm.  After the third layer one launch per token for ParNet, one workgroup per sequence for / max:
// 1 + 3 * 2 + 2 = 9 launches, no host synchronisation.  Every linear is y_o = b_o, then y_o = fma(W[o][i], x_i, y_o) for
// i ascending (k-ordered chains; the weights are wave-uniform loads); a score is the k-ordered chain of q_d * k_d,
// times 1/4.  The 32-wide linears are plain v_fma here, not MFMA: at 21 761 parameters and n <= 1023 tokens the forward
// is bound by the dependent chain of a token's layers, not by FLOPs.
#include "daco_device.h"
#include "../../include/deepaco_hip.h"

namespace daco {

constexpr int TH = 2, THD = 16, TLAYERS = 3, TTILE = 128;
// per layer: in_w 3072, in_b 96, out_w 1024, out_b 32, l1_w 1024, l1_b 32, l2_w 1024, l2_b 32, 4 x 32 norm = 6464
constexpr int OFF_IN_W = 0, OFF_IN_B = 3072, OFF_OUT_W = 3168, OFF_OUT_B = 4192, OFF_L1_W = 4224, OFF_L1_B = 5248,
              OFF_L2_W = 5280, OFF_L2_B = 6304, OFF_N1_W = 6336, OFF_N1_B = 6368, OFF_N2_W = 6400, OFF_N2_B = 6432,
              LAYER_FLOATS = 6464;
constexpr int HEAD_FLOATS = 1024 + 32 + 1024 + 32 + 32 + 1;

__host__ __device__ inline size_t t_layer_off(int feats, int l) { return (size_t)32 * feats + 32 + (size_t)l * LAYER_FLOATS; }

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

// (a) q, k, v of one token; layer 0 forms x from the input features first
__global__ void __launch_bounds__(128)
tf_qkv_kernel(int n, int feats, int first, const float *__restrict__ src, const float *__restrict__ params,
              const float *__restrict__ lp, float *__restrict__ X, float *__restrict__ QKV) {
  const int g = blockIdx.y, tok = blockIdx.x * 128 + threadIdx.x;
  if (tok >= n) return;
  const size_t row = (size_t)g * n + tok;
  float x[32];
  if (first) {
    const float *s = src + row * feats;
    const float *W = params, *b = params + 32 * feats;
    const float scale = sqrtf(32.0f);
    for (int o = 0; o < 32; ++o) {
      float acc = b[o];
      for (int i = 0; i < feats; ++i) acc = __builtin_fmaf(W[o * feats + i], s[i], acc);
      x[o] = acc * scale;
    }
#pragma unroll
    for (int o = 0; o < 32; ++o) X[row * 32 + o] = x[o];
  } else {
#pragma unroll
    for (int o = 0; o < 32; ++o) x[o] = X[row * 32 + o];
  }
  float *out = QKV + row * 96;
  for (int blk = 0; blk < 3; ++blk) {
    float y[32];
    linear32<32>(lp + OFF_IN_W + blk * 1024, lp + OFF_IN_B + blk * 32, x, y);
#pragma unroll
    for (int o = 0; o < 32; o += 4) *reinterpret_cast<float4 *>(out + blk * 32 + o) = make_float4(y[o], y[o + 1], y[o + 2], y[o + 3]);
  }
}

// (b) attention of both heads, out_proj, residual + LN1, FFN, residual + LN2 for one token
__global__ void __launch_bounds__(128)
tf_attn_ffn_kernel(int n, const float *__restrict__ lp, const float *__restrict__ QKV, float *__restrict__ X) {
  __shared__ __attribute__((aligned(16))) float Ks[TTILE * THD];
  __shared__ __attribute__((aligned(16))) float Vs[TTILE * THD];
  const int g = blockIdx.y, tok = blockIdx.x * 128 + threadIdx.x;
  const bool live = tok < n;
  const size_t row = (size_t)g * n + (live ? tok : n - 1);
  const float *base = QKV + (size_t)g * n * 96;
  float attn[32];
  for (int h = 0; h < TH; ++h) {
    float q[THD], tot[THD];
#pragma unroll
    for (int d = 0; d < THD; ++d) { q[d] = QKV[row * 96 + h * THD + d]; tot[d] = 0.0f; }
    // Two levels of sums: a tile's keys are summed under the tile's own running maximum, starting from zero, and the tile's
    // (maximum, denominator, accumulators) are then merged into the totals.  One float32 chain over all n keys loses
    // n * eps: at n = 4095 with the pretrained block that was 2.9 x the tolerance against float64 (1024: 0.83 x); chains of
    // 128 keys plus n / 128 merges keep 0.06 x.  One tile (n <= 128): the merge is * 1 and + 0, the result
    // is bit for bit that of the single chain.
    float tmx = -__builtin_inff(), tden = 0.0f;
    for (int t0 = 0; t0 < n; t0 += TTILE) {
      __syncthreads();
      const int key = t0 + threadIdx.x;
      if (key < n) {
        const float *kr = base + (size_t)key * 96 + 32 + h * THD, *vr = base + (size_t)key * 96 + 64 + h * THD;
#pragma unroll
        for (int d = 0; d < THD; d += 4) {
          *reinterpret_cast<float4 *>(Ks + threadIdx.x * THD + d) = *reinterpret_cast<const float4 *>(kr + d);
          *reinterpret_cast<float4 *>(Vs + threadIdx.x * THD + d) = *reinterpret_cast<const float4 *>(vr + d);
        }
      }
      __syncthreads();
      const int cnt = n - t0 < TTILE ? n - t0 : TTILE;
      float acc[THD];
#pragma unroll
      for (int d = 0; d < THD; ++d) acc[d] = 0.0f;
      float mx = -__builtin_inff(), den = 0.0f;
      for (int j = 0; j < cnt; ++j) {
        float s = 0.0f;
#pragma unroll
        for (int d = 0; d < THD; ++d) s = __builtin_fmaf(q[d], Ks[j * THD + d], s);
        s = s * 0.25f;                                   // 1 / sqrt(head_dim)
        if (s > mx) {                                    // online softmax: rescale what was summed under the old maximum
          const float c = expf(mx - s);                  // (first key: exp(-inf) = 0)
          den = den * c;
#pragma unroll
          for (int d = 0; d < THD; ++d) acc[d] = acc[d] * c;
          mx = s;
        }
        const float p = expf(s - mx);
        den = den + p;
#pragma unroll
        for (int d = 0; d < THD; ++d) acc[d] = __builtin_fmaf(p, Vs[j * THD + d], acc[d]);
      }
      // merge the tile (cnt >= 1: mx is a score) into the totals; first tile: exp(-inf) = 0 times zeros
      const float m = tmx > mx ? tmx : mx;
      const float ct = expf(tmx - m), ca = expf(mx - m);
      tden = __builtin_fmaf(tden, ct, den * ca);
#pragma unroll
      for (int d = 0; d < THD; ++d) tot[d] = __builtin_fmaf(tot[d], ct, acc[d] * ca);
      tmx = m;
    }
#pragma unroll
    for (int d = 0; d < THD; ++d) attn[h * THD + d] = tot[d] / tden;
  }
  if (!live) return;                                     // (no barrier below)
  float x[32], y[32];
#pragma unroll
  for (int o = 0; o < 32; ++o) x[o] = X[row * 32 + o];
  linear32<32>(lp + OFF_OUT_W, lp + OFF_OUT_B, attn, y);
#pragma unroll
  for (int o = 0; o < 32; ++o) x[o] = x[o] + y[o];
  layer_norm32(x, lp + OFF_N1_W, lp + OFF_N1_B);
  float hdn[32];
  linear32<32>(lp + OFF_L1_W, lp + OFF_L1_B, x, hdn);
#pragma unroll
  for (int o = 0; o < 32; ++o) hdn[o] = hdn[o] > 0.0f ? hdn[o] : 0.0f;
  linear32<32>(lp + OFF_L2_W, lp + OFF_L2_B, hdn, y);
#pragma unroll
  for (int o = 0; o < 32; ++o) x[o] = x[o] + y[o];
  layer_norm32(x, lp + OFF_N2_W, lp + OFF_N2_B);
#pragma unroll
  for (int o = 0; o < 32; ++o) X[row * 32 + o] = x[o];
}

// ParNet 32-32-32-1 with a sigmoid (mkp_transformer/net.py:48-75)
__global__ void __launch_bounds__(128)
tf_head_kernel(int n, const float *__restrict__ hp, const float *__restrict__ X, float *__restrict__ raw) {
  const int g = blockIdx.y, tok = blockIdx.x * 128 + threadIdx.x;
  if (tok >= n) return;
  const size_t row = (size_t)g * n + tok;
  float x[32], y[32];
#pragma unroll
  for (int o = 0; o < 32; ++o) x[o] = X[row * 32 + o];
  linear32<32>(hp, hp + 1024, x, y);
#pragma unroll
  for (int o = 0; o < 32; ++o) x[o] = y[o] > 0.0f ? y[o] : 0.0f;
  linear32<32>(hp + 1056, hp + 2080, x, y);
#pragma unroll
  for (int o = 0; o < 32; ++o) x[o] = y[o] > 0.0f ? y[o] : 0.0f;
  float z;
  linear32<1>(hp + 2112, hp + 2144, x, &z);
  raw[row] = 1.0f / (1.0f + expf(-z));
}

// heu / heu.max() per sequence (mkp_transformer/net.py:44)
__global__ void __launch_bounds__(256)
tf_max_div_kernel(int n, const float *__restrict__ raw, float *__restrict__ out) {
  __shared__ float red[256];
  const int g = blockIdx.x;
  float mx = -__builtin_inff();
  for (int i = threadIdx.x; i < n; i += 256) mx = fmaxf(mx, raw[(size_t)g * n + i]);
  red[threadIdx.x] = mx;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  mx = red[0];
  for (int i = threadIdx.x; i < n; i += 256) out[(size_t)g * n + i] = raw[(size_t)g * n + i] / mx;
}

}  // namespace daco

using namespace daco;

constexpr int TF_MAX_FEATS = 16, TF_MAX_TOKENS = 4096;

extern "C" size_t daco_transformer_param_floats(int feats) {
  if (feats < 1 || feats > TF_MAX_FEATS) return 0;
  return (size_t)32 * feats + 32 + (size_t)TLAYERS * LAYER_FLOATS + HEAD_FLOATS;
}

extern "C" size_t daco_transformer_workspace_bytes(int G, int n) {
  if (G <= 0 || n <= 0) return 0;
  return (size_t)G * n * (32 + 96 + 1) * sizeof(float);
}

extern "C" int daco_transformer_forward(void *stream, int G, int n, int feats, const float *src, const float *params,
                                        size_t param_floats, float *out, void *workspace, size_t workspace_bytes) {
  if (G <= 0 || n <= 0 || !src || !params || !out || !workspace) { set_error("daco_transformer_forward: bad argument (G=%d n=%d)", G, n); return DACO_E_BADARG; }
  if (feats < 1 || feats > TF_MAX_FEATS) { set_error("daco_transformer_forward: 1 <= feats <= %d (feats=%d)", TF_MAX_FEATS, feats); return DACO_E_BADARG; }
  if (n > TF_MAX_TOKENS || G > 65535) { set_error("daco_transformer_forward: n=%d tokens exceed %d (or G=%d > 65535)", n, TF_MAX_TOKENS, G); return DACO_E_TOOLARGE; }
  if (param_floats != daco_transformer_param_floats(feats)) { set_error("daco_transformer_forward: %zu parameter floats, the layout has %zu", param_floats, daco_transformer_param_floats(feats)); return DACO_E_BADARG; }
  const size_t need = daco_transformer_workspace_bytes(G, n);
  if (workspace_bytes < need) { set_error("daco_transformer_forward: workspace %zu < %zu bytes", workspace_bytes, need); return DACO_E_WORKSPACE; }
  hipStream_t s = (hipStream_t)stream;
  float *X = (float *)workspace, *QKV = X + (size_t)G * n * 32, *raw = QKV + (size_t)G * n * 96;
  dim3 grid((unsigned)((n + 127) / 128), (unsigned)G), block(128);
  for (int l = 0; l < TLAYERS; ++l) {
    const float *lp = params + t_layer_off(feats, l);
    hipLaunchKernelGGL(tf_qkv_kernel, grid, block, 0, s, n, feats, l == 0 ? 1 : 0, src, params, lp, X, QKV);
    hipLaunchKernelGGL(tf_attn_ffn_kernel, grid, block, 0, s, n, lp, QKV, X);
  }
  hipLaunchKernelGGL(tf_head_kernel, grid, block, 0, s, n, params + t_layer_off(feats, TLAYERS), X, raw);
  hipLaunchKernelGGL(tf_max_div_kernel, dim3((unsigned)G), dim3(256), 0, s, n, raw, out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error("transformer kernels launch: %s", hipGetErrorString(e)); return DACO_E_HIP; }
  return DACO_OK;
}
