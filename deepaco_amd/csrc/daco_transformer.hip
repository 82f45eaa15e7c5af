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
//
// Training forward (daco_transformer_forward_train): the same kernels instantiated with SAVE.  Same arithmetic -- the output is
// bit for bit the no-grad forward's -- and every intermediate the backward (daco_transformer_train.hip) needs goes to a
// caller-owned `saved` buffer, 871 floats per token + 2 per sequence (layout: daco_transformer.h): layer inputs, q/k/v, the
// attention output, both LayerNorm inputs, the ReLU input, the log-sum-exp of every (token, head), ParNet's hidden rows, the
// raw sigmoid, every sequence's maximum and the first index attaining it.  X and QKV live in `saved` there: the training
// forward needs no scratch, its workspace argument may be NULL / 0 bytes.
#include "daco_transformer.h"

namespace daco {

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
// SAVE (the training forward): the same arithmetic, and O, r1, the ReLU input, r2 and the log-sum-exp of every (token, head)
// go to the `saved` buffer (daco_transformer.h); X is the layer's input, Xout its output (no-grad forward: Xout == X).
template <bool SAVE>
__global__ void __launch_bounds__(128)
tf_attn_ffn_kernel(int n, const float *__restrict__ lp, const float *__restrict__ QKV, float *X, float *Xout,
                   float *__restrict__ svO, float *__restrict__ svR1, float *__restrict__ svH, float *__restrict__ svR2,
                   float *__restrict__ svLse) {
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
    if (SAVE && live) svLse[row * 2 + h] = tmx + logf(tden);
  }
  if (!live) return;                                     // (no barrier below)
  if (SAVE) {
#pragma unroll
    for (int o = 0; o < 32; ++o) svO[row * 32 + o] = attn[o];
  }
  float x[32], y[32];
#pragma unroll
  for (int o = 0; o < 32; ++o) x[o] = X[row * 32 + o];
  linear32<32>(lp + OFF_OUT_W, lp + OFF_OUT_B, attn, y);
#pragma unroll
  for (int o = 0; o < 32; ++o) x[o] = x[o] + y[o];
  if (SAVE) {
#pragma unroll
    for (int o = 0; o < 32; ++o) svR1[row * 32 + o] = x[o];
  }
  layer_norm32(x, lp + OFF_N1_W, lp + OFF_N1_B);
  float hdn[32];
  linear32<32>(lp + OFF_L1_W, lp + OFF_L1_B, x, hdn);
  if (SAVE) {
#pragma unroll
    for (int o = 0; o < 32; ++o) svH[row * 32 + o] = hdn[o];
  }
#pragma unroll
  for (int o = 0; o < 32; ++o) hdn[o] = hdn[o] > 0.0f ? hdn[o] : 0.0f;
  linear32<32>(lp + OFF_L2_W, lp + OFF_L2_B, hdn, y);
#pragma unroll
  for (int o = 0; o < 32; ++o) x[o] = x[o] + y[o];
  if (SAVE) {
#pragma unroll
    for (int o = 0; o < 32; ++o) svR2[row * 32 + o] = x[o];
  }
  layer_norm32(x, lp + OFF_N2_W, lp + OFF_N2_B);
#pragma unroll
  for (int o = 0; o < 32; ++o) Xout[row * 32 + o] = x[o];
}

// ParNet 32-32-32-1 with a sigmoid (mkp_transformer/net.py:48-75)
template <bool SAVE>
__global__ void __launch_bounds__(128)
tf_head_kernel(int n, const float *__restrict__ hp, const float *__restrict__ X, float *__restrict__ raw,
               float *__restrict__ svH1, float *__restrict__ svH2) {
  const int g = blockIdx.y, tok = blockIdx.x * 128 + threadIdx.x;
  if (tok >= n) return;
  const size_t row = (size_t)g * n + tok;
  float x[32], y[32];
#pragma unroll
  for (int o = 0; o < 32; ++o) x[o] = X[row * 32 + o];
  linear32<32>(hp, hp + 1024, x, y);
  if (SAVE) {
#pragma unroll
    for (int o = 0; o < 32; ++o) svH1[row * 32 + o] = y[o];
  }
#pragma unroll
  for (int o = 0; o < 32; ++o) x[o] = y[o] > 0.0f ? y[o] : 0.0f;
  linear32<32>(hp + 1056, hp + 2080, x, y);
  if (SAVE) {
#pragma unroll
    for (int o = 0; o < 32; ++o) svH2[row * 32 + o] = y[o];
  }
#pragma unroll
  for (int o = 0; o < 32; ++o) x[o] = y[o] > 0.0f ? y[o] : 0.0f;
  float z;
  linear32<1>(hp + 2112, hp + 2144, x, &z);
  raw[row] = 1.0f / (1.0f + expf(-z));
}

// heu / heu.max() per sequence (mkp_transformer/net.py:44)
// SAVE: the maximum and the FIRST index attaining it go to svMx / svArg (the backward's `/ max` needs both)
template <bool SAVE>
__global__ void __launch_bounds__(256)
tf_max_div_kernel(int n, const float *__restrict__ raw, float *__restrict__ out, float *__restrict__ svMx,
                  int *__restrict__ svArg) {
  __shared__ float red[256];
  __shared__ int arg[256];
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
  if (SAVE) {
    int first = n;
    for (int i = threadIdx.x; i < n; i += 256)
      if (raw[(size_t)g * n + i] == mx && i < first) first = i;
    arg[threadIdx.x] = first;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s && arg[threadIdx.x + s] < arg[threadIdx.x]) arg[threadIdx.x] = arg[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) { svMx[g] = mx; svArg[g] = arg[0]; }
  }
}

}  // namespace daco

using namespace daco;

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
    hipLaunchKernelGGL(tf_attn_ffn_kernel<false>, grid, block, 0, s, n, lp, QKV, X, X, nullptr, nullptr, nullptr, nullptr, nullptr);
  }
  hipLaunchKernelGGL(tf_head_kernel<false>, grid, block, 0, s, n, params + t_layer_off(feats, TLAYERS), X, raw, nullptr, nullptr);
  hipLaunchKernelGGL(tf_max_div_kernel<false>, dim3((unsigned)G), dim3(256), 0, s, n, raw, out, nullptr, nullptr);
  return launch_status("transformer kernels");
}

// ---- the training forward: the same kernels with SAVE, every intermediate in the caller's `saved` buffer
extern "C" size_t daco_transformer_saved_floats(int G, int n) {
  if (G <= 0 || n <= 0) return 0;
  return (size_t)G * n * SV_TOKEN + 2 * (size_t)G;
}

int tf_check_train_args(const char *who, int G, int n, int feats, size_t param_floats, size_t saved_floats,
                        bool needs_workspace, size_t workspace_bytes) {
  if (feats < 1 || feats > TF_MAX_FEATS) { set_error("%s: 1 <= feats <= %d (feats=%d)", who, TF_MAX_FEATS, feats); return DACO_E_BADARG; }
  if (n > TF_MAX_TOKENS || G > 65535) { set_error("%s: n=%d tokens exceed %d (or G=%d > 65535)", who, n, TF_MAX_TOKENS, G); return DACO_E_TOOLARGE; }
  if (param_floats != daco_transformer_param_floats(feats)) { set_error("%s: %zu parameter floats, the layout has %zu", who, param_floats, daco_transformer_param_floats(feats)); return DACO_E_BADARG; }
  if (saved_floats < daco_transformer_saved_floats(G, n)) { set_error("%s: saved buffer %zu < %zu floats", who, saved_floats, daco_transformer_saved_floats(G, n)); return DACO_E_WORKSPACE; }
  const size_t need = needs_workspace ? daco_transformer_train_workspace_bytes(G, n) : 0;
  if (workspace_bytes < need) { set_error("%s: workspace %zu < %zu bytes", who, workspace_bytes, need); return DACO_E_WORKSPACE; }
  return DACO_OK;
}

extern "C" int daco_transformer_forward_train(void *stream, int G, int n, int feats, const float *src, const float *params,
                                              size_t param_floats, float *out, float *saved, size_t saved_floats,
                                              void *workspace, size_t workspace_bytes) {
  if (G <= 0 || n <= 0 || !src || !params || !out || !saved) { set_error("daco_transformer_forward_train: bad argument (G=%d n=%d)", G, n); return DACO_E_BADARG; }
  const int rc = tf_check_train_args("daco_transformer_forward_train", G, n, feats, param_floats, saved_floats, false, workspace_bytes);
  (void)workspace;                                       // X and QKV live in `saved`: the forward needs no scratch
  if (rc != DACO_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  const size_t N = (size_t)G * n;
  const SavedHead hd = saved_head(saved, N, G);
  dim3 grid((unsigned)((n + 127) / 128), (unsigned)G), block(128);
  for (int l = 0; l < TLAYERS; ++l) {
    const float *lp = params + t_layer_off(feats, l);
    const SavedLayer sv = saved_layer(saved, N, l);
    float *Xout = l + 1 < TLAYERS ? saved_layer(saved, N, l + 1).X : hd.X;
    hipLaunchKernelGGL(tf_qkv_kernel, grid, block, 0, s, n, feats, l == 0 ? 1 : 0, src, params, lp, sv.X, sv.QKV);
    hipLaunchKernelGGL(tf_attn_ffn_kernel<true>, grid, block, 0, s, n, lp, sv.QKV, sv.X, Xout, sv.O, sv.R1, sv.HPRE, sv.R2, sv.LSE);
  }
  hipLaunchKernelGGL(tf_head_kernel<true>, grid, block, 0, s, n, params + t_layer_off(feats, TLAYERS), hd.X, hd.RAW, hd.H1, hd.H2);
  hipLaunchKernelGGL(tf_max_div_kernel<true>, dim3((unsigned)G), dim3(256), 0, s, n, hd.RAW, out, hd.MX, hd.AMAX);
  return launch_status("transformer training kernels");
}
