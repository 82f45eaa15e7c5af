// daco_transformer_train.hip -- backward of the heuristic network of mkp_transformer/net.py:9-45 (daco_transformer.hip's
// forward) for G sequences of n tokens: grad_out [G][n] -> the gradient of the flat parameter block, in the block's layout.
//
// Reference behaviour replaced: torch autograd through TransformerModel.forward in mkp_transformer/train.py:15-31
// (loss.backward()).  float32, except two float64 accumulators per thread in tfb_attn_dq (the softmax row term, see
// there); no library GEMM, no atomics, no memset: every word of grad_params and of the
// workspace that is read is written by a kernel of the same call first.  The gradient of src is not formed (the network's
// input is data; the autograd function returns None for it).
//
// Input: the `saved` buffer of daco_transformer_forward_train (daco_transformer.h: 871 floats per token + 2 per sequence).
//
// Launches, N = G * n tokens, from the output down:
//   tfb_max_div    one workgroup per sequence: S = sum_j g_j out_j (256 strided partial sums of <= 16 terms, then a tree),
//                  d raw_i = (g_i - [i = first argmax] S) / max, times the sigmoid's raw (1 - raw).  n = 1: g - g * 1 = 0.
//   tfb_head       one thread per token: ParNet backwards, leaves d h2pre, d h1pre and d X_3.
//   per layer 2, 1, 0:
//     tfb_ffn      one thread per token: LayerNorm 2, linear2, ReLU, linear1, LayerNorm 1 (recomputed from r1), out_proj
//                  backwards; leaves every linear's dy row, LayerNorm's dy * xhat rows and dO.
//     tfb_attn_dq  one thread per query, K / V of the (sequence, head) streamed through LDS in tiles of 128 keys, as the
//                  forward does, twice: P_ij = exp(s_ij - lse_i), D_i = sum_j P_ij (dO_i . V_j) / sum_j P_ij, then
//                  dS_ij = P_ij (dO_i . V_j - D_i), dQ_i = 1/4 sum_j dS_ij K_j.
//     tfb_attn_dkv one thread per key, Q / dO / lse / D streamed in tiles of 128 queries: dK_j = 1/4 sum_i dS_ij Q_i,
//                  dV_j = sum_i P_ij dO_i.  The n x n probabilities are never written; a tile is summed from zero and
//                  merged into the totals, so no chain is longer than 128 terms plus n / 128 merges.
//     tfb_wgrad    the weight and bias gradients of the layer's ten tensors: dW[o][i] = sum_tok dy[tok][o] x[tok][i] on
//                  v_mfma_f32_16x16x4_f32 with the tokens as the K dimension.  One workgroup per (tile of 128 tokens, tensor),
//                  one wave per 16 x 16 block of dW, operands straight from global memory in the instruction's lane map
//                  (A[l&15][k=l>>4] = dy[tok0+k][o], B[k=l>>4][l&15] = x[tok0+k][i]): four 64-byte row segments per load.
//                  The MFMA is a k-ordered fma chain from C, so a tile's partial is one chain of 128.  Partials go to
//                  workspace [tile][parameter], every word written exactly once -- no atomics, nothing to clear.
//     tfb_dx       one thread per token: d X_l = d r1 + in_proj^T d qkv (layer 0: times sqrt(32), the input projection's dy).
//   tfb_wgrad      once more for the head's three linears (right after tfb_head) and for the input projection.
//   tfb_merge      one thread per parameter sums the tile partials in tile order, 128 tiles to a chain, chains merged in
//                  order: two-stage, fixed order, so two calls on the same inputs agree bit for bit.
// 2 + 1 + 3 * 5 + 1 + 1 = 20 launches, no host synchronisation, every one capturable.
#include "daco_transformer.h"

namespace daco {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int WS_TOKEN = 32 * 9 + 96 + 2 + 1;        // workspace floats per token, before the tile partials

// LayerNorm backwards in place.  r: the LayerNorm's input (becomes xhat), g: d output (becomes d input); e = g * xhat
// (the row whose sum over tokens is d weight) goes to global memory.
__device__ inline void layer_norm32_backward(float (&r)[32], float (&g)[32], const float *__restrict__ w, float *__restrict__ e) {
  float mean = 0.0f;
#pragma unroll
  for (int i = 0; i < 32; ++i) mean = mean + r[i];
  mean = mean * (1.0f / 32.0f);
  float var = 0.0f;
#pragma unroll
  for (int i = 0; i < 32; ++i) { const float d = r[i] - mean; var = __builtin_fmaf(d, d, var); }
  const float rstd = 1.0f / sqrtf(var * (1.0f / 32.0f) + 1e-5f);
  float m1 = 0.0f, m2 = 0.0f;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    r[i] = (r[i] - mean) * rstd;
    e[i] = g[i] * r[i];
    g[i] = g[i] * w[i];
    m1 = m1 + g[i];
    m2 = __builtin_fmaf(g[i], r[i], m2);
  }
  m1 = m1 * (1.0f / 32.0f);
  m2 = m2 * (1.0f / 32.0f);
#pragma unroll
  for (int i = 0; i < 32; ++i) g[i] = rstd * (g[i] - m1 - r[i] * m2);
}

// x[i] += sum_o W[o][i] dy[o]  (W [NO][32] row-major: the transposed product, chains of NO in o order)
template <int NO>
__device__ inline void linear32_transposed(const float *__restrict__ W, const float *dy, float (&x)[32]) {
#pragma unroll 4
  for (int o = 0; o < NO; ++o) {
    const float d = dy[o];
#pragma unroll
    for (int i = 0; i < 32; ++i) x[i] = __builtin_fmaf(W[o * 32 + i], d, x[i]);
  }
}

__device__ inline void load32(float (&x)[32], const float *__restrict__ p) {
#pragma unroll
  for (int i = 0; i < 32; i += 4) {
    const float4 v = *reinterpret_cast<const float4 *>(p + i);
    x[i] = v.x; x[i + 1] = v.y; x[i + 2] = v.z; x[i + 3] = v.w;
  }
}
__device__ inline void store32(float *__restrict__ p, const float (&x)[32]) {
#pragma unroll
  for (int i = 0; i < 32; i += 4) *reinterpret_cast<float4 *>(p + i) = make_float4(x[i], x[i + 1], x[i + 2], x[i + 3]);
}

// One thread's two 16-float rows of a 128-row tile into LDS: all eight 16-byte loads are issued into registers before the
// first LDS store, so the tile costs one memory round trip, not eight (tools/scan_serialized_loads.py).  The row index is
// clamped by the caller: rows past the end of the sequence hold a copy of the last row and are never read.
__device__ inline void stage_rows(float *__restrict__ A, float *__restrict__ B, const float *__restrict__ a, const float *__restrict__ b) {
  float4 ra[THD / 4], rb[THD / 4];
#pragma unroll
  for (int d = 0; d < THD / 4; ++d) { ra[d] = reinterpret_cast<const float4 *>(a)[d]; rb[d] = reinterpret_cast<const float4 *>(b)[d]; }
#pragma unroll
  for (int d = 0; d < THD / 4; ++d) { reinterpret_cast<float4 *>(A)[d] = ra[d]; reinterpret_cast<float4 *>(B)[d] = rb[d]; }
}

// `/ max` and the sigmoid backwards: DZ[tok] = d (the last linear's output)
__global__ void __launch_bounds__(256)
tfb_max_div_kernel(int n, const float *__restrict__ raw, const float *__restrict__ svMx, const int *__restrict__ svArg,
                   const float *__restrict__ gout, float *__restrict__ DZ) {
  __shared__ float red[256];
  const int g = blockIdx.x;
  const size_t base = (size_t)g * n;
  const float mx = svMx[g];
  const int a = svArg[g];
  float s = 0.0f;
  for (int i = threadIdx.x; i < n; i += 256) s = s + gout[base + i] * (raw[base + i] / mx);
  red[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + k];
    __syncthreads();
  }
  const float S = red[0];
  for (int i = threadIdx.x; i < n; i += 256) {
    const float r = raw[base + i];
    const float draw = (gout[base + i] - (i == a ? S : 0.0f)) / mx;
    DZ[base + i] = draw * (r * (1.0f - r));
  }
}

// ParNet backwards for one token
__global__ void __launch_bounds__(128)
tfb_head_kernel(size_t N, const float *__restrict__ hp, const float *__restrict__ H1, const float *__restrict__ H2,
                const float *__restrict__ DZ, float *__restrict__ DH2, float *__restrict__ DH1, float *__restrict__ dX) {
  const size_t tok = (size_t)blockIdx.x * 128 + threadIdx.x;
  if (tok >= N) return;
  const float dz = DZ[tok];
  float h[32], d2[32], d1[32];
  load32(h, H2 + tok * 32);
#pragma unroll
  for (int i = 0; i < 32; ++i) d2[i] = h[i] > 0.0f ? hp[2112 + i] * dz : 0.0f;
  store32(DH2 + tok * 32, d2);
#pragma unroll
  for (int i = 0; i < 32; ++i) d1[i] = 0.0f;
  linear32_transposed<32>(hp + 1056, d2, d1);
  load32(h, H1 + tok * 32);
#pragma unroll
  for (int i = 0; i < 32; ++i) d1[i] = h[i] > 0.0f ? d1[i] : 0.0f;
  store32(DH1 + tok * 32, d1);
#pragma unroll
  for (int i = 0; i < 32; ++i) d2[i] = 0.0f;
  linear32_transposed<32>(hp, d1, d2);
  store32(dX + tok * 32, d2);
}

// one encoder layer's per-token part backwards, from d (layer output) in dX down to dO
__global__ void __launch_bounds__(128)
tfb_ffn_kernel(size_t N, const float *__restrict__ lp, const float *__restrict__ svR1,
               const float *__restrict__ svH, const float *__restrict__ svR2, const float *__restrict__ dX,
               float *__restrict__ E2, float *__restrict__ DR2, float *__restrict__ DHPRE, float *__restrict__ X1,
               float *__restrict__ DX1, float *__restrict__ E1, float *__restrict__ DR1, float *__restrict__ DO) {
  const size_t tok = (size_t)blockIdx.x * 128 + threadIdx.x;
  if (tok >= N) return;
  float r[32], dy[32], t[32];
  load32(r, svR2 + tok * 32);
  load32(dy, dX + tok * 32);
  layer_norm32_backward(r, dy, lp + OFF_N2_W, t);                   // dy = d r2
  store32(E2 + tok * 32, t);
  store32(DR2 + tok * 32, dy);
  load32(r, svR1 + tok * 32);                                       // x1 = LayerNorm1(r1), the forward's own code
  layer_norm32(r, lp + OFF_N1_W, lp + OFF_N1_B);
  store32(X1 + tok * 32, r);
#pragma unroll
  for (int i = 0; i < 32; ++i) t[i] = 0.0f;
  linear32_transposed<32>(lp + OFF_L2_W, dy, t);                    // d relu output
  load32(r, svH + tok * 32);
#pragma unroll
  for (int i = 0; i < 32; ++i) t[i] = r[i] > 0.0f ? t[i] : 0.0f;
  store32(DHPRE + tok * 32, t);
  linear32_transposed<32>(lp + OFF_L1_W, t, dy);                    // dy = d x1 = d r2 + linear1^T d hpre
  store32(DX1 + tok * 32, dy);
  load32(r, svR1 + tok * 32);
  layer_norm32_backward(r, dy, lp + OFF_N1_W, t);                   // dy = d r1
  store32(E1 + tok * 32, t);
  store32(DR1 + tok * 32, dy);
#pragma unroll
  for (int i = 0; i < 32; ++i) t[i] = 0.0f;
  linear32_transposed<32>(lp + OFF_OUT_W, dy, t);                   // t = dO
  store32(DO + tok * 32, t);
}

// D and dQ: one thread per query, two sweeps over the keys.  The first forms D_i = sum_j P_ij (dO_i . V_j) / sum_j P_ij from the
// same recomputed P_ij = exp(s_ij - lse_i) that the second sweep and tfb_attn_dkv use, both sums in float64 (two scalars per
// thread; everything else stays float32), so that a row of dS sums to zero to the rounding of D_i itself.  The textbook
// D_i = dO_i . O_i does not: lse_i near log(4096) = 8.3 is rounded to 5e-7, P's row sum is off by as much, and
// sum_j dS_ij = D_i (1 - sum_j P_ij) is an O(1) quantity times 1e-6 per query, where the terms of dK are O(1 / n).  The k rows
// of in_proj_bias (true gradient 0 = the sum of those row sums) show it: at n = 4096 with the pretrained block, against
// float64, 2.68 bounds of tests/mkp_grad_cases.py with dO . O, 1.30 with the two sums in float32 tiles, 0.064 with float64.
__global__ void __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(1, 3)))
tfb_attn_dq_kernel(int n, const float *__restrict__ QKV, const float *__restrict__ LSE, const float *__restrict__ DO,
                   float *__restrict__ D, float *__restrict__ dQKV) {
  __shared__ __attribute__((aligned(16))) float Ks[TTILE * THD];
  __shared__ __attribute__((aligned(16))) float Vs[TTILE * THD];
  const int g = blockIdx.y, tok = blockIdx.x * 128 + threadIdx.x;
  const bool live = tok < n;
  const size_t row = (size_t)g * n + (live ? tok : n - 1);
  const float *base = QKV + (size_t)g * n * 96;
  {
    const int h = blockIdx.z;                          // a head per workgroup: twice the workgroups, half the serial loop
    float q[THD], go[THD], tot[THD];
#pragma unroll
    for (int d = 0; d < THD; ++d) { q[d] = QKV[row * 96 + h * THD + d]; go[d] = DO[row * 32 + h * THD + d]; tot[d] = 0.0f; }
    const float lse = LSE[row * 2 + h];
    double psum = 0.0, dsum = 0.0;                      // two float64 scalars per thread: see above
    for (int t0 = 0; t0 < n; t0 += TTILE) {
      __syncthreads();
      const int key = t0 + (int)threadIdx.x < n ? t0 + (int)threadIdx.x : n - 1;
      stage_rows(Ks + threadIdx.x * THD, Vs + threadIdx.x * THD, base + (size_t)key * 96 + 32 + h * THD,
                 base + (size_t)key * 96 + 64 + h * THD);
      __syncthreads();
      const int cnt = n - t0 < TTILE ? n - t0 : TTILE;
#pragma unroll 2
      for (int j = 0; j < cnt; ++j) {
        float s = 0.0f, dp = 0.0f;
#pragma unroll
        for (int d = 0; d < THD; ++d) s = __builtin_fmaf(q[d], Ks[j * THD + d], s);
#pragma unroll
        for (int d = 0; d < THD; ++d) dp = __builtin_fmaf(go[d], Vs[j * THD + d], dp);
        const float p = expf(s * 0.25f - lse);
        psum = psum + (double)p;
        dsum = __builtin_fma((double)p, (double)dp, dsum);
      }
    }
    const float Di = (float)(dsum / psum);
    if (live) D[row * 2 + h] = Di;
    for (int t0 = 0; t0 < n; t0 += TTILE) {
      __syncthreads();
      const int key = t0 + (int)threadIdx.x < n ? t0 + (int)threadIdx.x : n - 1;
      stage_rows(Ks + threadIdx.x * THD, Vs + threadIdx.x * THD, base + (size_t)key * 96 + 32 + h * THD,
                 base + (size_t)key * 96 + 64 + h * THD);
      __syncthreads();
      const int cnt = n - t0 < TTILE ? n - t0 : TTILE;
      float acc[THD];
#pragma unroll
      for (int d = 0; d < THD; ++d) acc[d] = 0.0f;
#pragma unroll 2
      for (int j = 0; j < cnt; ++j) {
        float s = 0.0f, dp = 0.0f;
#pragma unroll
        for (int d = 0; d < THD; ++d) s = __builtin_fmaf(q[d], Ks[j * THD + d], s);
#pragma unroll
        for (int d = 0; d < THD; ++d) dp = __builtin_fmaf(go[d], Vs[j * THD + d], dp);
        const float ds = expf(s * 0.25f - lse) * (dp - Di);
#pragma unroll
        for (int d = 0; d < THD; ++d) acc[d] = __builtin_fmaf(ds, Ks[j * THD + d], acc[d]);
      }
#pragma unroll
      for (int d = 0; d < THD; ++d) tot[d] = tot[d] + acc[d];
    }
    if (live) {
#pragma unroll
      for (int d = 0; d < THD; ++d) dQKV[row * 96 + h * THD + d] = tot[d] * 0.25f;
    }
  }
}

// dK and dV: one thread per key
__global__ void __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(1, 2)))
tfb_attn_dkv_kernel(int n, const float *__restrict__ QKV, const float *__restrict__ LSE, const float *__restrict__ DO,
                    const float *__restrict__ D, float *__restrict__ dQKV) {
  __shared__ __attribute__((aligned(16))) float Qs[TTILE * THD];
  __shared__ __attribute__((aligned(16))) float Gs[TTILE * THD];
  __shared__ float Ls[TTILE], Ds[TTILE];
  const int g = blockIdx.y, tok = blockIdx.x * 128 + threadIdx.x;
  const bool live = tok < n;
  const size_t row = (size_t)g * n + (live ? tok : n - 1);
  const size_t seq = (size_t)g * n;
  {
    const int h = blockIdx.z;
    float k[THD], v[THD], tk[THD], tv[THD];
#pragma unroll
    for (int d = 0; d < THD; ++d) {
      k[d] = QKV[row * 96 + 32 + h * THD + d]; v[d] = QKV[row * 96 + 64 + h * THD + d]; tk[d] = 0.0f; tv[d] = 0.0f;
    }
    for (int t0 = 0; t0 < n; t0 += TTILE) {
      __syncthreads();
      const int qi = t0 + (int)threadIdx.x < n ? t0 + (int)threadIdx.x : n - 1;
      const float lq = LSE[(seq + qi) * 2 + h], dq = D[(seq + qi) * 2 + h];
      stage_rows(Qs + threadIdx.x * THD, Gs + threadIdx.x * THD, QKV + (seq + qi) * 96 + h * THD, DO + (seq + qi) * 32 + h * THD);
      Ls[threadIdx.x] = lq;
      Ds[threadIdx.x] = dq;
      __syncthreads();
      const int cnt = n - t0 < TTILE ? n - t0 : TTILE;
      float ak[THD], av[THD];
#pragma unroll
      for (int d = 0; d < THD; ++d) { ak[d] = 0.0f; av[d] = 0.0f; }
#pragma unroll 2
      for (int i = 0; i < cnt; ++i) {
        float s = 0.0f, dp = 0.0f;
#pragma unroll
        for (int d = 0; d < THD; ++d) s = __builtin_fmaf(Qs[i * THD + d], k[d], s);
#pragma unroll
        for (int d = 0; d < THD; ++d) dp = __builtin_fmaf(Gs[i * THD + d], v[d], dp);
        const float p = expf(s * 0.25f - Ls[i]);
        const float ds = p * (dp - Ds[i]);
#pragma unroll
        for (int d = 0; d < THD; ++d) {
          av[d] = __builtin_fmaf(p, Gs[i * THD + d], av[d]);
          ak[d] = __builtin_fmaf(ds, Qs[i * THD + d], ak[d]);
        }
      }
#pragma unroll
      for (int d = 0; d < THD; ++d) { tk[d] = tk[d] + ak[d]; tv[d] = tv[d] + av[d]; }
    }
    if (live) {
#pragma unroll
      for (int d = 0; d < THD; ++d) {
        dQKV[row * 96 + 32 + h * THD + d] = tk[d] * 0.25f;
        dQKV[row * 96 + 64 + h * THD + d] = tv[d];
      }
    }
  }
}

// d X_l = d r1 + in_proj^T d qkv; layer 0: times sqrt(32), which makes it the dy of the input projection
__global__ void __launch_bounds__(128)
tfb_dx_kernel(size_t N, int first, const float *__restrict__ lp, const float *__restrict__ DR1,
              const float *__restrict__ dQKV, float *__restrict__ dX) {
  const size_t tok = (size_t)blockIdx.x * 128 + threadIdx.x;
  if (tok >= N) return;
  float x[32], d[32];
  load32(x, DR1 + tok * 32);
  for (int blk = 0; blk < 3; ++blk) {
    load32(d, dQKV + tok * 96 + blk * 32);
    linear32_transposed<32>(lp + OFF_IN_W + blk * 1024, d, x);
  }
  if (first) {
    const float scale = sqrtf(32.0f);
#pragma unroll
    for (int i = 0; i < 32; ++i) x[i] = x[i] * scale;
  }
  store32(dX + tok * 32, x);
}

// One tensor pair of tfb_wgrad: dW [nrows][ncols] at offW (offW < 0: none) and db [nrows] at offB of the parameter layout;
// dy rows of dy_stride floats, x rows of x_stride floats (relu_x: x = max(x, 0), the ReLU output of a saved ReLU input).
struct TfJob { const float *dy, *x; int dy_stride, x_stride, nrows, ncols, relu_x, offW, offB; };
constexpr int TF_MAX_JOBS = 10;
struct TfJobs { TfJob j[TF_MAX_JOBS]; };

__global__ void __launch_bounds__(256)
tfb_wgrad_kernel(size_t N, TfJobs jobs, float *__restrict__ partials, size_t P) {
  const TfJob jb = jobs.j[blockIdx.y];
  const size_t tok0 = (size_t)blockIdx.x * TTILE;
  const int cnt = N - tok0 < (size_t)TTILE ? (int)(N - tok0) : TTILE;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ob = (wave >> 1) * 16, ib = (wave & 1) * 16;
  float *dst = partials + (size_t)blockIdx.x * P;
  if (jb.offW >= 0 && ob < jb.nrows && ib < jb.ncols) {                       // wave-uniform
    const int o = ob + (lane & 15), i = ib + (lane & 15), kk = lane >> 4;
    const bool ov = o < jb.nrows, iv = i < jb.ncols;
    f32x4 c = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int t = 0; t < cnt; t += 4) {
      const bool tv = t + kk < cnt;
      const size_t tok = tok0 + t + kk;
      float a = (tv && ov) ? jb.dy[tok * jb.dy_stride + o] : 0.0f;
      float b = (tv && iv) ? jb.x[tok * jb.x_stride + i] : 0.0f;
      if (jb.relu_x) b = b > 0.0f ? b : 0.0f;
      c = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int orow = ob + 4 * (lane >> 4) + r;
      if (orow < jb.nrows && iv) dst[jb.offW + orow * jb.ncols + i] = c[r];
    }
  }
  // db[o] = sum_tok dy[tok][o]: 16 columns x four runs of 32 tokens per wave, the four runs' sums added in token order
  if (ib == 0 && ob < jb.nrows) {                                             // wave-uniform
    const int o = ob + (lane & 15), run = lane >> 4;
    const bool ov = o < jb.nrows;
    float acc = 0.0f;
    for (int t = run * 32; t < run * 32 + 32; ++t) {
      const float v = (ov && t < cnt) ? jb.dy[(tok0 + t) * jb.dy_stride + o] : 0.0f;
      acc = acc + v;
    }
    const float r1 = __shfl(acc, lane + 16), r2 = __shfl(acc, lane + 32), r3 = __shfl(acc, lane + 48);
    if (lane < 16 && ov) dst[jb.offB + o] = ((acc + r1) + r2) + r3;
  }
}

// grad[p] = the tile partials in tile order: chains of 128 tiles, the chains' sums added in order
__global__ void __launch_bounds__(256)
tfb_merge_kernel(size_t ntiles, size_t P, const float *__restrict__ partials, float *__restrict__ grad) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  float total = 0.0f;
  for (size_t c0 = 0; c0 < ntiles; c0 += 128) {
    const size_t c1 = c0 + 128 < ntiles ? c0 + 128 : ntiles;
    float s = 0.0f;
    for (size_t t = c0; t < c1; ++t) s = s + partials[t * P + p];
    total = total + s;
  }
  grad[p] = total;
}

static TfJob tf_job(const float *dy, int dy_stride, int nrows, const float *x, int x_stride, int ncols, int relu_x, size_t offW,
                    size_t offB) {
  return TfJob{dy, x, dy_stride, x_stride, nrows, ncols, relu_x, x ? (int)offW : -1, (int)offB};
}

}  // namespace daco

using namespace daco;

extern "C" size_t daco_transformer_train_workspace_bytes(int G, int n) {
  if (G <= 0 || n <= 0) return 0;
  const size_t N = (size_t)G * n, ntiles = (N + TTILE - 1) / TTILE;
  return (N * WS_TOKEN + ntiles * daco_transformer_param_floats(TF_MAX_FEATS)) * sizeof(float);
}

extern "C" int daco_transformer_backward(void *stream, int G, int n, int feats, const float *src, const float *params,
                                         size_t param_floats, const float *saved, size_t saved_floats, const float *grad_out,
                                         float *grad_params, void *workspace, size_t workspace_bytes) {
  if (G <= 0 || n <= 0 || !src || !params || !saved || !grad_out || !grad_params || !workspace) { set_error("daco_transformer_backward: bad argument (G=%d n=%d)", G, n); return DACO_E_BADARG; }
  const int rc = tf_check_train_args("daco_transformer_backward", G, n, feats, param_floats, saved_floats, true, workspace_bytes);
  if (rc != DACO_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  const size_t N = (size_t)G * n, ntiles = (N + TTILE - 1) / TTILE, P = param_floats;
  float *sv = const_cast<float *>(saved);
  float *w = (float *)workspace;
  float *dX = w, *E2 = w + 32 * N, *DR2 = w + 64 * N, *DHPRE = w + 96 * N, *X1 = w + 128 * N, *DX1 = w + 160 * N,
        *E1 = w + 192 * N, *DR1 = w + 224 * N, *DO = w + 256 * N, *dQKV = w + 288 * N, *D = w + 384 * N, *DZ = w + 386 * N,
        *partials = w + (size_t)WS_TOKEN * N;
  const SavedHead hd = saved_head(sv, N, G);
  const dim3 tokens((unsigned)ntiles), seqs((unsigned)((n + 127) / 128), (unsigned)G, TH), b128(128), b256(256);
  const size_t hoff = t_layer_off(feats, TLAYERS);
  TfJobs jobs;

  hipLaunchKernelGGL(tfb_max_div_kernel, dim3((unsigned)G), b256, 0, s, n, hd.RAW, hd.MX, hd.AMAX, grad_out, DZ);
  hipLaunchKernelGGL(tfb_head_kernel, tokens, b128, 0, s, N, params + hoff, hd.H1, hd.H2, DZ, DR2, DHPRE, dX);   // d h2pre -> DR2, d h1pre -> DHPRE
  for (int k = 0; k < TF_MAX_JOBS; ++k) jobs.j[k] = TfJob{};
  jobs.j[0] = tf_job(DZ, 1, 1, hd.H2, 32, 32, 1, hoff + 2112, hoff + 2144);
  jobs.j[1] = tf_job(DR2, 32, 32, hd.H1, 32, 32, 1, hoff + 1056, hoff + 2080);
  jobs.j[2] = tf_job(DHPRE, 32, 32, hd.X, 32, 32, 0, hoff, hoff + 1024);
  hipLaunchKernelGGL(tfb_wgrad_kernel, dim3((unsigned)ntiles, 3), b256, 0, s, N, jobs, partials, P);
  for (int l = TLAYERS - 1; l >= 0; --l) {
    const float *lp = params + t_layer_off(feats, l);
    const size_t lo = t_layer_off(feats, l);
    const SavedLayer L = saved_layer(sv, N, l);
    hipLaunchKernelGGL(tfb_ffn_kernel, tokens, b128, 0, s, N, lp, L.R1, L.HPRE, L.R2, dX, E2, DR2, DHPRE, X1, DX1, E1, DR1, DO);
    hipLaunchKernelGGL(tfb_attn_dq_kernel, seqs, b128, 0, s, n, L.QKV, L.LSE, DO, D, dQKV);
    hipLaunchKernelGGL(tfb_attn_dkv_kernel, seqs, b128, 0, s, n, L.QKV, L.LSE, DO, D, dQKV);
    jobs.j[0] = tf_job(DR2, 32, 32, L.HPRE, 32, 32, 1, lo + OFF_L2_W, lo + OFF_L2_B);
    jobs.j[1] = tf_job(DHPRE, 32, 32, X1, 32, 32, 0, lo + OFF_L1_W, lo + OFF_L1_B);
    jobs.j[2] = tf_job(DR1, 32, 32, L.O, 32, 32, 0, lo + OFF_OUT_W, lo + OFF_OUT_B);
    for (int blk = 0; blk < 3; ++blk)
      jobs.j[3 + blk] = tf_job(dQKV + blk * 32, 96, 32, L.X, 32, 32, 0, lo + OFF_IN_W + blk * 1024, lo + OFF_IN_B + blk * 32);
    jobs.j[6] = tf_job(E2, 32, 32, nullptr, 0, 0, 0, 0, lo + OFF_N2_W);
    jobs.j[7] = tf_job(dX, 32, 32, nullptr, 0, 0, 0, 0, lo + OFF_N2_B);
    jobs.j[8] = tf_job(E1, 32, 32, nullptr, 0, 0, 0, 0, lo + OFF_N1_W);
    jobs.j[9] = tf_job(DX1, 32, 32, nullptr, 0, 0, 0, 0, lo + OFF_N1_B);
    hipLaunchKernelGGL(tfb_wgrad_kernel, dim3((unsigned)ntiles, 10), b256, 0, s, N, jobs, partials, P);
    hipLaunchKernelGGL(tfb_dx_kernel, tokens, b128, 0, s, N, l == 0 ? 1 : 0, lp, DR1, dQKV, dX);
  }
  jobs.j[0] = tf_job(dX, 32, 32, src, feats, feats, 0, 0, (size_t)32 * feats);
  hipLaunchKernelGGL(tfb_wgrad_kernel, dim3((unsigned)ntiles, 1), b256, 0, s, N, jobs, partials, P);
  hipLaunchKernelGGL(tfb_merge_kernel, dim3((unsigned)((P + 255) / 256)), b256, 0, s, ntiles, P, partials, grad_params);
  return launch_status("transformer backward kernels");
}
