// daco_edge_grad.hip -- tour log-probabilities and their gradient on the k-sparse graph's edge list.
//
// Reference behaviour replaced: autograd through ACO.gen_path(require_prob=True) on the heuristic that Net.reshape scatters
// (tsp/net.py:94-102: k values per row into zeros, `+ EPS` by the caller; tsp/train.ipynb:32-49, tsp_nls/train.py:15-44) with
// the pheromone of a fresh colony (ones).  The dense kernels (daco_tsp_sample with logp, daco_sample_backward) walk all n
// candidates of a row and leave a [B][n][n] gradient of which reshape's backward gathers n k entries; here a step reads and
// differentiates the k edges that leave the current node and nothing else:
//   eta_e = heu_e + eps on the graph, eps off it;   p_e = eta_e^beta over the row's edges whose destination is unvisited;
//   S_t   = sum p_e + eps^beta * ((n - t) - live neighbours)        (the off-graph candidates: an integer count, no row walk)
//   log p_t = log clamp(p_j / S_t, EPS_F32, 1 - EPS_F32),  p_j = eps^beta when the move itself is off the graph;
//   d log p_t / d heu_e = beta * ([e chosen] / eta_e - p_e / (eta_e * S_t)) on live edges, 0 when clamped.
// The [k = j] term of an off-graph move has no edge and is dropped, as reshape's backward drops it on the dense path.
//
// Layout of the work.  A draw's open set is "not yet visited", which here must be answered per DESTINATION id; instead of a
// visited bitmap that a wave updates step by step, a block holds its ant's tour as the table pos[node] = step at which the
// node is visited (2 n bytes of LDS, written once): destination d is open at step t iff pos[d] >= t.  That makes every step
// independent of the ones before it, so the waves that share an ant (four per block, `segs` blocks per ant -- the split of
// daco_sample_backward) replay nothing: each takes its own steps.  A lane owns edge `lane` (and `lane + 64` for k > 64) of
// the row; the row's k floats are contiguous, so a step's atomic adds land on one contiguous segment of 4 k <= 512 bytes,
// the shape global float atomics run at full rate for; an LDS-resident [n k] accumulator would fit at 500 x 50 but not at
// 1000 x 100, and would tie a block to one instance's ants.  Summation order across ants is not fixed (hardware f32 atomics):
// reproducible to rounding, as daco_sample_backward.
#include "daco_host.h"

namespace daco {

struct EdgeParams {
  int B, n, k, A, segs;
  const float *heu;              // [B][n*k]
  const int64_t *dst64;          // [B] rows of n*k graph-local ids, dst64_bs elements apart, or null
  long dst64_bs;
  const int32_t *dst32;          // [B][n*k] ids of the block-diagonal batch graph (b * n + local), or null
  float eps, beta;
  const int64_t *paths;          // [B][n][A]
  float *logp, *rowsum;          // forward: out [B][n-1][A]
  const float *rowsum_in, *grad_logp;   // backward: in [B][n-1][A]
  float *grad_heu;               // backward: [B][n*k], accumulated into
};

template <bool BACKWARD>
__global__ void __launch_bounds__(256)
edge_replay_kernel(const EdgeParams p) {
  __shared__ uint16_t pos[DACO_MAX_NODES];       // pos[node] = step at which the ant visits it (0xFFFF: never)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int seg = blockIdx.x % p.segs, ant = blockIdx.x / p.segs;
  const int b = ant / p.A, a = ant - b * p.A;
  const int n = p.n, k = p.k, A = p.A;
  const size_t E = (size_t)n * k;
  const int64_t *path = p.paths + (size_t)b * n * A + a;
  for (int i = threadIdx.x; i < n; i += 256) pos[i] = 0xFFFFu;
  __syncthreads();
  for (int t = threadIdx.x; t < n; t += 256) {
    const int64_t v = path[(size_t)t * A];
    if (v >= 0 && v < n) pos[v] = (uint16_t)t;
  }
  __syncthreads();

  const float *heu = p.heu + (size_t)b * E;
  const int64_t *d64 = p.dst64 ? p.dst64 + (size_t)b * p.dst64_bs : nullptr;
  const int32_t *d32 = p.dst32 ? p.dst32 + (size_t)b * E : nullptr;
  const int bias = p.dst32 ? b * n : 0;
  const size_t out0 = (size_t)b * (n - 1) * A + a;
  const float epsb = pw(p.eps, p.beta);
  const int per = (n - 1 + p.segs - 1) / p.segs;
  const int t_lo = 1 + seg * per, t_hi = min(n, t_lo + per);          // this block's steps [t_lo, t_hi), dealt to its four waves
  const bool two = k > 64;

  for (int t = t_lo + wave; t < t_hi; t += 4) {
    float g = 0.0f, Ssaved = 1.0f;
    if (BACKWARD) {
      g = p.grad_logp[out0 + (size_t)(t - 1) * A];
      if (g == 0.0f) continue;
      Ssaved = p.rowsum_in[out0 + (size_t)(t - 1) * A];
    }
    int64_t iv = path[(size_t)(t - 1) * A];
    const int j = (int)path[(size_t)t * A];
    const int i = (int)(iv < 0 ? 0 : (iv >= n ? n - 1 : iv));         // (a tour outside [0, n) is the caller's error: stay in bounds)
    const size_t row = (size_t)i * k;
    float pe[2] = {0.0f, 0.0f}, ee[2] = {1.0f, 1.0f};
    bool live[2] = {false, false}, hit[2] = {false, false};
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int e = lane + 64 * u;
      if ((u == 0 || two) && e < k) {
        const int d = (d32 ? d32[row + e] : (int)d64[row + e]) - bias;
        const float eta = heu[row + e] + p.eps;
        live[u] = d >= 0 && d < n && (int)pos[d] >= t;
        ee[u] = eta;
        pe[u] = live[u] ? pw(eta, p.beta) : 0.0f;
        hit[u] = live[u] && d == j;
      }
    }
    const int nlive = __popcll(__ballot(live[0])) + __popcll(__ballot(live[1]));
    // the chosen edge's p (destinations of a row are distinct: at most one lane adds a non-zero, the sum is exact)
    const bool on_graph = __ballot(hit[0] || hit[1]) != 0ull;
    const float pj_edge = wave_sum((hit[0] ? pe[0] : 0.0f) + (hit[1] ? pe[1] : 0.0f));
    const float pj = on_graph ? pj_edge : epsb;
    if (!BACKWARD) {
      const float S = wave_sum(pe[0] + pe[1]) + (float)(n - t - nlive) * epsb;
      if (lane == 0) {
        p.rowsum[out0 + (size_t)(t - 1) * A] = S;
        p.logp[out0 + (size_t)(t - 1) * A] = clamp_log(pj / S);
      }
    } else {
      const float pr = pj / Ssaved;
      if (!(pr > DACO_EPS_F32 && pr < 1.0f - DACO_EPS_F32)) continue;      // clamped: no gradient
      const float c = g / Ssaved;
      float *grow = p.grad_heu + (size_t)b * E + row;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (!live[u]) continue;
        float val = -c * dprob_deta(pe[u], 1.0f, ee[u], 1.0f, p.beta);
        if (hit[u]) val += g * p.beta / ee[u];
        unsafeAtomicAdd(grow + lane + 64 * u, val);
      }
    }
  }
}

static long edge_args(const char *what, int B, int n, int k, int A, const float *heu, const int64_t *edge_dst, long edge_dst_bstride,
                      const int32_t *edge_dst32, float eps, const int64_t *paths, const void *o1, const void *o2, const void *o3, int *segs) {
  static const char *dense = "the dense path (daco_tsp_sample with logp / daco_sample_backward on daco_heu_matrix's matrix) has no such limit";
  if (B <= 0 || n < 2 || A <= 0 || k < 1 || !heu || !paths || !o1 || !o2 || !o3 || (edge_dst == nullptr) == (edge_dst32 == nullptr) ||
      (edge_dst && edge_dst_bstride < 0) || !(eps >= 0.0f)) {
    set_error("%s: bad argument (B=%d n=%d k=%d A=%d; exactly one of edge_dst / edge_dst32; eps >= 0); %s", what, B, n, k, A, dense);
    return DACO_E_BADARG;
  }
  if (n > DACO_MAX_NODES) { set_error("%s: n=%d exceeds DACO_MAX_NODES; %s", what, n, dense); return DACO_E_TOOLARGE; }
  if (k > 128) { set_error("%s: k=%d exceeds the 128 edges per row a wavefront holds; %s", what, k, dense); return DACO_E_TOOLARGE; }
  if (k >= n) { set_error("%s: k=%d must stay below n=%d (a node has at most n - 1 neighbours); %s", what, k, n, dense); return DACO_E_BADARG; }
  // blocks per ant so that a small batch still fills the device (the rule of daco_sample_backward)
  int s = 1;
  while (s < 8 && (long)B * A * s * 2 <= 2048) s *= 2;
  if ((long)B * A * s > 0x7fffffffL || (edge_dst32 && (long)B * n > 0x7fffffffL)) {
    set_error("%s: B * A = %ld blocks (or B * n node ids) do not fit 32 bits; %s", what, (long)B * A, dense);
    return DACO_E_TOOLARGE;
  }
  *segs = s;
  return DACO_OK;
}

}  // namespace daco

using namespace daco;

extern "C" long daco_tsp_edge_logp(void *stream, int B, int n, int k, int A, const float *heu, const int64_t *edge_dst,
                                   long edge_dst_bstride, const int32_t *edge_dst32, float eps, float beta, const int64_t *paths,
                                   float *logp, float *rowsum) {
  EdgeParams ep = {};
  const long rc = edge_args("daco_tsp_edge_logp", B, n, k, A, heu, edge_dst, edge_dst_bstride, edge_dst32, eps, paths, logp, rowsum, rowsum,
                            &ep.segs);
  if (rc != DACO_OK) return rc;
  ep.B = B; ep.n = n; ep.k = k; ep.A = A; ep.heu = heu; ep.dst64 = edge_dst; ep.dst64_bs = edge_dst_bstride; ep.dst32 = edge_dst32;
  ep.eps = eps; ep.beta = beta; ep.paths = paths; ep.logp = logp; ep.rowsum = rowsum;
  hipLaunchKernelGGL(edge_replay_kernel<false>, dim3((unsigned)((long)B * A * ep.segs)), dim3(256), 0, (hipStream_t)stream, ep);
  return launch_status("edge_replay_kernel (logp)");
}

extern "C" long daco_tsp_edge_backward(void *stream, int B, int n, int k, int A, const float *heu, const int64_t *edge_dst,
                                       long edge_dst_bstride, const int32_t *edge_dst32, float eps, float beta, const int64_t *paths,
                                       const float *rowsum, const float *grad_logp, float *grad_heu) {
  EdgeParams ep = {};
  const long rc = edge_args("daco_tsp_edge_backward", B, n, k, A, heu, edge_dst, edge_dst_bstride, edge_dst32, eps, paths, rowsum, grad_logp,
                            grad_heu, &ep.segs);
  if (rc != DACO_OK) return rc;
  ep.B = B; ep.n = n; ep.k = k; ep.A = A; ep.heu = heu; ep.dst64 = edge_dst; ep.dst64_bs = edge_dst_bstride; ep.dst32 = edge_dst32;
  ep.eps = eps; ep.beta = beta; ep.paths = paths; ep.rowsum_in = rowsum; ep.grad_logp = grad_logp; ep.grad_heu = grad_heu;
  hipLaunchKernelGGL(edge_replay_kernel<true>, dim3((unsigned)((long)B * A * ep.segs)), dim3(256), 0, (hipStream_t)stream, ep);
  return launch_status("edge_replay_kernel (backward)");
}
