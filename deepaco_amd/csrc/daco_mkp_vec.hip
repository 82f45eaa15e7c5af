// daco_mkp_vec.hip -- the vector-pheromone knapsack colony of mkp_transformer/aco.py: construction, its gradient
// with respect to the heuristic, and the pheromone update.
//
// Reference behaviour replaced:
//   mkp_transformer/aco.py:111-178 gen_sol / pick_item / update_dummy_state / update_knapsack (a Python loop of
//     ~20 aten ops per step plus a per-ant Python loop for the capacity rule), fused with :101-109 gen_sol_obj;
//   autograd through Categorical(dist).log_prob of :141-148 (the REINFORCE loss of mkp_transformer/train.py:26-30);
//   mkp_transformer/aco.py:85-99 update_pheronome, with run()'s best tracking of :71-83.
//
// What differs from mkp/ (DACO_SIB_MKP): pheromone and heuristic are VECTORS over the items (dummy item last), so
// every draw of every ant uses the same weights w_k = tau_k^alpha * eta_k^beta and only the open set differs; the
// first item is drawn like every other one and has a log-probability; every capacity is 1.
//
// Construction.  One wavefront per (instance, ant), four ants of an instance per workgroup.  Candidate
// k = (c*64 + lane)*4 + v (the layout of daco_device.h with VEC = 4), so a lane holds NJ = 4*CH candidates, CH = 1, 2, 4
// for n <= 256, 512, 1024.  w_k is formed once and stays in registers next to a bit per candidate (open / closed).
// The workgroup stages the instance's item weights in LDS transposed, Wt[d][k] (a lane's four candidates are one
// 16-byte read, 64 lanes read consecutive addresses), and the prices behind them: (m + 1) * 256 * CH floats, 36 KB at
// the limit.  A step reads no global memory except the RACE_NOISE tensor: close what no longer fits, draw, broadcast
// the pick, add its m weights to the knapsack (uniform LDS reads).  The closure rule of :159-178 --
// "if more than one candidate is open counting the dummy" -- always holds while a real item is open (the dummy's mask
// entry is reset to 1 after every pass), so it reduces to: every open item k with any_d(knapsack_d + W[k][d] > 1)
// closes for good (strict, float32, knapsack summed in pick order).  An ant whose real items are all closed is done:
// the reference keeps drawing the dummy with probability 1 until the slowest ant is done, which is the padding written
// here (dummy, log(1 - eps)).  Draws, noise layout and Philox counters are those of daco_sibling_sample; the draw
// index t = 0, 1, ... takes the step number t + 1 (the siblings' first draw is step 1 as well).
//
// Backward.  d log p_t / d eta_k = beta * ([k = pick] / eta_k - w_k m_k / (eta_k S_t)), zero where the probability
// was clamped.  A wavefront replays its ant (same closure code), keeps its candidates' sums in registers over all
// steps -- w_k / eta_k does not depend on the step, so a step costs one multiply-add per open candidate -- the four
// ants of a workgroup are combined in LDS and the workgroup adds each non-zero sum to grad_eta once.
//
// Update.  One workgroup per instance, a thread per item (four items per thread above 256).  The ants' amounts
// Q * obj are added in ant order, membership from a per-ant bitmap built in LDS from the solutions (64 ants at a
// time), so duplicate entries of a solution (the dummy padding) count once, as the reference's index-put does, and
// the result does not depend on any atomic's order: bit-identical to the reference's loop.
#include "daco_sample_kernel.h"

namespace daco {

constexpr int MKPV_MAX_ITEMS = 1024;     // items including the dummy: 16 candidates per lane

struct MkpvParams {
  int B, n, A, m, Lmax, noise_steps;     // n counts the dummy item n-1
  const float *tau, *eta;                // [B][n]
  long tau_bs, eta_bs;
  float alpha, beta;
  const float *wts;                      // [B][n][m]
  const float *price;                    // [B][n] or null
  const float *noise;                    // RACE_NOISE: [B][noise_steps][A][n]
  uint64_t seed, iter;
  uint32_t ant_gid0;
  int64_t *sols;                         // [B][Lmax][A]
  int32_t *lens;                         // [B][A]
  float *logp, *rowsum;                  // [B][Lmax][A] or null
  float *objs;                           // [B][A] or null
  int32_t *flags;                        // [B] or null
  // backward
  const float *grad_logp;                // [B][Lmax][A]
  float *grad_eta;                       // [B][n]
};

// the instance's item weights into LDS, transposed: Wt[d * ld + k]; candidates past n are never open (not initialised)
__device__ inline void stage_weights(float *Wt, const float *wts_b, int n, int m, int ld) {
  for (int i = threadIdx.x; i < n * m; i += blockDim.x) {
    const int k = i / m, d = i - k * m;
    Wt[d * ld + k] = wts_b[i];
  }
}

// mkp_transformer/aco.py:169-176: an open item that no longer fits in some dimension closes for good
template <int CH>
__device__ inline uint32_t close_full(uint32_t open, const float *Wt, const float (&knap)[8], int m, int lane) {
  constexpr int ld = CH * 256;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    if (((open >> (4 * c)) & 15u) == 0u) continue;
    const int k0 = (c * 64 + lane) * 4;
    bool over[4] = {false, false, false, false};
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      if (d < m) {
        const float4 x = *reinterpret_cast<const float4 *>(Wt + d * ld + k0);
        over[0] = over[0] || (knap[d] + x.x > 1.0f);
        over[1] = over[1] || (knap[d] + x.y > 1.0f);
        over[2] = over[2] || (knap[d] + x.z > 1.0f);
        over[3] = over[3] || (knap[d] + x.w > 1.0f);
      }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) if (over[v]) open &= ~(1u << (4 * c + v));
  }
  return open;
}

template <int CH, int MODE, bool LOGP>
__global__ void __launch_bounds__(256)
mkpv_sample_kernel(const MkpvParams p) {
  constexpr int NJ = CH * 4, ld = CH * 256;
  extern __shared__ __attribute__((aligned(16))) float mkpv_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bpi = (p.A + 3) >> 2;
  const int b = blockIdx.x / bpi;
  const int a = (blockIdx.x - b * bpi) * 4 + wave;
  const int n = p.n, m = p.m, A = p.A;
  float *Wt = mkpv_lds;                                 // [m][ld]
  float *price = mkpv_lds + m * ld;                     // [ld]
  stage_weights(Wt, p.wts + (size_t)b * n * m, n, m, ld);
  if (p.price) for (int k = threadIdx.x; k < n; k += blockDim.x) price[k] = p.price[(size_t)b * n + k];
  __syncthreads();
  if (a >= A) return;                                   // (no barrier below)

  const float *tau = p.tau + (size_t)b * p.tau_bs, *eta = p.eta + (size_t)b * p.eta_bs;
  const uint32_t gid = p.ant_gid0 + (uint32_t)(b * A + a);
  float w[NJ], rinv[MODE == DACO_RACE_PHILOX ? NJ : 1];
  uint32_t open = 0;
  static_for<NJ>([&](auto J) {
    constexpr int j = J, c = j / 4, v = j % 4;
    const int k = (c * 64 + lane) * 4 + v;
    w[j] = k < n ? pw(tau[k], p.alpha) * pw(eta[k], p.beta) : 0.0f;
    if constexpr (MODE == DACO_RACE_PHILOX) rinv[j] = k < n ? 1.0f / w[j] : __builtin_inff();
    if (k < n - 1) open |= 1u << j;                      // the dummy is never a candidate of a running ant
  });
  float knap[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float obj = 0.0f;
  int64_t *sol_out = p.sols + (size_t)b * p.Lmax * A + a;
  float *logp_out = LOGP ? p.logp + (size_t)b * p.Lmax * A + a : nullptr;
  float *rs_out = (LOGP && p.rowsum) ? p.rowsum + (size_t)b * p.Lmax * A + a : nullptr;

  u32x4 ublk = {0, 0, 0, 0};
  uint32_t ucur = 0;
  bool infeasible = false, overflow = false;
  int t = 0;
  for (;;) {
    open = close_full<CH>(open, Wt, knap, m, lane);
    if (__ballot(open != 0u) == 0) break;               // nothing left to add: the ant rests on the dummy
    if (t >= p.Lmax || (MODE == DACO_RACE_NOISE && t >= p.noise_steps)) { overflow = true; break; }
    const int step = t + 1;
    float row[NJ];
    float part = 0.0f;
    static_for<NJ>([&](auto J) {
      constexpr int j = J;
      row[j] = ((open >> j) & 1u) ? w[j] : 0.0f;
      part = j == 0 ? row[j] : part + row[j];           // (+0.0f + x == x)
    });
    int choice = -1;
    float pchoice = 0.0f, S = 0.0f;
    if constexpr (MODE == DACO_SCAN) {
      // uniform for step s: lane (s&63), component (s>>6)&3 of the Philox block (s>>8)*64 + lane
      if ((step & 63) == 0 || t == 0) {
        if ((step & 255) == 0 || t == 0) ublk = rng_block(p.seed, p.iter, STREAM_SCAN, gid, (uint32_t)(((step >> 8) << 6) + lane));
        ucur = comp(ublk, (step >> 6) & 3);
      }
      const uint32_t ux = (uint32_t)readlane_i((int)ucur, step & 63);
      float pre[NJ];
      float run = 0.0f;
      static_for<NJ>([&](auto J) { constexpr int j = J; run = j == 0 ? row[j] : run + row[j]; pre[j] = run; });
      const float incl = wave_scan_add(part);
      S = readlane_f(incl, 63);
      float r = u01(ux) * S;
      r = r > 0.0f ? r : 1.401298464e-45f;              // keep r > 0 if u*S underflows
      const uint64_t hit = __ballot(incl >= r && part > 0.0f);
      if (hit != 0) {
        const int L = __builtin_ctzll(hit);
        const float excl = L ? readlane_f(incl, L - 1) : 0.0f;
        const float thr = r - excl;
        int cnt = 0, last = 0;
        static_for<NJ>([&](auto J) { constexpr int j = J; cnt += pre[j] < thr ? 1 : 0; last = row[j] > 0.0f ? j : last; });
        int jsel = readlane_i(cnt, L);
        if (jsel >= NJ) jsel = readlane_i(last, L);     // rounding: the lane's own sum fell short of r - excl
        float wsel = 0.0f;
        static_for<NJ>([&](auto J) { constexpr int j = J; wsel = j == jsel ? row[j] : wsel; });
        pchoice = readlane_f(wsel, L);
        choice = (((jsel >> 2) * 64 + L) << 2) + (jsel & 3);
        if (!(pchoice > 0.0f)) choice = -1;
      }
    } else if constexpr (MODE == DACO_RACE_PHILOX) {
      float bk = __builtin_inff();
      int bi = 0x7fffffff;
      u32x4 r4{};
      static_for<NJ>([&](auto J) {
        constexpr int j = J, c = j / 4, v = j % 4;
        const int k = (c * 64 + lane) * 4 + v;
        // one Philox block serves candidates 4g..4g+3: a lane's four candidates of a chunk
        if (v == 0) r4 = rng_block(p.seed, p.iter, STREAM_RACE, gid, ((uint32_t)step << 12) | (uint32_t)(k >> 2));
        const float Lk = neg_log2_1m(u01(comp(r4, v)));
        const float key = ((open >> j) & 1u) ? Lk * rinv[j] : __builtin_inff();
        if (key < bk) { bk = key; bi = k; }
      });
      const KeyIdx r = wave_arg<false>(bk, bi);
      if (r.key < __builtin_inff()) choice = r.idx;
      if constexpr (LOGP) {
        S = wave_sum(part);
        if (choice >= 0) {
          float wsel = 0.0f;
          const int jsel = ((choice >> 8) << 2) + (choice & 3);
          static_for<NJ>([&](auto J) { constexpr int j = J; wsel = j == jsel ? w[j] : wsel; });
          pchoice = readlane_f(wsel, (choice >> 2) & 63);
        }
      }
    } else {  // DACO_RACE_NOISE: the arithmetic of Categorical's normalisation and torch.multinomial's one-sample path
      const float *q = p.noise + (((size_t)b * p.noise_steps + t) * A + a) * n;
      S = wave_sum(part);
      float bk = -__builtin_inff(), bp = 0.0f;
      int bi = 0x7fffffff;
      static_for<NJ>([&](auto J) {
        constexpr int j = J, c = j / 4, v = j % 4;
        const int k = (c * 64 + lane) * 4 + v;
        if (k < n) {
          const float pk = row[j] / S;
          const float key = pk / q[k];
          if (key > bk) { bk = key; bi = k; bp = pk; }
        }
      });
      const KeyIdx r = wave_arg<true>(bk, bi);
      if (r.key > 0.0f) choice = r.idx;
      if (choice >= 0) pchoice = readlane_f(bp, (choice >> 2) & 63);     // already normalised
    }
    choice = __builtin_amdgcn_readfirstlane(choice);
    if (choice < 0) { infeasible = true; break; }        // every open candidate has weight 0
    if constexpr (LOGP) {
      if (lane == 0) {
        logp_out[(size_t)t * A] = clamp_log(MODE == DACO_RACE_NOISE ? pchoice : pchoice / S);
        if (rs_out) rs_out[(size_t)t * A] = S;
      }
    }
    if (lane == ((choice >> 2) & 63)) open &= ~(1u << (((choice >> 8) << 2) + (choice & 3)));
#pragma unroll
    for (int d = 0; d < 8; ++d) if (d < m) knap[d] = knap[d] + Wt[d * ld + choice];
    if (p.price) obj = obj + price[choice];              // mkp_transformer/aco.py:109 (price of the dummy: 0), in pick order
    if (lane == 0) sol_out[(size_t)t * A] = choice;
    ++t;
  }
  // the reference steps every ant until the slowest one is done: a done ant keeps drawing the dummy (probability 1)
  const float lp1 = clamp_log(1.0f);
  for (int tt = t + lane; tt < p.Lmax; tt += 64) {
    sol_out[(size_t)tt * A] = n - 1;
    if constexpr (LOGP) {
      logp_out[(size_t)tt * A] = lp1;
      if (rs_out) rs_out[(size_t)tt * A] = 1.0f;
    }
  }
  if (lane == 0) {
    p.lens[(size_t)b * A + a] = t;
    if (p.objs) p.objs[(size_t)b * A + a] = obj;
    if (p.flags && (infeasible || overflow)) atomicOr(p.flags + b, (infeasible ? 1 : 0) | (overflow ? 2 : 0));
  }
}

template <int CH>
__global__ void __launch_bounds__(256)
mkpv_backward_kernel(const MkpvParams p) {
  constexpr int NJ = CH * 4, ld = CH * 256;
  extern __shared__ __attribute__((aligned(16))) float mkpv_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bpi = (p.A + 3) >> 2;
  const int b = blockIdx.x / bpi;
  const int a = (blockIdx.x - b * bpi) * 4 + wave;
  const int n = p.n, m = p.m, A = p.A;
  float *Wt = mkpv_lds;                                 // [m][ld]
  float *gsum = mkpv_lds + m * ld;                      // [ld] the workgroup's sums
  stage_weights(Wt, p.wts + (size_t)b * n * m, n, m, ld);
  for (int k = threadIdx.x; k < ld; k += blockDim.x) gsum[k] = 0.0f;
  __syncthreads();
  if (a < A) {
    const float *tau = p.tau + (size_t)b * p.tau_bs, *eta = p.eta + (size_t)b * p.eta_bs;
    float dk[NJ], acc[NJ];
    uint32_t open = 0;
    static_for<NJ>([&](auto J) {
      constexpr int j = J, c = j / 4, v = j % 4;
      const int k = (c * 64 + lane) * 4 + v;
      acc[j] = 0.0f;
      dk[j] = 0.0f;
      if (k < n) {
        const float tk = tau[k], e = eta[k];
        dk[j] = dprob_deta(pw(tk, p.alpha) * pw(e, p.beta), tk, e, p.alpha, p.beta);
      }
      if (k < n - 1) open |= 1u << j;
    });
    float knap[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int64_t *sol = p.sols + (size_t)b * p.Lmax * A + a;
    const float *rs = p.rowsum + (size_t)b * p.Lmax * A + a;
    const float *gl = p.grad_logp + (size_t)b * p.Lmax * A + a;
    int len = p.lens[(size_t)b * A + a];
    len = len < p.Lmax ? len : p.Lmax;
    for (int t = 0; t < len; ++t) {
      open = close_full<CH>(open, Wt, knap, m, lane);
      const int64_t j64 = sol[(size_t)t * A];
      if (j64 < 0 || j64 >= n - 1) break;                // not a solution of the construction kernel
      const int j = (int)j64;
      const float g = gl[(size_t)t * A], S = rs[(size_t)t * A];
      if (g != 0.0f) {
        const float ej = eta[j];
        const float pr = (pw(tau[j], p.alpha) * pw(ej, p.beta)) / S;
        if (pr > DACO_EPS_F32 && pr < 1.0f - DACO_EPS_F32) {      // inside the clamp: gradient flows
          const float cg = g / S;
          const int jown = lane == ((j >> 2) & 63) ? ((j >> 8) << 2) + (j & 3) : -1;
          static_for<NJ>([&](auto J) {
            constexpr int jj = J;
            if ((open >> jj) & 1u) {
              float val = -cg * dk[jj];
              if (jj == jown) val += g * p.beta / ej;
              acc[jj] = acc[jj] + val;
            }
          });
        }
      }
      if (lane == ((j >> 2) & 63)) open &= ~(1u << (((j >> 8) << 2) + (j & 3)));
#pragma unroll
      for (int d = 0; d < 8; ++d) if (d < m) knap[d] = knap[d] + Wt[d * ld + j];
    }
    static_for<NJ>([&](auto J) {
      constexpr int j = J, c = j / 4, v = j % 4;
      const int k = (c * 64 + lane) * 4 + v;
      if (k < n && acc[j] != 0.0f) unsafeAtomicAdd(gsum + k, acc[j]);
    });
  }
  __syncthreads();
  float *grad = p.grad_eta + (size_t)b * n;
  for (int k = threadIdx.x; k < n; k += blockDim.x)
    if (gsum[k] != 0.0f) unsafeAtomicAdd(grad + k, gsum[k]);       // one flush per workgroup; items no draw had open stay untouched
}

struct MkpvUpdateParams {
  int B, n, A, rows;
  const int64_t *sols;       // [B][rows][A]
  const int32_t *lens;       // [B][A] or null (every row counts)
  const float *objs;         // [B][A]
  const float *Q;            // [B]
  float decay;
  int elitist, min_max;
  float tmin, tmax;
  float *tau;                // [B][n]
  float *best_obj;           // [B] or null
  int64_t *best_sol;         // [B][rows] or null
};

constexpr int MKPV_TILE = 64;      // ants whose membership bitmaps are in LDS at a time

__global__ void __launch_bounds__(256)
mkpv_update_kernel(const MkpvUpdateParams p) {
  __shared__ uint32_t bm[MKPV_TILE][MKPV_MAX_ITEMS / 32];
  __shared__ float amt[MKPV_TILE];
  __shared__ float red_v[256];
  __shared__ int red_i[256];
  __shared__ int s_best, s_len, s_new;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = p.n, A = p.A;
  const int64_t *sols = p.sols + (size_t)b * p.rows * A;
  const float *objs = p.objs + (size_t)b * A;
  // ---- rows in use (the longest ant) and the first maximum of the objectives (mkp_transformer/aco.py:77)
  int len = 0, bi = 0x7fffffff;
  float bv = -__builtin_inff();
  for (int a = tid; a < A; a += 256) {
    const int l = p.lens ? p.lens[(size_t)b * A + a] : p.rows;
    len = l > len ? l : len;
    const float v = objs[a];
    if (v > bv || bi == 0x7fffffff) { bv = v; bi = a; }
  }
  red_v[tid] = bv; red_i[tid] = bi;
  if (tid == 0) s_len = 0;
  __syncthreads();
  atomicMax(&s_len, len);
  if (tid == 0) {
    float v = red_v[0];
    int i = red_i[0];
    for (int k = 1; k < 256; ++k)
      if (red_i[k] != 0x7fffffff && (red_v[k] > v || (red_v[k] == v && red_i[k] < i))) { v = red_v[k]; i = red_i[k]; }
    s_best = i;
    s_new = 0;
    if (p.best_obj && v > p.best_obj[b]) { p.best_obj[b] = v; s_new = 1; }     // strict: the first best stays (:78)
  }
  __syncthreads();
  const int best = s_best;
  int L = s_len;
  L = L < p.rows ? L : p.rows;
  if (s_new && p.best_sol)
    for (int t = tid; t < p.rows; t += 256) p.best_sol[(size_t)b * p.rows + t] = sols[(size_t)t * A + best];
  // ---- evaporation, then the ants' amounts in ant order (:87-95)
  float *tau = p.tau + (size_t)b * n;
  float v4[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { const int k = tid + 256 * i; v4[i] = k < n ? tau[k] * p.decay : 0.0f; }
  const float Q = p.Q[b];
  const int a_lo = p.elitist ? best : 0, a_hi = p.elitist ? best + 1 : A;
  for (int a0 = a_lo; a0 < a_hi; a0 += MKPV_TILE) {
    const int cnt = a_hi - a0 < MKPV_TILE ? a_hi - a0 : MKPV_TILE;
    for (int i = tid; i < MKPV_TILE * (MKPV_MAX_ITEMS / 32); i += 256) (&bm[0][0])[i] = 0u;
    if (tid < cnt) amt[tid] = Q * objs[a0 + tid];
    __syncthreads();
    for (int i = tid; i < L * MKPV_TILE; i += 256) {
      const int t = i / MKPV_TILE, al = i % MKPV_TILE;
      if (al < cnt) {
        const int64_t item = sols[(size_t)t * A + a0 + al];
        if (item >= 0 && item < n) atomicOr(&bm[al][item >> 5], 1u << (item & 31));
      }
    }
    __syncthreads();
    for (int al = 0; al < cnt; ++al) {
      const float x = amt[al];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = tid + 256 * i;                     // (k < 1024: inside the bitmap)
        if ((bm[al][k >> 5] >> (k & 31)) & 1u) v4[i] = v4[i] + x;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = tid + 256 * i;
    if (k < n) {
      float x = v4[i];
      if (p.min_max) {
        // :98 reads ((tau > 1e-9) * tau) < min: the product is compared, so EVERY entry below min is raised to min
        x = (x > 1e-9f ? x : 0.0f * x) < p.tmin ? p.tmin : x;
        x = x > p.tmax ? p.tmax : x;
      }
      tau[k] = x;
    }
  }
}

template <int CH>
static hipError_t launch_mkpv_sample(const MkpvParams &p, int mode, hipStream_t s) {
  dim3 grid((unsigned)(p.B * ((p.A + 3) / 4))), block(256);
  const size_t dyn = (size_t)(p.m + 1) * CH * 256 * sizeof(float);
  const bool lp = p.logp != nullptr;
#define MKPV_LAUNCH(M, L) hipLaunchKernelGGL((mkpv_sample_kernel<CH, M, L>), grid, block, dyn, s, p)
  if (mode == DACO_SCAN) { if (lp) MKPV_LAUNCH(DACO_SCAN, true); else MKPV_LAUNCH(DACO_SCAN, false); }
  else if (mode == DACO_RACE_PHILOX) { if (lp) MKPV_LAUNCH(DACO_RACE_PHILOX, true); else MKPV_LAUNCH(DACO_RACE_PHILOX, false); }
  else { if (lp) MKPV_LAUNCH(DACO_RACE_NOISE, true); else MKPV_LAUNCH(DACO_RACE_NOISE, false); }
#undef MKPV_LAUNCH
  return hipGetLastError();
}

}  // namespace daco

using namespace daco;

static int mkpv_check_sizes(const char *who, int B, int n, int A, int m) {
  if (B <= 0 || n < 2 || A <= 0) { set_error("%s: bad argument (B=%d n=%d A=%d)", who, B, n, A); return DACO_E_BADARG; }
  if (m < 1 || m > 8) { set_error("%s: 1 <= m <= 8 knapsack dimensions (m=%d)", who, m); return DACO_E_BADARG; }
  if (n > MKPV_MAX_ITEMS) { set_error("%s: n=%d items (with the dummy) exceed %d", who, n, MKPV_MAX_ITEMS); return DACO_E_TOOLARGE; }
  return DACO_OK;
}

extern "C" int daco_mkpv_sample(void *stream, int B, int n, int A, int m, const float *tau, long tau_bstride,
                                const float *eta, long eta_bstride, float alpha, float beta,
                                const float *item_weights, const float *price, int mode, const float *noise,
                                int noise_steps, uint64_t seed, uint64_t iter, uint32_t ant_gid0, int Lmax,
                                int64_t *sols, int32_t *lens, float *logp, float *rowsum, float *objs, int32_t *flags) {
  if (const int rc = mkpv_check_sizes("daco_mkpv_sample", B, n, A, m)) return rc;
  if (!tau || !eta || !item_weights || !sols || !lens) { set_error("daco_mkpv_sample: bad argument (null pointer)"); return DACO_E_BADARG; }
  if (Lmax < 1) { set_error("daco_mkpv_sample: bad argument (Lmax=%d)", Lmax); return DACO_E_BADARG; }
  if (mode == DACO_SCAN_WAVE) mode = DACO_SCAN;
  if (mode < 0 || mode > 2) { set_error("daco_mkpv_sample: bad mode %d", mode); return DACO_E_BADARG; }
  if (mode == DACO_RACE_NOISE && (!noise || noise_steps <= 0)) { set_error("daco_mkpv_sample: DACO_RACE_NOISE needs a noise tensor"); return DACO_E_BADARG; }
  if (rowsum && !logp) { set_error("daco_mkpv_sample: rowsum needs logp"); return DACO_E_BADARG; }
  MkpvParams p{};
  p.B = B; p.n = n; p.A = A; p.m = m; p.Lmax = Lmax; p.noise_steps = noise_steps;
  p.tau = tau; p.eta = eta; p.tau_bs = tau_bstride; p.eta_bs = eta_bstride; p.alpha = alpha; p.beta = beta;
  p.wts = item_weights; p.price = price; p.noise = noise; p.seed = seed; p.iter = iter; p.ant_gid0 = ant_gid0;
  p.sols = sols; p.lens = lens; p.logp = logp; p.rowsum = rowsum; p.objs = price ? objs : nullptr; p.flags = flags;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = n <= 256 ? launch_mkpv_sample<1>(p, mode, s) : (n <= 512 ? launch_mkpv_sample<2>(p, mode, s) : launch_mkpv_sample<4>(p, mode, s));
  return launch_status(e, "mkpv_sample_kernel");
}

extern "C" int daco_mkpv_backward(void *stream, int B, int n, int A, int m, int rows, const float *tau, long tau_bstride,
                                  const float *eta, long eta_bstride, float alpha, float beta, const float *item_weights,
                                  const int64_t *sols, const float *rowsum, const float *grad_logp, const int32_t *lens,
                                  float *grad_eta) {
  if (const int rc = mkpv_check_sizes("daco_mkpv_backward", B, n, A, m)) return rc;
  if (!tau || !eta || !item_weights || !sols || !rowsum || !grad_logp || !lens || !grad_eta) { set_error("daco_mkpv_backward: bad argument (null pointer)"); return DACO_E_BADARG; }
  if (rows < 1) { set_error("daco_mkpv_backward: bad argument (rows=%d)", rows); return DACO_E_BADARG; }
  MkpvParams p{};
  p.B = B; p.n = n; p.A = A; p.m = m; p.Lmax = rows;
  p.tau = tau; p.eta = eta; p.tau_bs = tau_bstride; p.eta_bs = eta_bstride; p.alpha = alpha; p.beta = beta;
  p.wts = item_weights; p.sols = const_cast<int64_t *>(sols); p.rowsum = const_cast<float *>(rowsum);
  p.lens = const_cast<int32_t *>(lens); p.grad_logp = grad_logp; p.grad_eta = grad_eta;
  dim3 grid((unsigned)(B * ((A + 3) / 4))), block(256);
  hipStream_t s = (hipStream_t)stream;
  const int CH = n <= 256 ? 1 : (n <= 512 ? 2 : 4);
  const size_t dyn = (size_t)(m + 1) * CH * 256 * sizeof(float);
  if (CH == 1) hipLaunchKernelGGL(mkpv_backward_kernel<1>, grid, block, dyn, s, p);
  else if (CH == 2) hipLaunchKernelGGL(mkpv_backward_kernel<2>, grid, block, dyn, s, p);
  else hipLaunchKernelGGL(mkpv_backward_kernel<4>, grid, block, dyn, s, p);
  return launch_status("mkpv_backward_kernel");
}

extern "C" int daco_mkpv_update(void *stream, int B, int n, int A, int rows, const int64_t *sols, const int32_t *lens,
                                const float *objs, const float *Q, float decay, int elitist, int min_max, float tmin,
                                float tmax, float *tau, float *best_obj, int64_t *best_sol) {
  if (B <= 0 || n < 2 || A <= 0 || rows < 1 || !sols || !objs || !Q || !tau) {
    set_error("daco_mkpv_update: bad argument (B=%d n=%d A=%d rows=%d)", B, n, A, rows);
    return DACO_E_BADARG;
  }
  if (n > MKPV_MAX_ITEMS) { set_error("daco_mkpv_update: n=%d items (with the dummy) exceed %d", n, MKPV_MAX_ITEMS); return DACO_E_TOOLARGE; }
  if (best_sol && !best_obj) { set_error("daco_mkpv_update: best_sol needs best_obj"); return DACO_E_BADARG; }
  MkpvUpdateParams p{};
  p.B = B; p.n = n; p.A = A; p.rows = rows; p.sols = sols; p.lens = lens; p.objs = objs; p.Q = Q; p.decay = decay;
  p.elitist = elitist; p.min_max = min_max; p.tmin = tmin; p.tmax = tmax; p.tau = tau; p.best_obj = best_obj; p.best_sol = best_sol;
  hipLaunchKernelGGL(mkpv_update_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, p);
  return launch_status("mkpv_update_kernel");
}
