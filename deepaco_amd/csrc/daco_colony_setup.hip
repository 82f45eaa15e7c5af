// daco_colony_setup.hip -- what gets a TSP / OP colony ready for its first iteration, as kernels.
//
// Reference behaviour replaced: ACO.sparsify (tsp/aco.py:52-67, op/aco.py: topk / full_like / gather / scatter_ / divide) and, on
// this project's side, the head table of the head-row samplers (engine.sparse_head) and the concentration test of
// sampler='auto' (engine.auto_head_k), which were torch.topk + cumsum + scatter_ on the device.
//
// All three kernels: one wavefront per matrix row, the row in registers (lane l owns columns l, l + 64, ..: any n and any
// alignment loads coalesced), 2 <= n <= 1024 = at most 16 values per lane.  The k-th value of a row is found by a threshold
// search, not by k rounds of arg-max: the floats are taken to their order-preserving 32-bit image (-0.0 counted as +0.0) and
// the threshold is built bit by bit, 32 steps of one compare per owned column and a wave-wide count (ballot + scalar
// popcount).  The selection is then "everything beyond the threshold, and of the entries equal to it those of the smallest
// column ids that still fit": with this layout column order is (chunk, lane), so the rank of a column among the selected ones is
// the popcounts of the earlier chunks' ballots plus the bits below the lane in its own chunk's ballot.
// NaN inputs are outside the contract (some k columns come out, nothing is written out of bounds).
// A fourth kernel, head_eta_kernel (daco_head_eta), serves the uniform-tail mode of the head-row path: also one wavefront per
// row, but it walks the row (no selection) and tests that eta is one number outside the head.
#include "daco_host.h"

namespace daco {

constexpr int CS_MAX_N = 1024;                      // 16 columns per lane
constexpr int CS_HEAD_MAX_K = 127;                  // the head-row samplers' largest head (128 slots, the last one the count)

// order-preserving image of a float: a < b <=> key(a) < key(b), -0.0 and +0.0 on one key
__device__ inline uint32_t cs_key(float v) {
  const uint32_t b = __float_as_uint(v == 0.0f ? 0.0f : v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ inline float cs_unkey(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

// bits of `mask` below this lane
__device__ inline int cs_below(uint64_t mask) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// the k-th largest key of the wave's 64 * CPL keys (1 <= k <= 64 * CPL): the largest t with #(key >= t) >= k
template <int CPL>
__device__ inline uint32_t cs_kth_largest(const uint32_t (&key)[CPL], int k) {
  uint32_t t = 0;
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t cand = t | (1u << bit);
    int cnt = 0;
#pragma unroll
    for (int q = 0; q < CPL; ++q) cnt += __popcll(__ballot(key[q] >= cand));
    if (cnt >= k) t = cand;
  }
  return t;
}

template <int CPL>
__device__ inline int cs_count_above(const uint32_t (&key)[CPL], uint32_t t) {
  int g = 0;
#pragma unroll
  for (int q = 0; q < CPL; ++q) g += __popcll(__ballot(key[q] > t));
  return g;
}

// The k largest by (key descending, column ascending), t = cs_kth_largest(key, k): bit q of the returned mask = column
// lane + 64 q is one of them; pos[q] = how many selected columns come before it in column order.
template <int CPL>
__device__ inline uint32_t cs_choose(const uint32_t (&key)[CPL], int k, uint32_t t, int (&pos)[CPL]) {
  const int room = k - cs_count_above(key, t);            // entries equal to the threshold that still fit (>= 1)
  int eq_before = 0, ch_before = 0;
  uint32_t chosen = 0;
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
    const bool eq = key[q] == t;
    const uint64_t eqs = __ballot(eq);
    const bool c = key[q] > t || (eq && eq_before + cs_below(eqs) < room);
    const uint64_t cs = __ballot(c);
    pos[q] = ch_before + cs_below(cs);
    chosen |= (c ? 1u : 0u) << q;
    eq_before += __popcll(eqs);
    ch_before += __popcll(cs);
  }
  return chosen;
}

// ---- daco_sparsify: out = num / dist on each row's k smallest (value, column), num / 1e10f elsewhere
template <int CPL>
__global__ void __launch_bounds__(256)
sparsify_kernel(int B, int n, int k, const float *dist, long dist_bstride, const float *numer, long numer_bstride, float *out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * 4 + wave;          // b*n + i
  if (row >= (long)B * n) return;
  const int b = (int)(row / n), i = (int)(row % n);
  const float *d = dist + (size_t)b * dist_bstride + (size_t)i * n;
  float v[CPL];
  uint32_t key[CPL];                                      // the smallest distance = the largest key; a lane past the row: below all
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
    const int j = lane + 64 * q;
    v[q] = j < n ? d[j] : 0.0f;
    key[q] = j < n ? ~cs_key(v[q]) : 0u;
  }
  int pos[CPL];
  const uint32_t chosen = cs_choose(key, k, cs_kth_largest(key, k), pos);
  const float *nu = numer ? numer + (size_t)b * numer_bstride : nullptr;
  float *o = out + (size_t)row * n;
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
    const int j = lane + 64 * q;
    if (j < n) o[j] = (nu ? nu[j] : 1.0f) / (((chosen >> q) & 1u) ? v[q] : 1e10f);
  }
}

// ---- daco_sparse_head: ids of each row's k largest (value, column), ascending, in S slots; unused slots 0, slot S-1 = k.
// The table of a row is put together in LDS (256 bytes per wave) and leaves as one coalesced store per instance it serves.
template <int CPL>
__global__ void __launch_bounds__(256)
sparse_head_kernel(int B, int n, int k, int slots, const float *w, long w_bstride, uint16_t *ids) {
  __shared__ uint16_t tab[4][128];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long rows = (w_bstride == 0 ? 1L : (long)B) * n;  // a shared matrix: every row is read once and written B times
  const long row = (long)blockIdx.x * 4 + wave;
  const bool active = row < rows;
  tab[wave][lane] = 0;
  tab[wave][lane + 64] = 0;
  __syncthreads();
  if (active) {
    const float *r = w + (size_t)(row / n) * w_bstride + (size_t)(row % n) * n;
    uint32_t key[CPL];
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
      const int j = lane + 64 * q;
      key[q] = j < n ? cs_key(r[j]) : 0u;
    }
    int pos[CPL];
    const uint32_t chosen = cs_choose(key, k, cs_kth_largest(key, k), pos);
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
      const int j = lane + 64 * q;
      if (((chosen >> q) & 1u) && j < n && pos[q] < k) tab[wave][pos[q]] = (uint16_t)j;
    }
    if (lane == 0) tab[wave][slots - 1] = (uint16_t)k;
  }
  __syncthreads();
  const int words = slots >> 1;
  if (active && lane < words) {
    const uint32_t word = (uint32_t)tab[wave][2 * lane] | ((uint32_t)tab[wave][2 * lane + 1] << 16);
    uint32_t *out = reinterpret_cast<uint32_t *>(ids);
    if (w_bstride == 0) {
      for (int b = 0; b < B; ++b) out[((size_t)b * n + (size_t)row) * words + lane] = word;
    } else {
      out[(size_t)row * words + lane] = word;
    }
  }
}

// ---- daco_head_eta: what the uniform-tail mode of the head-row path needs of eta, once per head table (daco_head_rows.h).
// head_eta[row][m] = eta[row][id_m] for the table's live slots (m < count, id < n), +0 for the others; and the test the mode
// rests on, over all B n rows: every entry outside the head has ONE bit pattern c, a finite number with the sign bit clear
// (-0.0 in the tail is refused: it is not bit-equal to +0.0), and every live head entry is >= c (a NaN fails).
// verdict[0] |= 1 for a row that fails on its own; verdict[1] = max of ~(tail pattern), verdict[2] = max of the tail pattern over
// the rows (patterns with a clear sign bit order as unsigned): the caller accepts when verdict[0] == 0 and ~verdict[1] ==
// verdict[2], and c is that pattern.  (No row has a tail: ~0 != 0, refused.)
__global__ void __launch_bounds__(256)
head_eta_kernel(int B, int n, int slots, const float *eta, long eta_bs, const uint16_t *ids, float *head_eta, uint32_t *verdict) {
  __shared__ uint32_t bm[4][32];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * 4 + wave;
  if (row >= (long)B * n) return;
  const int b = (int)(row / n), r = (int)(row - (long)b * n);
  const float *er = eta + (size_t)b * eta_bs + (size_t)r * n;
  const uint16_t *id = ids + (size_t)row * slots;
  const int cnt = id[slots - 1] < slots - 1 ? id[slots - 1] : slots - 1;
  if (lane < 32) bm[wave][lane] = 0u;
  __builtin_amdgcn_wave_barrier();
  float eh[2];
  bool live[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int m = lane + 64 * j;
    const int k = m < slots ? (int)id[m] : n;
    live[j] = m < cnt && k < n;
    eh[j] = live[j] ? er[k] : 0.0f;
    if (live[j]) atomicOr(&bm[wave][k >> 5], 1u << (k & 31));
    if (m < slots) head_eta[(size_t)row * slots + m] = eh[j];
  }
  __builtin_amdgcn_wave_barrier();
  uint32_t lo = 0xFFFFFFFFu, hi = 0u;                       // the tail's bit patterns: smallest and largest
  for (int k = lane; k < n; k += 64) {
    if ((bm[wave][k >> 5] >> (k & 31)) & 1u) continue;
    const uint32_t u = __float_as_uint(er[k]);
    lo = u < lo ? u : lo;
    hi = u > hi ? u : hi;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t l2 = (uint32_t)__shfl_xor((int)lo, o, 64), h2 = (uint32_t)__shfl_xor((int)hi, o, 64);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  const bool tail = lo <= hi;                               // (a row that is all head: nothing to say about c)
  const float c = __uint_as_float(lo);
  bool bad = tail && (lo != hi || lo >= 0x7f800000u);
#pragma unroll
  for (int j = 0; j < 2; ++j) bad = bad || (tail && live[j] && !(eh[j] >= c));
  const bool any_bad = __ballot(bad) != 0;
  if (lane == 0) {
    if (any_bad) atomicOr(verdict + 0, 1u);
    if (tail) { atomicMax(verdict + 1, ~lo); atomicMax(verdict + 2, hi); }
  }
}

// the wave's total of a double, the same in every lane (a fixed butterfly: deterministic)
__device__ inline double cs_wave_sum(double x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
  return x;
}

// ---- daco_head_stats: rows whose K largest values hold at least `mass` of the row, K = ks[0..2] (K < 1: not asked)
struct HeadStatsArgs { int k[3]; double mass[3]; };

template <int CPL>
__global__ void __launch_bounds__(256)
head_stats_kernel(long rows, int n, const float *w, long w_bstride, HeadStatsArgs a, int32_t *counts) {
  __shared__ int passed[4][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int pass[3] = {0, 0, 0};
  for (long row = (long)blockIdx.x * 4 + wave; row < rows; row += (long)gridDim.x * 4) {
    const float *r = w + (size_t)(row / n) * w_bstride + (size_t)(row % n) * n;
    float v[CPL];
    uint32_t key[CPL];
    double part = 0.0;
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
      const int j = lane + 64 * q;
      v[q] = j < n ? r[j] : 0.0f;
      key[q] = j < n ? cs_key(v[q]) : 0u;
      part += (double)v[q];
    }
    const double tot = cs_wave_sum(part);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (a.k[c] < 1) continue;
      const int K = a.k[c] < n ? a.k[c] : n;
      const uint32_t t = cs_kth_largest(key, K);
      const int above = cs_count_above(key, t);
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < CPL; ++q) s += key[q] > t ? (double)v[q] : 0.0;
      s = cs_wave_sum(s) + (double)(K - above) * (double)cs_unkey(t);
      pass[c] += (s / tot >= a.mass[c]) ? 1 : 0;            // (a NaN ratio fails)
    }
  }
  if (lane == 0) { passed[wave][0] = pass[0]; passed[wave][1] = pass[1]; passed[wave][2] = pass[2]; }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int c = threadIdx.x, sum = passed[0][c] + passed[1][c] + passed[2][c] + passed[3][c];
    if (sum) atomicAdd(counts + c, sum);
  }
}

}  // namespace daco

using namespace daco;

// the instantiated columns per lane: 1, 2, 4, 8, 16 (a row is padded with keys below every value up to the next of them)
#define DACO_CS_DISPATCH(n, LAUNCH) \
  do {                              \
    const int cpl_ = ((n) + 63) / 64; \
    if (cpl_ <= 1) { LAUNCH(1); }     \
    else if (cpl_ <= 2) { LAUNCH(2); } \
    else if (cpl_ <= 4) { LAUNCH(4); } \
    else if (cpl_ <= 8) { LAUNCH(8); } \
    else { LAUNCH(16); }              \
  } while (0)

static int cs_check_size(const char *what, int B, int n) {
  if (n > CS_MAX_N) { set_error("%s: n=%d exceeds %d (one row per wavefront, in registers)", what, n, CS_MAX_N); return DACO_E_TOOLARGE; }
  if ((long)B * n > 0x7fffffffL) { set_error("%s: B * n = %ld rows do not fit 32 bits", what, (long)B * n); return DACO_E_TOOLARGE; }
  return DACO_OK;
}

extern "C" long daco_sparsify(void *stream, int B, int n, int k, const float *dist, long dist_bstride, const float *numer,
                             long numer_bstride, float *out) {
  if (B <= 0 || n < 2 || k < 1 || k > n || !dist || !out || dist_bstride < 0 || numer_bstride < 0) {
    set_error("daco_sparsify: bad argument (B=%d n=%d k=%d)", B, n, k);
    return DACO_E_BADARG;
  }
  if (const int rc = cs_check_size("daco_sparsify", B, n)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(((long)B * n + 3) / 4)), block(256);
#define DACO_CS_SPARSIFY(C) hipLaunchKernelGGL(sparsify_kernel<C>, grid, block, 0, s, B, n, k, dist, dist_bstride, numer, numer_bstride, out)
  DACO_CS_DISPATCH(n, DACO_CS_SPARSIFY);
#undef DACO_CS_SPARSIFY
  return launch_status("sparsify_kernel");
}

extern "C" long daco_sparse_head(void *stream, int B, int n, int k, const float *weights, long w_bstride, uint16_t *ids) {
  if (B <= 0 || n < 2 || k < 1 || k > n || k > CS_HEAD_MAX_K || !weights || !ids || w_bstride < 0) {
    set_error("daco_sparse_head: bad argument (B=%d n=%d k=%d, k <= %d)", B, n, k, CS_HEAD_MAX_K);
    return DACO_E_BADARG;
  }
  if (const int rc = cs_check_size("daco_sparse_head", B, n)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const long rows = (w_bstride == 0 ? 1L : (long)B) * n;
  const int slots = k <= 63 ? 64 : 128;
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
#define DACO_CS_HEAD(C) hipLaunchKernelGGL(sparse_head_kernel<C>, grid, block, 0, s, B, n, k, slots, weights, w_bstride, ids)
  DACO_CS_DISPATCH(n, DACO_CS_HEAD);
#undef DACO_CS_HEAD
  return launch_status("sparse_head_kernel");
}

extern "C" long daco_head_stats(void *stream, int B, int n, const float *weights, long w_bstride, int k_lds, double mass,
                               double mass_lds, int32_t *counts) {
  if (B <= 0 || n < 2 || !weights || !counts || w_bstride < 0) {
    set_error("daco_head_stats: bad argument (B=%d n=%d)", B, n);
    return DACO_E_BADARG;
  }
  if (const int rc = cs_check_size("daco_head_stats", B, n)) return rc;
  hipStream_t s = (hipStream_t)stream;
  // (cleared by a kernel: a captured graph of this library holds kernel nodes only -- zero_async in daco_device.h)
  if (const int rc = launch_status(zero_async(counts, 3 * sizeof(int32_t), s), "daco_head_stats (clearing the counters)")) return rc;
  const long rows = (w_bstride == 0 ? 1L : (long)B) * n;
  const HeadStatsArgs a = {{63, 127, k_lds}, {mass, mass, mass_lds}};
  const long want = (rows + 3) / 4;
  const dim3 grid((unsigned)(want < 1024 ? want : 1024)), block(256);       // (the waves walk the rows: at most 3 * 1024 atomics)
#define DACO_CS_STATS(C) hipLaunchKernelGGL(head_stats_kernel<C>, grid, block, 0, s, rows, n, weights, w_bstride, a, counts)
  DACO_CS_DISPATCH(n, DACO_CS_STATS);
#undef DACO_CS_STATS
  return launch_status("head_stats_kernel");
}

extern "C" long daco_head_eta(void *stream, int B, int n, const float *eta, long eta_bstride, const uint16_t *head_id, int head_slots,
                              float *head_eta, uint32_t *verdict) {
  if (B <= 0 || n < 2 || !eta || !head_id || !head_eta || !verdict || eta_bstride < 0 || (head_slots != 64 && head_slots != 128)) {
    set_error("daco_head_eta: bad argument (B=%d n=%d head_slots=%d)", B, n, head_slots);
    return DACO_E_BADARG;
  }
  if (const int rc = cs_check_size("daco_head_eta", B, n)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (const int rc = launch_status(zero_async(verdict, 3 * sizeof(uint32_t), s), "daco_head_eta (clearing the verdict)")) return rc;
  hipLaunchKernelGGL(head_eta_kernel, dim3((unsigned)(((long)B * n + 3) / 4)), dim3(256), 0, s, B, n, head_slots, eta, eta_bstride, head_id,
                     head_eta, verdict);
  return launch_status("head_eta_kernel");
}
