// daco_cvrp_adaptive.hip -- the three phases of the "adaptive elitist AS" that shares the reference's cvrp/aco.py (lines 207-383):
//   improvement_phase      -> cvrp_reinsert_kernel   (cheapest-insertion rebuild of the selected ants' subroutes)
//   intensification_phase  -> cvrp_n1_kernel         (the record of run(), :81-93, and the N1 relocation on a new record)
//   update_pheronome / diversification_phase / the elite pool -> cvrp_adaptive_update_kernel (per instance, one of the two)
// and the one phase in which cvrp_nls/aco.py's copy of that baseline (:289-441) differs:
//   intensification_phase with N1 AND N2 (:313-394, 419-434) -> cvrp_intensify_kernel (one workgroup per instance, a wavefront per trial)
// Restated in plain Python in tests/cvrp_adaptive_spec.py, which tests/golden/a1_*.npz pin on the reference itself, and in
// tests/cvrp_nls_adaptive_spec.py (tests/golden/a2_*.npz).
//
// Arithmetic: an insertion's added length is
// (d[p1][c] + d[c][p2]) - d[p1][p2] in float32, two roundings, no contraction (the Makefile's -ffp-contract=off); the minimum
// over positions takes the smallest position among equals (the reference's min over (cost, i) tuples); a subroute's cost is the
// double sum of its float32 deltas in insertion order, an ant's the double sum of those in subroute order.
//
// Lane mapping.  A wavefront owns one ant (reinsertion) or one instance (N1); the route under construction lives in LDS as u16
// node ids and the 64 lanes take 64 consecutive insertion positions at a time: three gathers from the distance matrix per lane,
// one (key, index) DPP reduction (daco_device.h wave_arg, ties to the smaller index), and a running minimum across the chunks
// of 64 that is replaced on strict < only, so that a tie between two chunks keeps the earlier one.  A CVRP route under capacity
// 50 holds about ten customers, so most lanes of a scan idle; the phases are a chain of gather latencies either way, and what a
// block gains instead is one wavefront per selected ant, all of an instance's ants in flight at once.
//
// What the kernels share is written once, as inline device functions: best_gap (the insertion scan, with or without a skipped
// entry), first_min, load_route (a route column into LDS: all three route-reading kernels), and for the two intensification
// kernels for_each_subroute (the walk over a route's consecutive depots; the reinsertion keeps that walk as text of its own, for
// the reason given there), RouteTables (the LDS layout, carved and sized side by side), take_record, lay_record, n1_draws,
// n1_trial, apply_n1 and record_tail.  cvrp_n1_kernel is those in a row with five
// trials in one wavefront; cvrp_intensify_kernel runs one n1_trial per wavefront beside N2's, which only it has.
#include "daco_host.h"

namespace daco {

constexpr uint32_t STREAM_N1 = 4;            // the N1 draws' own stream of the counter-based generator (daco_device.h rng_block)
constexpr uint32_t STREAM_N2 = 6;            // the N2 draws' stream (5 is the sparse sampler's retry)
constexpr int AD_POOL = 5;                   // pool_size of cvrp/aco.py:99
constexpr int AD_TOPK = 5;                   // the literal 5 of cvrp/aco.py:342
constexpr int AD_TRIALS = 5;                 // count = 5 of N1_neighbourhood and of N2_neighbourhood
constexpr int N1_DRAWS = 2, N2_DRAWS = 4;    // uniforms a trial takes: (subroute, node) | (subroute, other subroute, node, position)
constexpr int N1_ROW = N1_DRAWS * AD_TRIALS;             // an instance's noise row: cvrp_n1_kernel's [5][2], and the head of
constexpr int IN_ROW = N1_ROW + N2_DRAWS * AD_TRIALS;    // cvrp_intensify_kernel's [30], N2's [5][4] behind it

// least added length of inserting c into rt[0 .. len-1] (len >= 2): the position i of the gap (rt[i], rt[i+1]) and its delta,
// uniform over the wavefront.  SKIP: the entry at index `skip` is left out (1 <= skip <= len - 2: the route then has len - 1 >= 2
// entries) and the position returned is one of the route without that entry.
template <bool SKIP = false>
__device__ inline KeyIdx best_gap(const float *d, int n, const uint16_t *rt, int len, int c, int lane, int skip = 0) {
  float bk = 0.0f;
  int bi = -1;
  if (SKIP) --len;
  for (int i0 = 0; i0 + 1 < len; i0 += 64) {
    const int i = i0 + lane;
    float k = __builtin_inff();
    int id = 0x7fffffff;
    if (i + 1 < len) {
      const int p1 = rt[SKIP ? i + (i >= skip ? 1 : 0) : i], p2 = rt[SKIP ? i + 1 + (i + 1 >= skip ? 1 : 0) : i + 1];
      const float s = d[(size_t)p1 * n + c] + d[(size_t)c * n + p2];
      k = s - d[(size_t)p1 * n + p2];
      id = i;
    }
    const KeyIdx r = wave_arg<false>(k, id);
    if (bi < 0 || r.key < bk) { bk = r.key; bi = r.idx == 0x7fffffff ? i0 : r.idx; }   // (a chunk of NaN only: its first position)
  }
  return KeyIdx{bk, bi};
}

// first minimum of costs[0 .. A-1] (torch.min(dim=0)), uniform over the wavefront
__device__ inline KeyIdx first_min(const float *costs, int A, int lane) {
  float bk = __builtin_inff();
  int bi = 0x7fffffff;
  for (int a = lane; a < A; a += 64) {
    const float c = costs[a];
    if (c < bk) { bk = c; bi = a; }
  }
  KeyIdx r = wave_arg<false>(bk, bi);
  if (r.idx == 0x7fffffff) r.idx = 0;
  return r;
}

// the route src[0], src[stride], ... (Lmax rows: a column of paths, or a row of shortest) into rt as u16; the row of its last
// customer, -1 if it has none.  rt is written for every lane when this returns.
__device__ inline int load_route(const int64_t *src, long stride, int Lmax, uint16_t *rt, int lane) {
  int last = -1;
  for (int k0 = 0; k0 < Lmax; k0 += 64) {
    const int k = k0 + lane;
    const int v = k < Lmax ? (int)src[(size_t)k * stride] : 0;
    if (k < Lmax) rt[k] = (uint16_t)v;
    const uint64_t nz = __ballot(v != 0);
    if (nz) last = k0 + 63 - __builtin_clzll(nz);
  }
  __builtin_amdgcn_wave_barrier();
  __threadfence_block();
  return last;
}

// rows of a route up to the depot that closes its last subroute (a column whose last row is a customer: that open tail is no
// subroute, :209-217)
__device__ inline int route_end(int last, int Lmax) { return last + 2 <= Lmax ? last + 2 : Lmax; }

// get_subroutes(end_with_zero=True): f(start, j) for every two consecutive depots of rt[0 .. end-1] with a customer between
// them, in route order and uniform over the wavefront.
template <typename Fn>
__device__ inline void for_each_subroute(const uint16_t *rt, int end, int lane, Fn f) {
  int start = -1;
  for (int k0 = 0; k0 < end; k0 += 64) {
    const int k = k0 + lane;
    uint64_t zero = __ballot(k < end && rt[k] == 0);
    while (zero) {
      const int j = k0 + __builtin_ctzll(zero);
      zero &= zero - 1;
      if (start >= 0 && j - start > 1) f(start, j);
      start = j;
    }
  }
}

// ------------------------------------------------------------------ improvement_phase (cvrp/aco.py:336-357)
// One workgroup per instance, NW wavefronts.  Wavefront 0 selects (all ants, or the AD_TOPK cheapest: AD_TOPK rounds of a
// (cost, id) minimum over the ants not yet taken, so equal costs go to the smaller ant id), then wavefront w rebuilds the
// selected ants w, w + NW, ...  LDS per wavefront: out[Lmax] u16, the ant's column, rewritten subroute by subroute | rt[n + 1]
// u16, the subroute under construction.  The column goes back to global memory, with its cost and length, only if accepted.
__global__ void __launch_bounds__(512)
cvrp_reinsert_kernel(int n, int A, int Lmax, int K, const float *dist, long dist_bs, int64_t *paths, float *costs, int32_t *lens,
                     int32_t *selected, int rt_ld) {
  extern __shared__ __attribute__((aligned(16))) uint16_t ad_lds[];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, NW = blockDim.x >> 6;
  const float *d = dist + (size_t)b * dist_bs;
  float *cb = costs + (size_t)b * A;
  int32_t *sel = selected + (size_t)b * K;
  if (wave == 0) {
    if (K == A) {
      for (int a = lane; a < A; a += 64) sel[a] = a;
    } else {
      uint64_t taken_lo = 0;                 // this lane's ants already selected: bit j = ant lane + 64 j, j < 64 (A <= 4096)
      for (int r = 0; r < K; ++r) {
        float bk = __builtin_inff();
        int bi = 0x7fffffff;
        for (int a = lane, j = 0; a < A; a += 64, ++j) {
          if (j < 64 && ((taken_lo >> j) & 1)) continue;
          const float c = cb[a];
          if (c < bk || (c == bk && a < bi) || bi == 0x7fffffff) { bk = c; bi = a; }
        }
        const KeyIdx m = wave_arg<false>(bk, bi);
        if ((m.idx & 63) == lane && m.idx != 0x7fffffff) taken_lo |= 1ull << (m.idx >> 6);
        if (lane == 0) sel[r] = m.idx;
      }
    }
    __threadfence_block();
  }
  __syncthreads();
  uint16_t *out = ad_lds + (size_t)wave * rt_ld;
  uint16_t *rt = out + Lmax;
  for (int r = wave; r < K; r += NW) {
    const int a = sel[r];
    int64_t *p = paths + (size_t)b * Lmax * A + a;
    const int end = route_end(load_route(p, A, Lmax, out, lane), Lmax);
    double total = 0.0;
    int w = 0;                                              // entries of the rebuilt column written so far
    // for_each_subroute's walk, written out: with the rebuild as its functor the compiler keeps the ballot word out of VCC and
    // the insertion scan's selects in it, and the launch measured 1.1 us (1.7 %) slower, outside its windows' spread
    int start = -1;
    for (int k0 = 0; k0 < end; k0 += 64) {
      const int k = k0 + lane;
      uint64_t zero = __ballot(k < end && out[k] == 0);
      while (zero) {
        const int j = k0 + __builtin_ctzll(zero);
        zero &= zero - 1;
        if (start >= 0 && j - start > 1) {
          // rebuild out[start + 1 .. j - 1] from [0, 0], customers in their order in the path
          const int m = min(j - start - 1, n - 1);              // (n - 1 customers at the most: rt holds n + 1 entries)
          if (lane == 0) { rt[0] = 0; rt[1] = 0; }
          __builtin_amdgcn_wave_barrier();
          __threadfence_block();
          double sub = 0.0;
          for (int t = 0; t < m; ++t) {
            const int c = out[start + 1 + t], len = t + 2;
            const KeyIdx g = best_gap(d, n, rt, len, c, lane);
            sub += (double)g.key;
            // rt[g.idx + 1 .. len - 1] move up by one, from the tail, 64 at a time; c takes rt[g.idx + 1]
            for (int hi = len - 1; hi > g.idx; hi -= 64) {
              const int i = hi - lane;
              const int v = i > g.idx ? rt[i] : 0;
              __builtin_amdgcn_wave_barrier();
              if (i > g.idx) rt[i + 1] = (uint16_t)v;
              __builtin_amdgcn_wave_barrier();
              __threadfence_block();
            }
            if (lane == 0) rt[g.idx + 1] = (uint16_t)c;
            __builtin_amdgcn_wave_barrier();
            __threadfence_block();
          }
          total += sub;
          // merge_subroutes (:240-251): the subroute without its closing depot, packed (w <= start: its source is consumed)
          for (int i = lane; i <= m; i += 64) out[w + i] = rt[i];
          w += m + 1;
          __builtin_amdgcn_wave_barrier();
          __threadfence_block();
        }
        start = j;
      }
    }
    // `if new_cost < costs[i]` (:355): torch compares in float32, and stores the float32 rounding
    const float nc = (float)total;
    if (nc < cb[a]) {
      for (int k = lane; k < Lmax; k += 64) p[(size_t)k * A] = k < w ? (int64_t)out[k] : 0;
      if (lane == 0) {
        cb[a] = nc;
        if (lens) lens[(size_t)b * A + a] = w + 1 <= Lmax ? w + 1 : Lmax;
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// ------------------------------------------------------------------ the record and intensification_phase (cvrp/aco.py:81-93, 254-286, 359-376)
// a draw of random.randint(lo, hi) from a uniform u in [0, 1): lo + min(floor(u * (hi - lo + 1)), hi - lo), the product in float32
__device__ inline int draw_int(float u, int lo, int hi) {
  const int span = hi - lo;
  int k = (int)floorf(u * (float)(span + 1));
  k = k < span ? k : span;
  return lo + (k < 0 ? 0 : k);
}

// The record's route tables in LDS, the layout of both intensification kernels: load[n'] DT each subroute's demand (DT: the
// demand's dtype; first, so that a double is aligned) | rt[Lmax'] u16 the record's route | sstart[n'] u16 the row of each
// subroute's opening depot | scnt[n'] u16 its customers | tail: what a kernel keeps behind them, from the next multiple of 8
// bytes.  n', Lmax': rounded up to even.  end: rows of the route with its closing depot; S: subroutes.  The size, for the host
// entries, and the carve, for the kernels, stand side by side:
template <typename DT>
struct RouteTables {
  DT *load;
  uint16_t *rt, *sstart, *scnt;
  void *tail;
  int end, S;
};
__host__ __device__ inline size_t tables_ld(int x) { return (size_t)((x + 1) & ~1); }
__host__ __device__ inline size_t route_tables_bytes(int n, int Lmax, size_t dt) {
  return tables_ld(n) * (dt + 2 * sizeof(uint16_t)) + tables_ld(Lmax) * sizeof(uint16_t);
}
__host__ __device__ inline size_t route_tables_tail(int n, int Lmax, size_t dt) { return (route_tables_bytes(n, Lmax, dt) + 7) & ~(size_t)7; }
template <typename DT>
__device__ inline RouteTables<DT> carve_route_tables(void *lds, int n, int Lmax) {
  RouteTables<DT> T;
  T.load = (DT *)lds;
  T.rt = (uint16_t *)(T.load + tables_ld(n));
  T.sstart = T.rt + tables_ld(Lmax);
  T.scnt = T.sstart + tables_ld(n);
  T.tail = (char *)lds + route_tables_tail(n, Lmax, sizeof(DT));
  T.end = T.S = 0;
  return T;
}

// The record of run() (cvrp/aco.py:81-85, cvrp_nls/aco.py:148-152) for one instance, by one wavefront: the first minimum of its
// costs cb[A]; track: `if best_cost < self.lowest_cost`, the ant's column of pb [Lmax][A] copied into sp [Lmax] and *improved
// written; else *improved read.  low: the record's cost as it stands after that.
struct Record { KeyIdx best; float low; int imp; };
__device__ inline Record take_record(const float *cb, int A, int Lmax, const int64_t *pb, int64_t *sp, const float *lowest,
                                     int32_t *improved, int track, int lane) {
  Record r;
  r.best = first_min(cb, A, lane);
  r.low = *lowest;
  if (track) {
    r.imp = r.best.key < r.low;
    if (r.imp) {
      r.low = r.best.key;
      for (int k = lane; k < Lmax; k += 64) sp[k] = pb[(size_t)k * A + r.best.idx];
    }
    if (lane == 0) *improved = r.imp;
  } else {
    r.imp = *improved != 0;
  }
  return r;
}

// The record's route (load_route's src, stride) laid into T by one wavefront: rt, end, the subroute table and S, the loads.
template <typename DT>
__device__ inline void lay_record(RouteTables<DT> &T, const int64_t *src, long stride, int Lmax, int n, const DT *dem, int lane) {
  T.end = route_end(load_route(src, stride, Lmax, T.rt, lane), Lmax);
  int S = 0;
  for_each_subroute(T.rt, T.end, lane, [&](int start, int j) {
    if (S < n) {                                            // (a route of valid node ids has fewer subroutes than nodes)
      if (lane == 0) { T.sstart[S] = (uint16_t)start; T.scnt[S] = (uint16_t)min(j - start - 1, n - 1); }
      ++S;
    }
  });
  T.S = S;
  __builtin_amdgcn_wave_barrier();
  __threadfence_block();
  for (int s = lane; s < S; s += 64) {                      // self.demand[r].sum() per subroute (:363), sequential in route order
    DT x = (DT)0;
    const int s0 = T.sstart[s], m = T.scnt[s];
    for (int t = 1; t <= m; ++t) x = x + dem[T.rt[s0 + t]];
    T.load[s] = x;
  }
  __builtin_amdgcn_wave_barrier();
  __threadfence_block();
}

// trial t's two uniforms: entries 2t, 2t + 1 of the instance's noise row, else the counter-based stream keyed by (seed, iter, gid, t)
__device__ inline void n1_draws(const float *row, int t, uint64_t seed, uint64_t iter, uint32_t gid, float &u0, float &u1) {
  if (row) {
    u0 = row[N1_DRAWS * t];
    u1 = row[N1_DRAWS * t + 1];
  } else {
    const u32x4 r = rng_block(seed, iter, STREAM_N1, gid, (uint32_t)t);
    u0 = u01(r.x);
    u1 = u01(r.y);
  }
}

// source subroute (-1: none), node index in it, target subroute, index in the target the node goes before
struct N1Move { int src, ni, dst, pos; };

// One trial of N1_neighbourhood (cvrp/aco.py:254-286) against the running best (bdelta, mv), which starts as best_insertion =
// (None, 0.0) and is replaced on strict < only.  T.S > 0.
template <typename DT>
__device__ inline void n1_trial(const RouteTables<DT> &T, const float *d, int n, const DT *dem, DT cap, float u0, float u1, int lane,
                                float &bdelta, N1Move &mv) {
  const int S = T.S;
  const int si = draw_int(u0, 0, S - 1);
  const int s0 = T.sstart[si], m = T.scnt[si];
  const int ni = draw_int(u1, 1, m);
  const int pred = T.rt[s0 + ni - 1], node = T.rt[s0 + ni], next = T.rt[s0 + ni + 1];
  const DT dn = dem[node];
  const float g0 = d[(size_t)pred * n + next] - d[(size_t)pred * n + node];
  const float gain = g0 - d[(size_t)node * n + next];
  for (int i = 0; i < S; ++i) {
    if (i == si || !(T.load[i] + dn <= cap)) continue;
    const KeyIdx g = best_gap(d, n, T.rt + T.sstart[i], (int)T.scnt[i] + 2, node, lane);
    const float cand = g.key + gain;
    if (cand < bdelta) { bdelta = cand; mv = N1Move{si, ni, i, g.idx + 1}; }
  }
}

// N1's move on the packed route: the node at row prm leaves (with its subroute's opening depot if it was alone) and enters
// before the element at row pins; every other element keeps its order.  Written to sp [Lmax] and to the column col (stride A);
// *len, if given, takes the rows of the new route.
template <typename DT>
__device__ inline void apply_n1(const RouteTables<DT> &T, N1Move mv, int Lmax, int64_t *sp, int64_t *col, int A, int32_t *len, int lane) {
  const int s0 = T.sstart[mv.src], vanish = T.scnt[mv.src] == 1, prm = s0 + mv.ni, pins = T.sstart[mv.dst] + mv.pos;
  const int node = T.rt[prm];
  const int used = T.end - vanish;                          // rows of the new route, its closing depot included
  for (int k = lane; k < Lmax; k += 64) {
    if (k >= used) {
      sp[k] = 0;
      col[(size_t)k * A] = 0;
    }
  }
  for (int k = lane; k < T.end; k += 64) {
    if (k == prm || (vanish && k == s0)) continue;
    const int to = k - (k > prm ? 1 : 0) - (vanish && k > s0 ? 1 : 0) + (k >= pins ? 1 : 0);
    sp[to] = T.rt[k];
    col[(size_t)to * A] = T.rt[k];
  }
  if (lane == 0) {
    const int to = pins - (prm < pins ? 1 : 0) - (vanish && s0 < pins ? 1 : 0);
    sp[to] = node;
    col[(size_t)to * A] = node;
    if (len) *len = used;
  }
}

// what both kernels leave of the record: lowest[b] where the instance improved, mmas_max[b] and moved[b] if asked for
__device__ inline void record_tail(const Record &rec, int did, int b, float *lowest, float *mmas_max, float mmas_scale, int32_t *moved,
                                   int lane) {
  if (lane != 0) return;
  if (rec.imp) lowest[b] = rec.low;
  if (mmas_max) mmas_max[b] = (1.0f / rec.low) * mmas_scale;    // n / lowest_cost as rtruediv computes it (daco_track_best)
  if (moved) moved[b] = did;
}

// cvrp/aco.py's intensification: one wavefront per instance takes the record, lays it, runs N1's five trials against one
// running best and applies the move.  LDS: RouteTables<float>, no tail.
__global__ void __launch_bounds__(64)
cvrp_n1_kernel(int n, int A, int Lmax, const float *dist, long dist_bs, const float *demand, float capacity, const float *noise,
               uint64_t seed, uint64_t iter, uint32_t inst_gid0, int64_t *paths, float *costs, int32_t *lens, float *lowest,
               int64_t *shortest, int32_t *improved, int track, float *mmas_max, float mmas_scale, int32_t *moved) {
  extern __shared__ __attribute__((aligned(16))) uint16_t ad_lds[];
  RouteTables<float> T = carve_route_tables<float>(ad_lds, n, Lmax);
  const int b = blockIdx.x, lane = threadIdx.x;
  const float *d = dist + (size_t)b * dist_bs, *dem = demand + (size_t)b * n;
  float *cb = costs + (size_t)b * A;
  int64_t *pb = paths + (size_t)b * Lmax * A, *sp = shortest + (size_t)b * Lmax;
  Record rec = take_record(cb, A, Lmax, pb, sp, lowest + b, improved + b, track, lane);
  int did = 0;
  if (rec.imp) {
    const int bi = rec.best.idx;
    lay_record(T, track ? pb + bi : sp, track ? A : 1, Lmax, n, dem, lane);
    float bdelta = 0.0f;
    N1Move mv{-1, 0, 0, 0};
    for (int t = 0; t < AD_TRIALS && T.S > 0; ++t) {
      float u0, u1;
      n1_draws(noise ? noise + (size_t)b * N1_ROW : nullptr, t, seed, iter, inst_gid0 + (uint32_t)b, u0, u1);
      n1_trial(T, d, n, dem, capacity, u0, u1, lane, bdelta, mv);
    }
    if (mv.src >= 0) {
      did = 1;
      apply_n1(T, mv, Lmax, sp, pb + bi, A, lens ? lens + (size_t)b * A + bi : nullptr, lane);
      rec.low = rec.low + bdelta;                           // self.lowest_cost = ogcost + best_neighbour[1] (:374)
      if (lane == 0) cb[bi] = rec.low;
    }
  }
  record_tail(rec, did, b, lowest, mmas_max, mmas_scale, moved, lane);
}

// ------------------------------------------------------------------ cvrp_nls's intensification_phase (cvrp_nls/aco.py:313-394, 419-434)
// The record, then N1 AND N2 on it, both evaluated on the unmodified record.
constexpr int IN_WAVES = 2 * AD_TRIALS;      // wavefront t < 5: N1's trial t; wavefront 5 + t: N2's trial t
constexpr int IN_RES = 8;                    // ints a trial leaves in LDS: valid | its move
constexpr size_t IN_TAIL_BYTES = 2 * sizeof(int) + IN_WAVES * sizeof(float) + (size_t)IN_WAVES * IN_RES * sizeof(int);

// One workgroup of IN_WAVES wavefronts per instance.  Wavefront 0 takes the record and lays it as cvrp_n1_kernel does; after a
// barrier wavefront w runs its one trial (ten independent chains of gather latencies side by side) and leaves (delta, move) in
// LDS; after a second barrier wavefront 0 takes the first least delta below 0.0 in the order N1's trials, N2's trials (strict <:
// the winner rule of cvrp_nls/aco.py:425-429 and of both neighbourhoods' own loops) and applies it.
// LDS: RouteTables<DT> | tail: hdr[2] int (improved, S) | delta[10] f32 | res[10][IN_RES] int (IN_TAIL_BYTES).  DT is the
// demand's dtype: loads and every capacity test run in it.
template <typename DT>
__global__ void __launch_bounds__(64 * IN_WAVES)
cvrp_intensify_kernel(int n, int A, int Lmax, const float *dist, long dist_bs, const DT *demand, double capacity, const float *noise,
                      uint64_t seed, uint64_t iter, uint32_t inst_gid0, int64_t *paths, float *costs, int32_t *lens, float *lowest,
                      int64_t *shortest, int32_t *improved, int track, float *mmas_max, float mmas_scale, int32_t *moved) {
  extern __shared__ __attribute__((aligned(16))) uint16_t ad_lds[];
  RouteTables<DT> T = carve_route_tables<DT>(ad_lds, n, Lmax);
  int *hdr = (int *)T.tail;
  float *rdelta = (float *)(hdr + 2);
  int *res = (int *)(rdelta + IN_WAVES);
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float *d = dist + (size_t)b * dist_bs;
  const DT *dem = demand + (size_t)b * n;
  const DT cap = (DT)capacity;
  const float *row = noise ? noise + (size_t)b * IN_ROW : nullptr;
  float *cb = costs + (size_t)b * A;
  int64_t *pb = paths + (size_t)b * Lmax * A, *sp = shortest + (size_t)b * Lmax;
  Record rec{KeyIdx{0.0f, 0}, 0.0f, 0};
  if (wave == 0) {
    rec = take_record(cb, A, Lmax, pb, sp, lowest + b, improved + b, track, lane);
    if (rec.imp) lay_record(T, track ? pb + rec.best.idx : sp, track ? A : 1, Lmax, n, dem, lane);
    if (lane == 0) { hdr[0] = rec.imp; hdr[1] = T.S; }
  }
  __syncthreads();
  {
    const uint16_t *rt = T.rt, *sstart = T.sstart, *scnt = T.scnt;
    const DT *load = T.load;
    const int go = hdr[0], S = hdr[1];
    float bdelta = 0.0f;
    int r0 = 0, r1 = 0, r2 = 0, r3 = 0, r4 = 0, r5 = 0, valid = 0;
    if (go && wave < AD_TRIALS && S > 0) {                  // N1_neighbourhood's trial `wave`
      float u0, u1;
      n1_draws(row, wave, seed, iter, inst_gid0 + (uint32_t)b, u0, u1);
      N1Move mv{-1, 0, 0, 0};
      T.S = S;
      n1_trial(T, d, n, dem, cap, u0, u1, lane, bdelta, mv);
      if (mv.src >= 0) { valid = 1; r0 = mv.src; r1 = mv.ni; r2 = mv.dst; r3 = mv.pos; }
    } else if (go && wave >= AD_TRIALS && S >= 2) {         // N2_neighbourhood's trial wave - 5 (S < 2: skipped; the reference raises)
      const int t = wave - AD_TRIALS;
      float u0, u1, u2, u3;
      if (row) {
        const float *q = row + N1_ROW + N2_DRAWS * t;
        u0 = q[0]; u1 = q[1]; u2 = q[2]; u3 = q[3];
      } else {
        const u32x4 r = rng_block(seed, iter, STREAM_N2, inst_gid0 + (uint32_t)b, (uint32_t)t);
        u0 = u01(r.x); u1 = u01(r.y); u2 = u01(r.z); u3 = u01(r.w);
      }
      const int sr1 = draw_int(u0, 0, S - 1);
      int sr2 = draw_int(u1, 0, S - 2);
      if (sr2 >= sr1) ++sr2;
      const int a0 = sstart[sr1], m1 = scnt[sr1], c0 = sstart[sr2], m2 = scnt[sr2];
      const int ni = draw_int(u2, 1, m1);
      const int p1 = rt[a0 + ni - 1], n1 = rt[a0 + ni], x1 = rt[a0 + ni + 1];
      const DT d1 = dem[n1];
      const DT room2 = load[sr2] + d1, room1 = load[sr1] - d1;
      int cnt = 0;
      for (int j0 = 1; j0 <= m2; j0 += 64) {
        const int j = j0 + lane;
        bool ok = false;
        if (j <= m2) { const DT c = dem[rt[c0 + j]]; ok = (room2 - c <= cap) && (room1 + c <= cap); }
        cnt += __popcll(__ballot(ok));
      }
      if (cnt > 0) {
        int k = draw_int(u3, 0, cnt - 1), nj = -1;          // the k-th available position, in increasing order
        for (int j0 = 1; j0 <= m2 && nj < 0; j0 += 64) {
          const int j = j0 + lane;
          bool ok = false;
          if (j <= m2) { const DT c = dem[rt[c0 + j]]; ok = (room2 - c <= cap) && (room1 + c <= cap); }
          const uint64_t mask = __ballot(ok);
          const int pc = __popcll(mask);
          if (k < pc) {
            const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
            nj = j0 + __builtin_ctzll(__ballot(ok && rank == k));
          } else {
            k -= pc;
          }
        }
        const int p2 = rt[c0 + nj - 1], n2 = rt[c0 + nj], x2 = rt[c0 + nj + 1];
        float c = d[(size_t)p1 * n + x1] - d[(size_t)p1 * n + n1];
        c = c - d[(size_t)n1 * n + x1];
        float c2 = d[(size_t)p2 * n + x2] - d[(size_t)p2 * n + n2];
        c2 = c2 - d[(size_t)n2 * n + x2];
        c = c + c2;
        const KeyIdx i1 = best_gap<true>(d, n, rt + c0, m2 + 2, n1, lane, nj);   // node1 into sr2 without node2
        c = c + i1.key;
        const KeyIdx i2 = best_gap<true>(d, n, rt + a0, m1 + 2, n2, lane, ni);   // node2 into sr1 without node1
        c = c + i2.key;
        if (c < bdelta) { bdelta = c; valid = 1; r0 = sr1; r1 = ni; r2 = i2.idx; r3 = sr2; r4 = nj; r5 = i1.idx; }
      }
    }
    if (lane == 0) {
      rdelta[wave] = bdelta;
      int *q = res + wave * IN_RES;
      q[0] = valid; q[1] = r0; q[2] = r1; q[3] = r2; q[4] = r3; q[5] = r4; q[6] = r5;
    }
  }
  __syncthreads();
  if (wave != 0) return;
  int did = 0;
  if (rec.imp) {
    float bdelta = 0.0f;
    int win = -1;
    for (int w = 0; w < IN_WAVES; ++w)
      if (res[w * IN_RES] && rdelta[w] < bdelta) { bdelta = rdelta[w]; win = w; }
    const int bi = rec.best.idx;
    if (win >= 0) {
      const int *q = res + win * IN_RES;
      rec.low = rec.low + bdelta;                           // self.lowest_cost = ogcost + best_neighbour[1] (:432)
      if (win < AD_TRIALS) {
        did = 1;
        apply_n1(T, N1Move{q[1], q[2], q[3], q[4]}, Lmax, sp, pb + bi, A, lens ? lens + (size_t)b * A + bi : nullptr, lane);
      } else {                                              // N2's: both routes keep their rows; each loses one node and takes the other's
        did = 2;
        const uint16_t *rt = T.rt, *sstart = T.sstart, *scnt = T.scnt;
        const int node1 = rt[sstart[q[1]] + q[2]], node2 = rt[sstart[q[4]] + q[5]];
        for (int side = 0; side < 2; ++side) {
          const int s0 = sstart[side ? q[4] : q[1]], m = scnt[side ? q[4] : q[1]], skip = side ? q[5] : q[2], loc = side ? q[6] : q[3];
          const int node = side ? node1 : node2;
          for (int k = lane; k <= m + 1; k += 64) {
            if (k == skip) continue;
            const int i = k - (k > skip ? 1 : 0), to = s0 + i + (i > loc ? 1 : 0);
            sp[to] = rt[s0 + k];
            pb[(size_t)to * A + bi] = rt[s0 + k];
          }
          if (lane == 0) {
            sp[s0 + loc + 1] = node;
            pb[((size_t)s0 + loc + 1) * A + bi] = node;
          }
        }
      }
      if (lane == 0) cb[bi] = rec.low;
    }
  }
  record_tail(rec, did, b, lowest, mmas_max, mmas_scale, moved, lane);
}

// ------------------------------------------------------------------ update_pheronome | diversification_phase, and the pool
// A workgroup owns R rows of one instance's tau.  It reads the routes whose edges are deposited -- the best ant's column for an
// improved instance, the pool's entries from the front for the others --, keeps for each route the successor of each of its
// rows' customers (a customer is left once per route) and, if it owns the depot's row, the SET of the depot's successors as a
// bitmap (so the padding's depot-to-depot edge counts once, like every duplicate of an index pair in the reference's
// `tau[u, v] += w`), and then walks its elements once: x = tau * f (+ 0.01), + w per route that holds the edge, in pool order.
// The workgroup of an improved instance's first slab also pushes (shortest, lowest) to the front of that instance's pool; no
// other workgroup of an improved instance reads the pool.
constexpr int AD_ROWS = 64;
__global__ void __launch_bounds__(256)
cvrp_adaptive_update_kernel(int n, int A, int Lmax, int R, float *tau, const int64_t *paths, const float *costs, const int32_t *improved,
                            float decay, const float *clamp_min, const float *clamp_max, float floor_val, const int64_t *shortest,
                            const float *lowest, int64_t *pool_routes, float *pool_costs, int32_t *pool_state) {
  __shared__ int nxt[AD_POOL][AD_ROWS];
  __shared__ uint32_t hubm[AD_POOL][(DACO_MAX_NODES + 31) / 32];
  __shared__ float wts[AD_POOL];
  __shared__ int best_s;
  const int bpi = (n + R - 1) / R;
  const int b = blockIdx.x / bpi, i0 = (blockIdx.x - b * bpi) * R, Rv = min(R, n - i0);
  const int tid = threadIdx.x, W = (n + 31) / 32;
  const int imp = improved[b] != 0;
  const int count = min(max(pool_state[2 * b], 0), AD_POOL), front = ((pool_state[2 * b + 1] % AD_POOL) + AD_POOL) % AD_POOL;
  const int routes = imp ? 1 : count;
  for (int i = tid; i < AD_POOL * AD_ROWS; i += 256) (&nxt[0][0])[i] = -1;
  for (int i = tid; i < routes * W; i += 256) hubm[i / W][i % W] = 0u;
  if (imp && tid < 64) {
    const KeyIdx m = first_min(costs + (size_t)b * A, A, tid);
    if (tid == 0) { best_s = m.idx; wts[0] = 1.0f / m.key; }
  }
  if (!imp && tid < count) wts[tid] = 1.0f / pool_costs[(size_t)b * AD_POOL + (front + tid) % AD_POOL];
  __syncthreads();
  for (int r = 0; r < routes; ++r) {
    const int64_t *p;
    long stride;
    if (imp) { p = paths + (size_t)b * Lmax * A + best_s; stride = A; }
    else { p = pool_routes + ((size_t)b * AD_POOL + (front + r) % AD_POOL) * Lmax; stride = 1; }
    for (int k = tid; k + 1 < Lmax; k += 256) {
      const int u = (int)p[(size_t)k * stride], v = (int)p[(size_t)(k + 1) * stride];
      if (u == 0) { if (i0 == 0) atomicOr(&hubm[r][v >> 5], 1u << (v & 31)); }
      else if (u >= i0 && u < i0 + Rv) nxt[r][u - i0] = v;
    }
  }
  __syncthreads();
  const bool clamp = imp && clamp_max != nullptr;
  const float cmin = clamp ? clamp_min[b] : 0.0f, cmax = clamp ? clamp_max[b] : 0.0f;
  const float f = imp ? decay : decay * 0.5f;               // (decay * 0.5 rounded once: halving a float32 is exact)
  float *g = tau + ((size_t)b * n + i0) * n;
  for (int e = tid; e < Rv * n; e += 256) {
    const int r_ = e / n, j = e - r_ * n, i = i0 + r_;
    float x = g[e] * f;
    if (!imp) x = x + 0.01f;
    for (int r = 0; r < routes; ++r) {
      const bool hit = i == 0 ? ((hubm[r][j >> 5] >> (j & 31)) & 1u) != 0 : nxt[r][r_] == j;
      if (hit) x = x + wts[r];
    }
    if (imp) {
      if (clamp) { x = x < cmin ? cmin : x; x = x > cmax ? cmax : x; }
      if (floor_val > 0.0f) x = x < floor_val ? floor_val : x;
    }
    g[e] = x;
  }
  if (imp && i0 == 0) {                                     // self.elite_pool.insert(0, ...); del self.elite_pool[5:] (:98-100)
    const int nf = (front + AD_POOL - 1) % AD_POOL;
    int64_t *q = pool_routes + ((size_t)b * AD_POOL + nf) * Lmax;
    for (int k = tid; k < Lmax; k += 256) q[k] = shortest[(size_t)b * Lmax + k];
    if (tid == 0) {
      pool_costs[(size_t)b * AD_POOL + nf] = lowest[b];
      pool_state[2 * b] = count < AD_POOL ? count + 1 : AD_POOL;
      pool_state[2 * b + 1] = nf;
    }
  }
}

}  // namespace daco

using namespace daco;

static bool adaptive_sizes_ok(const char *what, int n, int Lmax) {
  if (n > DACO_MAX_NODES) { set_error("%s: n=%d exceeds DACO_MAX_NODES", what, n); return false; }
  if (Lmax > 4 * DACO_MAX_NODES) { set_error("%s: Lmax=%d exceeds 4 * DACO_MAX_NODES", what, Lmax); return false; }
  return true;
}

extern "C" long daco_cvrp_reinsert(void *stream, int B, int n, int A, int Lmax, int topk, const float *dist, long dist_bstride,
                                   int64_t *paths, float *costs, int32_t *lens, int32_t *selected) {
  if (B <= 0 || n < 2 || A <= 0 || Lmax < 2 || !dist || !paths || !costs || !selected || dist_bstride < 0) {
    set_error("daco_cvrp_reinsert: bad argument (B=%d n=%d A=%d Lmax=%d)", B, n, A, Lmax);
    return DACO_E_BADARG;
  }
  const bool all = topk <= 0 || topk >= A;
  if (!all && A < AD_TOPK) { set_error("daco_cvrp_reinsert: topk=%d selects the %d cheapest of A=%d ants", topk, AD_TOPK, A); return DACO_E_BADARG; }
  if (!adaptive_sizes_ok("daco_cvrp_reinsert", n, Lmax)) return DACO_E_TOOLARGE;
  if (A > 4096) { set_error("daco_cvrp_reinsert: A=%d ants is above 4096", A); return DACO_E_TOOLARGE; }
  const int K = all ? A : AD_TOPK;
  const int rt_ld = (Lmax + n + 1 + 7) & ~7;               // u16 entries per wavefront
  int NW = (int)((64 * 1024) / ((size_t)rt_ld * sizeof(uint16_t)));
  if (NW > 8) NW = 8;
  if (NW > K) NW = K;
  if (NW < 1) NW = 1;
  const size_t lds = (size_t)NW * rt_ld * sizeof(uint16_t);
  hipLaunchKernelGGL(cvrp_reinsert_kernel, dim3(B), dim3(64 * NW), lds, (hipStream_t)stream, n, A, Lmax, K, dist, dist_bstride, paths,
                     costs, lens, selected, rt_ld);
  return launch_status("cvrp_reinsert_kernel");
}

// what daco_cvrp_n1_move and daco_cvrp_intensify (`what`) refuse alike: DACO_OK, or the code with the message set
static long record_args_status(const char *what, int B, int n, int A, int Lmax, long dist_bstride, const void *dist, const void *demand,
                               const void *paths, const void *costs, const void *lowest, const void *shortest, const void *improved) {
  if (B <= 0 || n < 2 || A <= 0 || Lmax < 2 || dist_bstride < 0) {
    set_error("%s: bad argument (B=%d n=%d A=%d Lmax=%d dist_bstride=%ld)", what, B, n, A, Lmax, dist_bstride);
    return DACO_E_BADARG;
  }
  const void *need[] = {dist, demand, paths, costs, lowest, shortest, improved};
  const char *names[] = {"dist", "demand", "paths", "costs", "lowest", "shortest", "improved"};
  for (int i = 0; i < 7; ++i)
    if (!need[i]) { set_error("%s: bad argument: %s is NULL", what, names[i]); return DACO_E_BADARG; }
  return adaptive_sizes_ok(what, n, Lmax) ? DACO_OK : DACO_E_TOOLARGE;
}

/* The record and cvrp/aco.py's intensification_phase, N1, for B instances in one launch.  Its route tables take 2 Lmax + 8 n
 * bytes of LDS, each rounded up to even: 65536 at n = DACO_MAX_NODES, Lmax = 4 DACO_MAX_NODES, so every accepted size fits. */
extern "C" long daco_cvrp_n1_move(void *stream, int B, int n, int A, int Lmax, const float *dist, long dist_bstride, const float *demand,
                                  float capacity, const float *noise, uint64_t seed, uint64_t iter, uint32_t inst_gid0, int64_t *paths,
                                  float *costs, int32_t *lens, float *lowest, int64_t *shortest, int32_t *improved, int track,
                                  float *mmas_max, float mmas_scale, int32_t *moved) {
  const long rc = record_args_status("daco_cvrp_n1_move", B, n, A, Lmax, dist_bstride, dist, demand, paths, costs, lowest, shortest, improved);
  if (rc != DACO_OK) return rc;
  hipLaunchKernelGGL(cvrp_n1_kernel, dim3(B), dim3(64), route_tables_bytes(n, Lmax, sizeof(float)), (hipStream_t)stream, n, A, Lmax, dist,
                     dist_bstride, demand, capacity, noise, seed, iter, inst_gid0, paths, costs, lens, lowest, shortest, improved, track,
                     mmas_max, mmas_scale, moved);
  return launch_status("cvrp_n1_kernel");
}

/* The record and cvrp_nls's intensification_phase, N1 and N2, for B instances in one launch.  Fits (one workgroup's 64 KiB of
 * LDS): 2 Lmax + 8 n + 368 <= 65536 bytes with float32 demands, 2 Lmax + 12 n + 368 with float64 ones -- with Lmax = 2 n + 1
 * every n <= DACO_MAX_NODES for float32 and n <= 4072 for float64; a larger (n, Lmax) is DACO_E_TOOLARGE and is not launched. */
extern "C" long daco_cvrp_intensify(void *stream, int B, int n, int A, int Lmax, const float *dist, long dist_bstride, const void *demand,
                                    int demand_f64, double capacity, const float *noise, uint64_t seed, uint64_t iter, uint32_t inst_gid0,
                                    int64_t *paths, float *costs, int32_t *lens, float *lowest, int64_t *shortest, int32_t *improved,
                                    int track, float *mmas_max, float mmas_scale, int32_t *moved) {
  const long rc = record_args_status("daco_cvrp_intensify", B, n, A, Lmax, dist_bstride, dist, demand, paths, costs, lowest, shortest, improved);
  if (rc != DACO_OK) return rc;
  const size_t lds = route_tables_tail(n, Lmax, demand_f64 ? sizeof(double) : sizeof(float)) + IN_TAIL_BYTES;
  if (lds > 64 * 1024) {
    set_error("daco_cvrp_intensify: n=%d, Lmax=%d with %s demands take %zu bytes of LDS, above 65536", n, Lmax,
              demand_f64 ? "float64" : "float32", lds);
    return DACO_E_TOOLARGE;
  }
  if (demand_f64)
    hipLaunchKernelGGL(cvrp_intensify_kernel<double>, dim3(B), dim3(64 * IN_WAVES), lds, (hipStream_t)stream, n, A, Lmax, dist, dist_bstride,
                       (const double *)demand, capacity, noise, seed, iter, inst_gid0, paths, costs, lens, lowest, shortest, improved, track,
                       mmas_max, mmas_scale, moved);
  else
    hipLaunchKernelGGL(cvrp_intensify_kernel<float>, dim3(B), dim3(64 * IN_WAVES), lds, (hipStream_t)stream, n, A, Lmax, dist, dist_bstride,
                       (const float *)demand, capacity, noise, seed, iter, inst_gid0, paths, costs, lens, lowest, shortest, improved, track,
                       mmas_max, mmas_scale, moved);
  return launch_status("cvrp_intensify_kernel");
}

extern "C" long daco_cvrp_adaptive_update(void *stream, int B, int n, int A, int Lmax, float *tau, const int64_t *paths, const float *costs,
                                          const int32_t *improved, float decay, const float *clamp_min, const float *clamp_max,
                                          float floor_val, const int64_t *shortest, const float *lowest, int64_t *pool_routes,
                                          float *pool_costs, int32_t *pool_state) {
  if (B <= 0 || n < 2 || A <= 0 || Lmax < 2 || !tau || !paths || !costs || !improved || !shortest || !lowest || !pool_routes || !pool_costs ||
      !pool_state) {
    set_error("daco_cvrp_adaptive_update: bad argument (B=%d n=%d A=%d Lmax=%d)", B, n, A, Lmax);
    return DACO_E_BADARG;
  }
  if ((clamp_min == nullptr) != (clamp_max == nullptr)) { set_error("daco_cvrp_adaptive_update: clamp_min/clamp_max must both be given"); return DACO_E_BADARG; }
  if (!adaptive_sizes_ok("daco_cvrp_adaptive_update", n, Lmax)) return DACO_E_TOOLARGE;
  // rows per workgroup: as many as keep two workgroups per CU in the launch (daco_costs_update.hip rows_per_block), 64 at the most
  int R = AD_ROWS;
  while (R > 1 && (long)B * ((n + R - 1) / R) < 512) R = (R + 1) / 2;
  const int bpi = (n + R - 1) / R;
  hipLaunchKernelGGL(cvrp_adaptive_update_kernel, dim3(B * bpi), dim3(256), 0, (hipStream_t)stream, n, A, Lmax, R, tau, paths, costs, improved,
                     decay, clamp_min, clamp_max, floor_val, shortest, lowest, pool_routes, pool_costs, pool_state);
  return launch_status("cvrp_adaptive_update_kernel");
}
