// daco_sib_objective.hip -- objective, elitist key, deposit amount and best-so-far record of the six sibling problems.
//
// Reference behaviour replaced (per iteration of ACO.run, for B instances at once and without a host branch):
//   smtwtp/aco.py:84-111 gen_path_costs + 1/(cost+1)     sop/aco.py gen_path_costs + 1/cost
//   pctsp/aco.py:104-129 gen_sol_obj + 1/obj             op/aco.py:141-147 gen_sol_obj + Q*obj
//   mkp/aco.py gen_sol_obj + Q*obj                        bpp/aco.py:26-40,121-126 cal_fitness + fit/n_ants
// and the `if best ... self.<record>` step of the six run() loops (include/deepaco_hip.h states the arithmetic).
//
// Mapping: the solutions are [B][rows][A], ants innermost, so ONE LANE PER ANT walks k upward: every row is one coalesced
// load per wavefront and the documented sequential order of every sum is the lane's own program order.  A workgroup is one
// wavefront (64 ants of one instance); the instance's vectors (at most three of n floats: SMTWTP) live in LDS, and so does
// PCTSP's "seen" set, one bitset of n bits per lane with the words lane-interleaved (word w of lane l at [w * 64 + l]: the 64
// lanes of an access hit 64 consecutive dwords, no bank is shared).  LDS at n = DACO_MAX_NODES: 48 KiB (SMTWTP 3 x 16 KiB,
// PCTSP 16 KiB + 64 x 512 B), below the 64 KiB a workgroup may have, so no size is refused below DACO_MAX_NODES.
// The rows of eight steps are fetched before the first of them is added: the adds stay in order, the loads do not wait for
// each other.  No atomics.
#include "daco_host.h"

#pragma clang fp contract(off)

namespace daco {

constexpr int OBJ_T = 64;      // lanes (ants) per workgroup
constexpr int OBJ_U = 8;       // rows fetched ahead

struct ObjParams {
  int kind, n, rows, A, elitist;
  const int64_t *paths;
  const int32_t *lens;
  const float *vec0, *vec1, *vec2, *mat, *scale;
  long mat_bs;
  double capacity;
  float *obj, *key, *weight;
  double *obj64;
};

__global__ void __launch_bounds__(OBJ_T)
sibling_objective_kernel(const ObjParams q) {
  extern __shared__ __attribute__((aligned(16))) float obj_lds[];
  const int n = q.n, rows = q.rows, A = q.A;
  const int per = (A + OBJ_T - 1) / OBJ_T;
  const int b = blockIdx.x / per, a = (blockIdx.x - b * per) * OBJ_T + threadIdx.x;
  const int lane = threadIdx.x;
  // ---- the instance's vectors -> LDS
  const int nv = q.kind == DACO_SIB_SMTWTP ? 3 : (q.kind == DACO_SIB_SOP ? 0 : 1);
  float *v0 = obj_lds, *v1 = obj_lds + n, *v2 = obj_lds + 2 * n;
  uint32_t *seen = (uint32_t *)(obj_lds + (size_t)nv * n);
  const int W = (n + 31) >> 5;
  for (int i = lane; i < n; i += OBJ_T) {
    if (nv >= 1) v0[i] = q.vec0[(size_t)b * n + i];
    if (nv == 3) { v1[i] = q.vec1[(size_t)b * n + i]; v2[i] = q.vec2[(size_t)b * n + i]; }
  }
  if (q.kind == DACO_SIB_PCTSP)
    for (int w = 0; w < W; ++w) seen[w * OBJ_T + lane] = 0u;
  // BPP: L = the longest route of the instance (the width of the reference's padded matrix)
  int L = rows;
  if (q.kind == DACO_SIB_BPP && q.lens) {
    int mx = 0;
    for (int i = lane; i < A; i += OBJ_T) mx = max(mx, q.lens[(size_t)b * A + i]);
#pragma unroll
    for (int off = 32; off; off >>= 1) mx = max(mx, __shfl_xor(mx, off, 64));
    L = min(mx, rows);
  }
  __syncthreads();
  if (a >= A) return;
  const size_t ia = (size_t)b * A + a;
  const int64_t *p = q.paths + (size_t)b * rows * A + a;
  int len = q.lens ? q.lens[ia] : rows;
  len = len < 0 ? 0 : (len > rows ? rows : len);
  // a node outside the instance (SMTWTP: n jobs and the dummy, n + 1 nodes) reads as node 0: nothing below indexes past its data
  const int nn = q.kind == DACO_SIB_SMTWTP ? n + 1 : n;
  auto node_at = [&](int k) { const long u = (long)p[(size_t)k * A]; return (u < 0 || u >= nn) ? 0 : (int)u; };

  if (q.kind == DACO_SIB_BPP) {
    const double C = q.capacity;
    double f = 0.0, sub = 0.0;
    int last_nz = -1;
    for (int k0 = 0; k0 < len; k0 += OBJ_U) {
      int u[OBJ_U];
#pragma unroll
      for (int j = 0; j < OBJ_U; ++j) u[j] = k0 + j < len ? node_at(k0 + j) : 0;
#pragma unroll
      for (int j = 0; j < OBJ_U; ++j) {
        const int k = k0 + j;
        if (k >= len) break;
        if (u[j] != 0) last_nz = k;
        if (k == 0) continue;
        if (u[j] != 0) sub = sub + (double)v0[u[j]];
        else { const double r = sub / C; f = f + r * r; sub = 0.0; }
      }
    }
    if (len < L) { const double r = sub / C; f = f + r * r; }      // the first padding row closes an open bin
    const int tz = last_nz < 0 ? 0 : L - 1 - last_nz;              // (count_last_zero leaves 0 for a row of zeros)
    const int n_bins = L - tz - n + 1;
    const double cost = -(f / (double)n_bins);
    const double fit = -cost;
    q.obj64[ia] = cost;
    q.key[ia] = (float)cost;
    q.weight[ia] = q.elitist ? (float)fit : (float)(fit / (double)A);
    return;
  }

  float c = 0.0f;
  if (q.kind == DACO_SIB_SMTWTP) {
    float t = 0.0f;
    for (int k0 = 1; k0 < len; k0 += OBJ_U) {
      int u[OBJ_U];
#pragma unroll
      for (int j = 0; j < OBJ_U; ++j) u[j] = k0 + j < len ? node_at(k0 + j) : 1;
#pragma unroll
      for (int j = 0; j < OBJ_U; ++j) {
        if (k0 + j >= len) break;
        const int job = u[j] >= 1 ? u[j] - 1 : 0;
        t = t + v0[job];
        const float d = t - v1[job];
        const float late = d < 0.0f ? 0.0f : d;
        c = c + v2[job] * late;
      }
    }
    q.obj[ia] = c;
    q.key[ia] = c;
    q.weight[ia] = 1.0f / (c + 1.0f);
    return;
  }
  if (q.kind == DACO_SIB_OP || q.kind == DACO_SIB_MKP) {
    for (int k0 = 0; k0 < len; k0 += OBJ_U) {
      int u[OBJ_U];
#pragma unroll
      for (int j = 0; j < OBJ_U; ++j) u[j] = k0 + j < len ? node_at(k0 + j) : 0;
#pragma unroll
      for (int j = 0; j < OBJ_U; ++j) {
        if (k0 + j >= len) break;
        c = c + v0[u[j]];
      }
    }
    q.obj[ia] = c;
    q.key[ia] = -c;
    q.weight[ia] = q.scale[b] * c;
    return;
  }
  // SOP / PCTSP: the open length sum_k d[u_k][u_{k+1}], k ascending (daco_tour_costs(closed = 0))
  const float *d = q.mat + (size_t)b * q.mat_bs;
  const bool pc = q.kind == DACO_SIB_PCTSP;
  if (len > 0) {
    int prev = node_at(0);
    if (pc) seen[(prev >> 5) * OBJ_T + lane] |= 1u << (prev & 31);
    for (int k0 = 1; k0 < len; k0 += OBJ_U) {
      int u[OBJ_U];
      float e[OBJ_U];
#pragma unroll
      for (int j = 0; j < OBJ_U; ++j) u[j] = k0 + j < len ? node_at(k0 + j) : 0;
#pragma unroll
      for (int j = 0; j < OBJ_U; ++j) e[j] = k0 + j < len ? d[(size_t)(j ? u[j - 1] : prev) * n + u[j]] : 0.0f;
#pragma unroll
      for (int j = 0; j < OBJ_U; ++j) {
        if (k0 + j >= len) break;
        c = c + e[j];
        if (pc) seen[(u[j] >> 5) * OBJ_T + lane] |= 1u << (u[j] & 31);
        prev = u[j];
      }
    }
  }
  if (!pc) {
    q.obj[ia] = c;
    q.key[ia] = c;
    q.weight[ia] = 1.0f / c;
    return;
  }
  float pen = 0.0f;
  for (int w = 0; w < W; ++w) {
    uint32_t out = ~seen[w * OBJ_T + lane];
    if (w == W - 1 && (n & 31)) out &= (1u << (n & 31)) - 1u;
    while (out) {                                   // node index ascending
      const int bit = __ffs((int)out) - 1;
      out &= out - 1u;
      pen = pen + v0[w * 32 + bit];
    }
  }
  const float o = c + pen;
  q.obj[ia] = o;
  q.key[ia] = -o;
  q.weight[ia] = 1.0f / o;
}

// the record step of the six run() loops: first minimum of the key; the rule compares that ant's objective with the record
__global__ void __launch_bounds__(256)
sibling_record_kernel(int rule, int len, int A, const float *key, const float *obj, const double *obj64, const int64_t *paths,
                      int row0, float *best_obj, double *best_obj64, int64_t *best_sol, int32_t *best_idx, float *mmas_max,
                      float mmas_n, const float *mmas_scale) {
  __shared__ float rk[4];
  __shared__ int ri[4];
  __shared__ int take;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float bk = __builtin_inff();
  int bi = 0x7fffffff;
  for (int a = tid; a < A; a += 256) {
    const float c = key[(size_t)b * A + a];
    if (c < bk) { bk = c; bi = a; }
  }
  const KeyIdx r = wave_arg<false>(bk, bi);
  if (lane == 0) { rk[wave] = r.key; ri[wave] = r.idx; }
  __syncthreads();
  if (tid == 0) {
    float k = rk[0];
    int i = ri[0];
    for (int w = 1; w < 4; ++w)
      if (rk[w] < k || (rk[w] == k && ri[w] < i)) { k = rk[w]; i = ri[w]; }
    if (i == 0x7fffffff) i = 0;
    if (best_idx) best_idx[b] = i;
    bool improved;
    if (rule == DACO_SIB_BPP) {
      const double fit = -obj64[(size_t)b * A + i];
      improved = fit > best_obj64[b];
      if (improved) best_obj64[b] = fit;
    } else {
      const float o = obj[(size_t)b * A + i];
      float rec = best_obj[b];
      improved = (rule == DACO_SIB_OP || rule == DACO_SIB_MKP) ? o > rec : o < rec;
      if (improved) { rec = o; best_obj[b] = o; }
      if (mmas_max) {
        if (rule == DACO_SIB_SOP) mmas_max[b] = (1.0f / rec) * mmas_n;
        else if (rule == DACO_SIB_PCTSP) mmas_max[b] = mmas_n / rec;
        else if (rule == DACO_SIB_OP) mmas_max[b] = (rec * mmas_n) * mmas_scale[b];
      }
    }
    take = improved ? i : -1;
  }
  __syncthreads();
  const int t = take;
  if (t >= 0 && best_sol) {
    const int out = len - row0;
    for (int k = tid; k < out; k += 256) best_sol[(size_t)b * out + k] = paths[((size_t)b * len + row0 + k) * A + t];
  }
}

}  // namespace daco

using namespace daco;

static bool sib_kind_ok(int kind) {
  return kind >= DACO_SIB_SOP && kind <= DACO_SIB_BPP;      // 3..8: the six constants are consecutive
}

extern "C" long daco_sibling_objective(void *stream, int kind, int B, int n, int rows, int A, const int64_t *paths,
                                      const int32_t *lens, const float *vec0, const float *vec1, const float *vec2,
                                      const float *mat, long mat_bstride, double capacity, int elitist, const float *scale,
                                      float *obj, double *obj64, float *key, float *weight) {
  if (!sib_kind_ok(kind)) { set_error("daco_sibling_objective: unknown kind %d", kind); return DACO_E_BADARG; }
  if (B <= 0 || n < 1 || rows < 1 || A <= 0 || !paths || !key || !weight) {
    set_error("daco_sibling_objective: bad argument (B=%d n=%d rows=%d A=%d)", B, n, rows, A);
    return DACO_E_BADARG;
  }
  if (n > DACO_MAX_NODES) { set_error("daco_sibling_objective: n=%d exceeds DACO_MAX_NODES=%d", n, DACO_MAX_NODES); return DACO_E_TOOLARGE; }
  if (kind == DACO_SIB_BPP ? !obj64 : !obj) { set_error("daco_sibling_objective: kind %d needs %s", kind, kind == DACO_SIB_BPP ? "obj64" : "obj"); return DACO_E_BADARG; }
  if (kind == DACO_SIB_SMTWTP && (!vec0 || !vec1 || !vec2 || rows != n + 1)) { set_error("daco_sibling_objective: SMTWTP needs vec0 (processing), vec1 (due), vec2 (weights) and rows = n + 1"); return DACO_E_BADARG; }
  if ((kind == DACO_SIB_SOP || kind == DACO_SIB_PCTSP) && !mat) { set_error("daco_sibling_objective: kind %d needs the distances in mat", kind); return DACO_E_BADARG; }
  if ((kind == DACO_SIB_PCTSP || kind == DACO_SIB_OP || kind == DACO_SIB_MKP || kind == DACO_SIB_BPP) && !vec0) { set_error("daco_sibling_objective: kind %d needs vec0 (penalties / prizes / demand)", kind); return DACO_E_BADARG; }
  if ((kind == DACO_SIB_OP || kind == DACO_SIB_MKP) && !scale) { set_error("daco_sibling_objective: kind %d needs scale [B]", kind); return DACO_E_BADARG; }
  if (kind == DACO_SIB_BPP && !(capacity > 0.0)) { set_error("daco_sibling_objective: BPP needs capacity > 0"); return DACO_E_BADARG; }
  ObjParams q;
  q.kind = kind; q.n = n; q.rows = rows; q.A = A; q.elitist = elitist ? 1 : 0;
  q.paths = paths; q.lens = lens; q.vec0 = vec0; q.vec1 = vec1; q.vec2 = vec2; q.mat = mat; q.scale = scale;
  q.mat_bs = mat_bstride; q.capacity = capacity; q.obj = obj; q.key = key; q.weight = weight; q.obj64 = obj64;
  const int nv = kind == DACO_SIB_SMTWTP ? 3 : (kind == DACO_SIB_SOP ? 0 : 1);
  size_t lds = (size_t)nv * n * sizeof(float);
  if (kind == DACO_SIB_PCTSP) lds += (size_t)((n + 31) / 32) * OBJ_T * sizeof(uint32_t);
  const int per = (A + OBJ_T - 1) / OBJ_T;
  hipLaunchKernelGGL(sibling_objective_kernel, dim3((unsigned)(B * per)), dim3(OBJ_T), lds, (hipStream_t)stream, q);
  return launch_status("sibling_objective_kernel");
}

extern "C" long daco_sibling_record(void *stream, int rule, int B, int len, int A, const float *key, const float *obj,
                                   const double *obj64, const int64_t *paths, int row0, float *best_obj, double *best_obj64,
                                   int64_t *best_sol, int32_t *best_idx, float *mmas_max, float mmas_n, const float *mmas_scale) {
  if (!sib_kind_ok(rule)) { set_error("daco_sibling_record: unknown rule %d", rule); return DACO_E_BADARG; }
  if (B <= 0 || len < 1 || A <= 0 || row0 < 0 || row0 >= len || !key || (best_sol && !paths)) {
    set_error("daco_sibling_record: bad argument (B=%d len=%d A=%d row0=%d)", B, len, A, row0);
    return DACO_E_BADARG;
  }
  if (rule == DACO_SIB_BPP ? (!obj64 || !best_obj64) : (!obj || !best_obj)) { set_error("daco_sibling_record: rule %d needs its objective and record arrays", rule); return DACO_E_BADARG; }
  if (mmas_max && rule == DACO_SIB_OP && !mmas_scale) { set_error("daco_sibling_record: OP's mmas_max needs mmas_scale [B]"); return DACO_E_BADARG; }
  hipLaunchKernelGGL(sibling_record_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, rule, len, A, key, obj, obj64, paths, row0,
                     best_obj, best_obj64, best_sol, best_idx, mmas_max, mmas_n, mmas_scale);
  return launch_status("sibling_record_kernel");
}
