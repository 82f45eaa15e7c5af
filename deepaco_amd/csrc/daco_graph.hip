// daco_graph.hip -- batched instance -> graph construction for the TSP family.
//
// Reference behaviour replaced: gen_distance_matrix + gen_pyg_data, tsp/utils.py:4-36 and
// tsp_nls/utils.py:5-45 (one instance at a time: norm of coordinate differences, diagonal 1e9,
// torch.topk(k, largest=False) per row, edge_index = [repeat_interleave(arange n, k); topk indices],
// edge_attr = topk values).  This is the step immediately before Net.forward; here it
// is one launch for B instances: one wavefront per node builds its distance row (kept in registers,
// lane l owns columns l, l+64, ...) and extracts the k nearest by k rounds of a wave arg-min
// (ties -> smaller index).  Output order = ascending distance, like topk's sorted result.
#include "daco_host.h"

namespace daco {

template <int CPL>   // columns per lane
__global__ void __launch_bounds__(256)
knn_graph_kernel(int B, int n, int k, const float *coords, float diag, float *dist, int64_t *edge_src,
                 int64_t *edge_dst, float *edge_attr, int32_t *src32, int32_t *dst32) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * 4 + wave;          // b*n + i
  if (row >= (long)B * n) return;
  const int b = (int)(row / n), i = (int)(row % n);
  const float *c = coords + (size_t)b * n * 2;
  const float xi = c[2 * i], yi = c[2 * i + 1];
  float dv[CPL];
  // (the row's coordinates first, all of them, unconditionally -- a lane past the row reads node 0 and drops it: read under
  // `if (j < n)` next to the store of the distance, every chunk's pair was a memory round trip of its own)
  float2 cjv[CPL];
#pragma unroll
  for (int q = 0; q < CPL; ++q) { const int j = lane + 64 * q; cjv[q] = *reinterpret_cast<const float2 *>(c + 2 * (j < n ? j : 0)); }
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
    const int j = lane + 64 * q;
    const float2 cj = cjv[q];
    float v = __builtin_inff();
    if (j < n) {
      const float dx = xi - cj.x, dy = yi - cj.y;
      v = j == i ? diag : sqrtf(dx * dx + dy * dy);
      if (dist) dist[(size_t)row * n + j] = v;
    }
    dv[q] = v;
  }
  // round r's winner is kept by lane r % 64; every 64 rounds (and at the end) the lanes store their edges side by side
  float rkey = 0.0f;
  int ridx = 0;
  for (int r = 0; r < k; ++r) {
    float bk = __builtin_inff();
    int bj = 0x7fffffff;
#pragma unroll
    for (int q = 0; q < CPL; ++q)
      if (dv[q] < bk) { bk = dv[q]; bj = lane + 64 * q; }
    const KeyIdx w = wave_arg<false>(bk, bj);
#pragma unroll
    for (int q = 0; q < CPL; ++q)
      if (lane + 64 * q == w.idx) dv[q] = __builtin_inff();          // taken
    if (lane == (r & 63)) { rkey = w.key; ridx = w.idx; }
    if ((r & 63) == 63 || r == k - 1) {
      const int r0 = r & ~63;
      if (lane <= r - r0) {
        const size_t e = (size_t)row * k + r0 + lane;
        edge_src[e] = i;
        edge_dst[e] = ridx;
        edge_attr[e] = rkey;
        if (src32) { src32[e] = b * n + i; dst32[e] = b * n + ridx; }
      }
    }
  }
}

// ---- the CVRP graph of cvrp_nls/utils.py:34-59 (gen_pyg_data) for B instances of n1 = n + 1 nodes (node 0 = the depot), from the
// distance matrix the caller holds (float64 in cvrp_nls, float32 instantiated too): one wavefront per customer row i = 1 .. n
// takes the k smallest of dist[i][1:] (the row in registers, lane l owns customer columns l, l + 64, ...; k rounds of a wave
// arg-min in the matrix's own precision, ascending, ties -> smaller column; the diagonal's 1e-10 makes the customer its own
// first neighbour, as torch.topk does in the reference: the self loop is kept).  Per instance E = n (k + 2) edges in the
// reference's order -- (i-1) k + r the k-NN part, n k + (i-1) depot -> i, n k + n + (i-1) i -> depot, both depot blocks with
// dist[i][0] -- as int64 graph-local ids and float32 attributes, and the whole batch as one merged int32 graph with its CSR by
// source: the depot has n out-edges and customer i has k + 1, so
//   rowptr[b n1] = b E,  rowptr[b n1 + i] = b E + n + (i-1)(k+1),  rowptr[B n1] = B E
//   perm[b E + (i-1)] = b E + n k + (i-1)                         (the depot's row: its edges in original order)
//   perm[b E + n + (i-1)(k+1) + r] = b E + (i-1) k + r, r < k;   ... + k] = b E + n k + n + (i-1)
// which is the stable argsort by source of the merged edge list (what Net's _csr_graph derives with a sort and a host read).
template <typename T> struct CvrpKey { T key; int idx; };

template <typename T, int CTRL, int ROW_MASK>
__device__ inline void cvrp_arg_step(T &k, int &i) {
  T ok;
  if constexpr (sizeof(T) == 4) {
    ok = dpp_f<CTRL, ROW_MASK, false>(k, k);
  } else {
    const long long bits = __double_as_longlong(k);
    const int lo = (int)(bits & 0xffffffffLL), hi = (int)(bits >> 32);
    const int olo = dpp_i<CTRL, ROW_MASK, false>(lo, lo), ohi = dpp_i<CTRL, ROW_MASK, false>(hi, hi);
    ok = __longlong_as_double(((long long)ohi << 32) | (long long)(unsigned)olo);
  }
  const int oi = dpp_i<CTRL, ROW_MASK, false>(i, i);
  if (ok < k || (ok == k && oi < i)) { k = ok; i = oi; }
}
// (key, idx) arg-min over the wave along wave_arg's network, in T
template <typename T>
__device__ inline CvrpKey<T> cvrp_wave_argmin(T k, int i) {
  cvrp_arg_step<T, DPP_ROW_SHR(1), 0xF>(k, i);
  cvrp_arg_step<T, DPP_ROW_SHR(2), 0xF>(k, i);
  cvrp_arg_step<T, DPP_ROW_SHR(4), 0xF>(k, i);
  cvrp_arg_step<T, DPP_ROW_SHR(8), 0xF>(k, i);
  cvrp_arg_step<T, DPP_ROW_BCAST15, 0xA>(k, i);
  cvrp_arg_step<T, DPP_ROW_BCAST31, 0xC>(k, i);
  CvrpKey<T> w;
  w.idx = readlane_i(i, 63);
  if constexpr (sizeof(T) == 4) {
    w.key = readlane_f(k, 63);
  } else {
    const long long bits = __double_as_longlong(k);
    const int lo = readlane_i((int)(bits & 0xffffffffLL), 63), hi = readlane_i((int)(bits >> 32), 63);
    w.key = __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
  }
  return w;
}

template <typename T, int CPL>   // customer columns per lane
__global__ void __launch_bounds__(256)
cvrp_knn_graph_kernel(int B, int n, int k, const T *dist, long dist_bs, int64_t *edge_index, float *edge_attr, int32_t *src32,
                      int32_t *dst32, int32_t *rowptr, int32_t *perm) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * 4 + wave;          // b*n + (i-1)
  if (row >= (long)B * n) return;
  const int b = (int)(row / n), c0 = (int)(row % n), i = c0 + 1;
  const int n1 = n + 1, E = n * (k + 2);
  const T *drow = dist + (size_t)b * dist_bs + (size_t)i * n1;
  const T inf = (T)__builtin_inff();
  T dv[CPL];
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
    const int c = lane + 64 * q;                          // customer column c is node c + 1
    dv[q] = c < n ? drow[1 + c] : inf;
  }
  int64_t *esrc = edge_index + (size_t)b * 2 * E, *edst = esrc + E;
  float *attr = edge_attr + (size_t)b * E;
  const int eb = b * E, nb = b * n1;                      // (B E and B n1 fit 32 bits: checked on the host)
  if (lane == 0) {
    const float d0 = (float)drow[0];
    const int e1 = n * k + c0, e2 = e1 + n;
    esrc[e1] = 0; edst[e1] = i; attr[e1] = d0;
    esrc[e2] = i; edst[e2] = 0; attr[e2] = d0;
    src32[eb + e1] = nb; dst32[eb + e1] = nb + i;
    src32[eb + e2] = nb + i; dst32[eb + e2] = nb;
    perm[eb + c0] = eb + e1;
    perm[eb + n + c0 * (k + 1) + k] = eb + e2;
    rowptr[nb + i] = eb + n + c0 * (k + 1);
    if (c0 == 0) rowptr[nb] = eb;
    if (row == (long)B * n - 1) rowptr[nb + n1] = eb + E;
  }
  // round r's winner is kept by lane r % 64; every 64 rounds (and at the end) the lanes store their edges side by side
  T rkey = (T)0;
  int ridx = 0;
  for (int r = 0; r < k; ++r) {
    T bk = inf;
    int bj = 0x7fffffff;
#pragma unroll
    for (int q = 0; q < CPL; ++q)
      if (dv[q] < bk) { bk = dv[q]; bj = lane + 64 * q; }
    const CvrpKey<T> w = cvrp_wave_argmin<T>(bk, bj);
#pragma unroll
    for (int q = 0; q < CPL; ++q)
      if (lane + 64 * q == w.idx) dv[q] = inf;            // taken
    if (lane == (r & 63)) { rkey = w.key; ridx = w.idx < n ? w.idx : n - 1; }   // (a row of NaN / inf has no winner: the id stays a node's)
    if ((r & 63) == 63 || r == k - 1) {
      const int r0 = r & ~63;
      if (lane <= r - r0) {
        const int e = c0 * k + r0 + lane;
        esrc[e] = i;
        edst[e] = ridx + 1;
        attr[e] = (float)rkey;
        src32[eb + e] = nb + i;
        dst32[eb + e] = nb + ridx + 1;
        perm[eb + n + c0 * (k + 1) + r0 + lane] = eb + e;
      }
    }
  }
}

// ---- Net.reshape for a batch (tsp/net.py:94-102) with the "+ eps" of its callers (tsp/train.ipynb:35, tsp_nls/test.py:28):
// out[b] = fill everywhere, heu[b][e] + add at [src_e][dst_e].  Two launches on one stream: the fill, then one thread per edge.
__global__ void __launch_bounds__(256)
heu_fill_kernel(size_t total, float fill, float *out) {
  const size_t quads = total / 4;
  const float4 v = make_float4(fill, fill, fill, fill);
  float4 *out4 = reinterpret_cast<float4 *>(out);
  for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (size_t)gridDim.x * 256) out4[q] = v;
  if (blockIdx.x == 0 && quads * 4 + threadIdx.x < total) out[quads * 4 + threadIdx.x] = fill;     // (past the last whole float4)
}
__global__ void __launch_bounds__(256)
heu_scatter_kernel(int B, int n, int E, const int64_t *edge_index, const float *heu, float add, float *out, int32_t *bad) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)B * E) return;
  const int b = (int)(idx / E), e = (int)(idx - (size_t)b * E);
  const int64_t sidx = edge_index[((size_t)b * 2) * E + e], didx = edge_index[((size_t)b * 2 + 1) * E + e];
  if (sidx < 0 || sidx >= n || didx < 0 || didx >= n) { if (bad) atomicAdd(bad, 1); return; }
  out[((size_t)b * n + (size_t)sidx) * n + (size_t)didx] = heu[idx] + add;
}

// ---- sop/: the network's graph is nonzero(adj) (sop/utils.py:52-57), adj[u][v] = 1 unless u == v or prec[u][v] = 1 -- its
// size depends on the data.  B instances as one block-diagonal graph in exactly torch.nonzero's order (instance after instance,
// source-major, destinations ascending): a count pass (one wavefront per row (b, u), a ballot per 64 columns), a scan of the row
// counts on the device, and a fill pass that compacts every row with the same ballots -- a lane's slot is the row's base + the
// kept columns before it (mbcnt): no sort, no atomics on the output.
__device__ inline bool sop_edge(const float *prow, int n, int u, int v) { return v < n && v != u && prow[v] == 0.0f; }

__global__ void __launch_bounds__(256)
sop_graph_count_kernel(int rows, int n, const float *prec, int32_t *cnt) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int u = row % n;
  const float *prow = prec + (size_t)row * n;
  int total = 0;
  for (int v0 = 0; v0 < n; v0 += 64) total += __popcll(__ballot(sop_edge(prow, n, u, v0 + lane)));
  if (lane == 0) cnt[row] = total;
}

// rowptr[0 .. rows) holds the row counts on entry and their exclusive sums on return, rowptr[rows] = E; edge_off[b] =
// rowptr[b n].  One workgroup: rows = B n is a few thousand.
__global__ void __launch_bounds__(1024)
sop_graph_scan_kernel(int rows, int n, int32_t *rowptr, int32_t *edge_off) {
  __shared__ int wsum[16], carry_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < rows; base += 1024) {
    const int i = base + tid;
    const int v = i < rows ? rowptr[i] : 0;
    int inc = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) { const int o = __shfl_up(inc, s, 64); if (lane >= s) inc += o; }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int off = carry_s;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    if (i < rows) {
      rowptr[i] = off + inc - v;
      if (i % n == 0) edge_off[i / n] = off + inc - v;
    }
    __syncthreads();
    if (tid == 1023) carry_s = off + inc;
    __syncthreads();
  }
  if (tid == 0) { rowptr[rows] = carry_s; edge_off[rows / n] = carry_s; }
}

// E: the size of the caller's outputs.  A call whose E is not rowptr[rows] writes no edge at all and raises *bad (sticky: the
// caller clears it): every slot the pass writes is below rowptr[rows] = E.
__global__ void __launch_bounds__(256)
sop_graph_fill_kernel(int rows, int n, int E, const float *prec, const float *dist, const int32_t *rowptr, int32_t *src32,
                      int32_t *dst32, float *edge_attr, int64_t *cell, int32_t *bad) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  if (rowptr[rows] != E) {
    if (row == 0 && lane == 0) *bad = 1;
    return;
  }
  const int u = row % n;
  const float *prow = prec + (size_t)row * n, *drow = dist + (size_t)row * n;
  int at = max(rowptr[row], 0);
  const int end = min(rowptr[row + 1], E);
  for (int v0 = 0; v0 < n; v0 += 64) {
    const int v = v0 + lane;
    const bool keep = sop_edge(prow, n, u, v);
    const unsigned long long m = __ballot(keep);
    const int slot = at + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    if (keep && slot < end) {                               // (slot < end always, unless prec changed between the passes)
      src32[slot] = row;
      dst32[slot] = row - u + v;
      edge_attr[slot] = drow[v];
      cell[slot] = (int64_t)row * n + v;
    }
    at += __popcll(m);
  }
}

}  // namespace daco

using namespace daco;

static long sop_graph_args(const char *what, int B, int n) {
  if (B <= 0 || n < 2) { set_error("%s: bad argument (B=%d n=%d; B >= 1, n >= 2)", what, B, n); return DACO_E_BADARG; }
  if ((long)B * n * n >= 0x80000000L) {
    set_error("%s: B * n * n = %ld cells do not fit 31 bits", what, (long)B * n * n);
    return DACO_E_TOOLARGE;
  }
  return DACO_OK;
}

extern "C" long daco_sop_graph_count(void *stream, int B, int n, const float *prec, int32_t *rowptr, int32_t *edge_off) {
  if (const long rc = sop_graph_args("daco_sop_graph_count", B, n)) return rc;
  if (!prec || !rowptr || !edge_off) { set_error("daco_sop_graph_count: bad argument (null pointer)"); return DACO_E_BADARG; }
  hipStream_t s = (hipStream_t)stream;
  const int rows = B * n;
  hipLaunchKernelGGL(sop_graph_count_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, rows, n, prec, rowptr);
  hipLaunchKernelGGL(sop_graph_scan_kernel, dim3(1), dim3(1024), 0, s, rows, n, rowptr, edge_off);
  return launch_status("sop_graph_count_kernel / sop_graph_scan_kernel");
}

extern "C" long daco_sop_graph_fill(void *stream, int B, int n, int E, const float *prec, const float *dist, const int32_t *rowptr,
                                    int32_t *src32, int32_t *dst32, float *edge_attr, int64_t *cell, int32_t *bad) {
  if (const long rc = sop_graph_args("daco_sop_graph_fill", B, n)) return rc;
  if (E < 1 || (long)E > (long)B * n * (n - 1)) {
    set_error("daco_sop_graph_fill: bad argument (E=%d; 1 <= E <= B n (n - 1) = %ld)", E, (long)B * n * (n - 1));
    return DACO_E_BADARG;
  }
  if (!prec || !dist || !rowptr || !src32 || !dst32 || !edge_attr || !cell || !bad) {
    set_error("daco_sop_graph_fill: bad argument (null pointer)");
    return DACO_E_BADARG;
  }
  hipStream_t s = (hipStream_t)stream;
  const int rows = B * n;
  hipLaunchKernelGGL(sop_graph_fill_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, rows, n, E, prec, dist, rowptr, src32,
                     dst32, edge_attr, cell, bad);
  return launch_status("sop_graph_fill_kernel");
}

static int knn_graph_launch(const char *what, void *stream, int B, int n, int k, const float *coords, float diag, float *dist,
                            int64_t *edge_src, int64_t *edge_dst, float *edge_attr, int32_t *src32, int32_t *dst32) {
  if (B <= 0 || n < 2 || k < 1 || k > n || !coords || !edge_src || !edge_dst || !edge_attr || (src32 == nullptr) != (dst32 == nullptr)) {
    set_error("%s: bad argument (B=%d n=%d k=%d)", what, B, n, k);
    return DACO_E_BADARG;
  }
  if (n > DACO_MAX_NODES) { set_error("%s: n=%d exceeds DACO_MAX_NODES", what, n); return DACO_E_TOOLARGE; }
  if (src32 && (long)B * n > 0x7fffffffL) { set_error("%s: B * n = %ld node ids do not fit 32 bits", what, (long)B * n); return DACO_E_TOOLARGE; }
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(((long)B * n + 3) / 4)), block(256);
  const int cpl = (n + 63) / 64;
#define DACO_KNN(C) hipLaunchKernelGGL(knn_graph_kernel<C>, grid, block, 0, s, B, n, k, coords, diag, dist, edge_src, edge_dst, edge_attr, src32, dst32)
  if (cpl <= 2) DACO_KNN(2);
  else if (cpl <= 4) DACO_KNN(4);
  else if (cpl <= 8) DACO_KNN(8);
  else if (cpl <= 16) DACO_KNN(16);
  else if (cpl <= 32) DACO_KNN(32);
  else DACO_KNN(64);
#undef DACO_KNN
  return launch_status("knn_graph_kernel");
}

extern "C" int daco_tsp_knn_graph(void *stream, int B, int n, int k, const float *coords, float diag, float *dist,
                                  int64_t *edge_src, int64_t *edge_dst, float *edge_attr) {
  return knn_graph_launch("daco_tsp_knn_graph", stream, B, n, k, coords, diag, dist, edge_src, edge_dst, edge_attr, nullptr, nullptr);
}

extern "C" int daco_tsp_knn_graph_csr(void *stream, int B, int n, int k, const float *coords, float diag, float *dist,
                                      int64_t *edge_src, int64_t *edge_dst, float *edge_attr, int32_t *src32, int32_t *dst32) {
  if (!src32 || !dst32) { set_error("daco_tsp_knn_graph_csr: src32 / dst32 missing"); return DACO_E_BADARG; }
  return knn_graph_launch("daco_tsp_knn_graph_csr", stream, B, n, k, coords, diag, dist, edge_src, edge_dst, edge_attr, src32, dst32);
}

template <typename T>
static void cvrp_knn_graph_dispatch(hipStream_t s, int B, int n, int k, const T *dist, long dist_bs, int64_t *edge_index,
                                    float *edge_attr, int32_t *src32, int32_t *dst32, int32_t *rowptr, int32_t *perm) {
  const dim3 grid((unsigned)(((long)B * n + 3) / 4)), block(256);
  const int cpl = (n + 63) / 64;
#define DACO_CVRP_KNN(C) hipLaunchKernelGGL((cvrp_knn_graph_kernel<T, C>), grid, block, 0, s, B, n, k, dist, dist_bs, edge_index, \
                                            edge_attr, src32, dst32, rowptr, perm)
  if (cpl <= 2) DACO_CVRP_KNN(2);
  else if (cpl <= 4) DACO_CVRP_KNN(4);
  else if (cpl <= 8) DACO_CVRP_KNN(8);
  else if (cpl <= 16) DACO_CVRP_KNN(16);
  else if (cpl <= 32) DACO_CVRP_KNN(32);
  else DACO_CVRP_KNN(64);
#undef DACO_CVRP_KNN
}

extern "C" long daco_cvrp_knn_graph(void *stream, int B, int n1, int k, const void *dist, int dist_f64, long dist_bstride,
                                    int64_t *edge_index, float *edge_attr, int32_t *src32, int32_t *dst32, int32_t *rowptr,
                                    int32_t *perm) {
  const int n = n1 - 1;                                   // customers
  if (B <= 0 || n1 < 2 || k < 1 || k > n || (dist_f64 != 0 && dist_f64 != 1) || dist_bstride < (long)n1 * n1) {
    set_error("daco_cvrp_knn_graph: bad argument (B=%d n1=%d k=%d dist_f64=%d dist_bstride=%ld; 1 <= k <= n1 - 1, n1 >= 2, "
              "dist_bstride >= n1 * n1)", B, n1, k, dist_f64, dist_bstride);
    return DACO_E_BADARG;
  }
  if (!dist || !edge_index || !edge_attr || !src32 || !dst32 || !rowptr || !perm) {
    set_error("daco_cvrp_knn_graph: bad argument (null pointer)");
    return DACO_E_BADARG;
  }
  if (n1 > DACO_MAX_NODES) { set_error("daco_cvrp_knn_graph: n1=%d exceeds DACO_MAX_NODES", n1); return DACO_E_TOOLARGE; }
  const long E = (long)n * (k + 2);
  if ((long)B * E > 0x7fffffffL || (long)B * n1 + 1 > 0x7fffffffL) {
    set_error("daco_cvrp_knn_graph: B * E = %ld edge ids / B * n1 = %ld node ids do not fit 32 bits", (long)B * E, (long)B * n1);
    return DACO_E_TOOLARGE;
  }
  hipStream_t s = (hipStream_t)stream;
  if (dist_f64) cvrp_knn_graph_dispatch<double>(s, B, n, k, (const double *)dist, dist_bstride, edge_index, edge_attr, src32, dst32, rowptr, perm);
  else cvrp_knn_graph_dispatch<float>(s, B, n, k, (const float *)dist, dist_bstride, edge_index, edge_attr, src32, dst32, rowptr, perm);
  return launch_status("cvrp_knn_graph_kernel");
}

extern "C" int daco_heu_matrix(void *stream, int B, int n, int E, const int64_t *edge_index, const float *heu, float fill, float add,
                               float *out, int32_t *bad) {
  if (B <= 0 || n < 1 || E < 0 || !edge_index || !heu || !out) {
    set_error("daco_heu_matrix: bad argument (B=%d n=%d E=%d)", B, n, E);
    return DACO_E_BADARG;
  }
  hipStream_t s = (hipStream_t)stream;
  const size_t total = (size_t)B * n * n, quads = total / 4;
  if (((uintptr_t)out & 15) != 0) { set_error("daco_heu_matrix: out must be 16-byte aligned"); return DACO_E_BADARG; }
  {
    const size_t want = (quads + 255) / 256;
    hipLaunchKernelGGL(heu_fill_kernel, dim3((unsigned)(want < 1 ? 1 : (want < 8192 ? want : 8192))), dim3(256), 0, s, total, fill, out);
  }
  if (E > 0)                                                // (the scatter follows the fill on the same stream)
    hipLaunchKernelGGL(heu_scatter_kernel, dim3((unsigned)(((size_t)B * E + 255) / 256)), dim3(256), 0, s, B, n, E, edge_index, heu, add,
                       out, bad);
  return launch_status("daco_heu_matrix");
}
