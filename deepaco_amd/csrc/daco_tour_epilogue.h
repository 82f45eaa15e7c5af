// daco_tour_epilogue.h -- how the finished tours of a TSP construction workgroup leave LDS, written once for the samplers
// that end this way: tsp_sample_kernel (daco_sample_kernel.h, one ant per wavefront), tsp_scan32_kernel (daco_tsp_scan32.hip),
// scan16_kernel (daco_scan16_kernel.h, its TSP branch) and both epilogues of scan_sparse_kernel (daco_scan_sparse.hip).
// A stage that could not be held at the parent's registers or time through these functions stays in its kernel's text on
// epi_chunk_sum and epi_edge, figures at the site: the costs of scan16_kernel and tsp_scan32_kernel, costs and table at n > 512.
//
// The workgroup's tours sit in LDS as rows of node ids.  Three stages, each asked for by a pointer of SampleParams and each run
// by all 256 threads (per-step stores and gathers with one active lane cost more than the row stream of the step loop):
//   epi_paths        paths[b][t][abase + k] (int64): G lanes write one run of G ants per step row;
//   epi_tour_costs   tour lengths (tsp/aco.py:121-132): sum_t d[u_t][u_{t-1}], t = 1 .. n-1, then the closing edge d[u_0][u_{n-1}]
//                    -- f32, that order.  DSW edges of each of the wavefront's ants are gathered with every lane active and
//                    staged in LDS; the ant's leading lane adds them one after the other (epi_chunk_sum: the arithmetic rule
//                    oracle.tour_costs restates);
//   epi_nbr_table    the pheromone update's table nbr[node][ant] = prev | next << 16: the tours are inverted in (dead) LDS -- zero
//                    fill, barrier, inv[k][tour_k[t]] = t, barrier -- and then NI lanes write one run per node row.
// A stage is templated on the width of its group of ants and on the accessor that answers "node at step t of tour k"; LDS
// layouts, staging places, the order of the stages and the barriers in front of them belong to the calling kernel.
#pragma once
#include <cstdint>

namespace daco {

// whole tours, one row of `stride` entries per ant (u16, or bytes where every id fits one)
template <class T>
struct TourRows {
  const T *base;
  int stride;
  __device__ __forceinline__ uint32_t operator()(int k, int t) const { return base[k * stride + t]; }
};
// two pieces per ant (the split-tour variant of scan_sparse_kernel): entries 0 .. TE-1 in rows of EW, the rest in rows of W
template <int EW, int W>
struct TourSplit {
  const uint16_t *early, *late;
  int TE;
  // (a select between two addresses, then one load: selecting the index and the base separately cost three VALU per entry)
  __device__ __forceinline__ uint32_t operator()(int k, int t) const { return *(t < TE ? early + k * EW + t : late + k * W + (t - TE)); }
};

// pb = &paths[b][0][first ant of the group]; ants k >= nant of the group do not exist
// NT: non-temporal stores -- nothing on the device reads the int64 paths again within the launch.  The head-row kernel at
// n <= 512 asks for it: in a colony's loop its launch goes 453.9 -> 425.5 us and reads 32 MB less past the L2 (FETCH_SIZE 149 477
// -> 133 838 KiB, WRITE_SIZE unchanged), the iteration 0.5353-0.5371 -> 0.5101-0.5138 ms; stand-alone launches gain 4-9 us only
// (profiles/iteration_tail_ab.txt part D).  Inferred from that, not counted: the stream of paths (131 MB at TSP-500 x 512 x 64)
// no longer takes the Infinity Cache from what the next launches read.  The other samplers keep plain stores, unmeasured.
template <int G, bool NT = false, class Tour>
__device__ __forceinline__ void epi_paths(const Tour &tour, int64_t *pb, int n, int A, int nant) {
  const int k = threadIdx.x & (G - 1);
  if (k < nant)
    for (int t = threadIdx.x / G; t < n; t += 256 / G) {
      if constexpr (NT) __builtin_nontemporal_store((int64_t)tour(k, t), &pb[(size_t)t * A + k]);
      else pb[(size_t)t * A + k] = (int64_t)tour(k, t);
    }
}

// where the length of edge u -> v is read: dist[u][v], or with `tri` (the caller's statement that dist[u][v] and dist[v][u] are
// the same bits) the upper triangle's dist[min(u, v)][max(u, v)] -- the same values from half the lines
__device__ __forceinline__ uint32_t epi_edge(uint32_t u, uint32_t v, int n, bool tri) {
  const bool sw = tri && v < u;
  return (sw ? v : u) * (uint32_t)n + (sw ? u : v);
}

// the ordered sum of one staged chunk: DSW edge lengths added one after the other, in step order (slots past the tour's end
// hold +0.0f).  The order of these additions is the specification; every sampler's tour length goes through here.
template <int DSW>
__device__ __forceinline__ float epi_chunk_sum(float cost, const float *stage) {
#pragma unroll
  for (int v4 = 0; v4 < DSW / 4; ++v4) {
    const float4 v = *reinterpret_cast<const float4 *>(stage + 4 * v4);
    cost = cost + v.x; cost = cost + v.y; cost = cost + v.z; cost = cost + v.w;
  }
  return cost;
}

// One wavefront, the APW ants k0 .. k0+APW-1 of the group (64 / APW lanes each, the first of them leads): passes of DSW (32 or
// 64) edges per ant -- gather, stage, wave barrier, the leading lanes add, wave barrier -- then the closing edge and the store.
// stage: this wavefront's [APW][DSW] floats; costs_g = &costs[b][first ant of the group]; tours k >= nk of the group are not
// read and their lengths not stored.
template <int DSW, int APW, class Tour>
__device__ __forceinline__ void epi_tour_costs(const Tour &tour, int k0_, int nk, int n, const float *dist_b, bool tri, float *stage,
                                               float *costs_g) {
  static_assert((DSW == 32 || DSW == 64) && APW * DSW >= 64 && 64 % APW == 0, "whole passes of the wavefront");
  const int k0 = __builtin_amdgcn_readfirstlane(k0_);      // (the same in every lane: "tour k exists" is decided on the scalar unit)
  const int lane = threadIdx.x & 63, q = lane / (64 / APW), slot = lane & (DSW - 1);
  const bool lead = (lane & (64 / APW - 1)) == 0;
  float cost = 0.0f;
  for (int base = 1; base < n; base += DSW) {
    const int t = base + slot;
#pragma unroll
    for (int r = 0; r < APW; r += 64 / DSW) {
      const int j = r + lane / DSW;
      float dv = 0.0f;
      if (t < n && k0 + j < nk) dv = dist_b[epi_edge(tour(k0 + j, t), tour(k0 + j, t - 1), n, tri)];
      stage[j * DSW + slot] = dv;
    }
    __builtin_amdgcn_wave_barrier();
    if (lead) cost = epi_chunk_sum<DSW>(cost, stage + q * DSW);
    __builtin_amdgcn_wave_barrier();
  }
  if (lead && k0 + q < nk) {
    cost = cost + dist_b[epi_edge(tour(k0 + q, 0), tour(k0 + q, n - 1), n, tri)];
    costs_g[k0 + q] = cost;
  }
}

// The table of the nh <= NI ants k0 .. k0+nh-1 of the group.  inv: [NI][IL] u16 of dead LDS (IL >= n, NI * IL a multiple of 8,
// 16-byte aligned); nb = the table's entry of node 0 and the first of these ants, nstride = entries between two nodes (classic
// layout [B][n][A]: A; grouped [B][ceil(A/8)][n][8]: 8).  Every thread of the workgroup calls it (two barriers inside); the barrier
// that ends the last use of `inv`'s bytes is the caller's.
template <int NI, class Tour>
__device__ __forceinline__ void epi_nbr_table(const Tour &tour, int k0, uint16_t *inv, int IL, int nh, int n, uint32_t *nb, size_t nstride) {
  const int k = threadIdx.x & (NI - 1);
  for (int e = threadIdx.x; e < NI * IL / 8; e += 256) reinterpret_cast<uint4 *>(inv)[e] = make_uint4(0, 0, 0, 0);
  __syncthreads();
  const int kt = k0 + (k < nh ? k : 0);                    // (the other slots hold no tour: their entries are not nodes)
  if (k < nh)
    for (int t = threadIdx.x / NI; t < n; t += 256 / NI) inv[k * IL + tour(kt, t)] = (uint16_t)t;
  __syncthreads();
  if (k < nh)
    for (int node = threadIdx.x / NI; node < n; node += 256 / NI) {
      const int t = inv[k * IL + node];
      const uint32_t pv = tour(kt, t == 0 ? n - 1 : t - 1), nx = tour(kt, t == n - 1 ? 0 : t + 1);
      nb[(size_t)node * nstride + k] = pv | (nx << 16);
    }
}

}  // namespace daco
