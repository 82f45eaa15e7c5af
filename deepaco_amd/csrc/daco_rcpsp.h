// daco_rcpsp.h -- the serial schedule generation scheme of rcpsp/aco.py:42-63 (SSGS_ordered) for one wavefront, shared by
// the decoder kernel of daco_rcpsp.hip and the construction kernel template (daco_sample_kernel.h, PROB_RCPSP), which
// decodes the route it has just drawn.
//
// The reference keeps, per resource, an event queue (rcpsp_inst.py:57-90): `available` units now, a sorted list of
// (release time, amount), and the time of the last request, which never goes back (request() asserts it).  So
// available_timestamp(v) is the first t >= last_r at which usage_r[t] <= cap_r - v, usage_r being the units in use per time
// slot: the releases up to t are exactly the activities that end by t.  request(t, v, d) adds v to the slots [t, t + d) and
// sets last_r = t.  There is no back-filling before last_r: this is the reference's rule, not the textbook's.
//
// One wavefront owns its ant's state in LDS: the route (u16), `ready` (the largest end time among the scheduled
// predecessors, -1 = none yet, -2 = the activity has no predecessor), `fin` (end time once scheduled, -1 before) and the R
// usage timelines (u16 slots).  The search from last_r probes 64 slots per ballot; the request is a strided add.
#pragma once
#include "daco_device.h"

namespace daco {

struct RcpspDev {
  // instance data, dense per instance
  int R = 0, H = 0, E = 0;          // resources, time slots per timeline, allocated successor entries per instance
  const int32_t *dur = nullptr;     // [B][n]
  const int32_t *req = nullptr;     // [B][n][R]
  const int32_t *cap = nullptr;     // [B][R]
  const int32_t *es = nullptr;      // [B][n] earliest start
  const int32_t *ls = nullptr;      // [B][n] latest start
  const int32_t *sptr = nullptr;    // [B][n + 1]
  const int32_t *sidx = nullptr;    // [B][E]
  int32_t *starts = nullptr;        // out [B][n][A] or null
  int32_t *costs = nullptr;         // out [B][A]
  // construction (daco_rcpsp_sample)
  int fused = 0;                    // the construction kernel decodes its own routes (LDS plan fits four waves)
  int rule = 0;                     // 0 direct, 1 summation, 2 balanced (rcpsp/aco.py:190-206)
  float gamma = 0.0f, cdir = 1.0f, csum = 0.0f;
  const float *taup = nullptr;      // [B][n][ld] tau, zero padded
  const float *etab = nullptr;      // [B][n][ld] eta^beta, zero padded
};

constexpr int RCPSP_MAX_N = 256, RCPSP_MAX_R = 8, RCPSP_MAX_H = 8192;
constexpr int RCPSP_FLAG_ORDER = 4, RCPSP_FLAG_RESOURCE = 8;

__host__ __device__ inline int rcpsp_hs(int H) { return (H + 1) & ~1; }
// LDS bytes of one wavefront: route | ready | fin | R timelines
__host__ __device__ inline size_t rcpsp_wave_lds(int n, int R, int H) {
  return ((size_t)(((2 * n + 15) & ~15) + 8 * n + 2 * R * rcpsp_hs(H)) + 15) & ~(size_t)15;
}

// Decodes route[0..n) (LDS, entries already checked to lie in [0, n)) of instance b into start times.  Returns the flag bits;
// *cost = start of activity n-1.  starts_out: this ant's column (stride A) or null.
__device__ inline int ssgs_wave(const RcpspDev &q, int n, int b, int A, unsigned char *lds, int lane, int32_t *starts_out, int *cost) {
  const int R = q.R, H = q.H, Hs = rcpsp_hs(H);
  const uint16_t *route = reinterpret_cast<const uint16_t *>(lds);
  int32_t *ready = reinterpret_cast<int32_t *>(lds + ((2 * n + 15) & ~15));
  int32_t *fin = ready + n;
  uint16_t *usage = reinterpret_cast<uint16_t *>(fin + n);
  const int32_t *dur = q.dur + (size_t)b * n, *req = q.req + (size_t)b * n * R, *cap = q.cap + (size_t)b * R;
  const int32_t *es = q.es + (size_t)b * n, *ls = q.ls + (size_t)b * n;
  const int32_t *sptr = q.sptr + (size_t)b * (n + 1), *sidx = q.sidx + (size_t)b * q.E;
  int flags = 0;
  for (int k = lane; k < n; k += 64) { ready[k] = -2; fin[k] = -1; }
  {
    uint32_t *u32 = reinterpret_cast<uint32_t *>(usage);
    for (int i = lane; i < R * (Hs >> 1); i += 64) u32[i] = 0u;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const int etot = min(max(sptr[n], 0), q.E);
  for (int e = lane; e < etot; e += 64) {              // whoever is somebody's successor waits for a predecessor
    const int k = sidx[e];
    if (k >= 0 && k < n) ready[k] = -1; else flags |= RCPSP_FLAG_ORDER;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  int last = 0;                                        // lane r: last_event_time of resource r
  const int capl = lane < R ? cap[lane] : 0;
  int c_out = 0;
  for (int i = 0; i < n; ++i) {
    const int j = __builtin_amdgcn_readfirstlane((int)route[i]);
    const int d_in = dur[j], lsj = ls[j], esj = es[j];
    const int d = d_in < 0 ? 0 : (d_in > H ? H : d_in);
    if (d != d_in) flags |= RCPSP_FLAG_RESOURCE;
    const int vl = lane < R ? req[(size_t)j * R + lane] : 0;          // lane r: the requirement on resource r
    const int rd = ready[j];
    if (fin[j] >= 0 || rd == -1) flags |= RCPSP_FLAG_ORDER;         // twice in the route / before one of its predecessors
    int arrange = 0;
    const uint64_t need = __ballot(vl > 0);
    for (uint64_t m = need; m; m &= m - 1) {
      const int r = __builtin_ctzll(m);
      const int v = readlane_i(vl, r), room = readlane_i(capl, r) - v;
      if (room < 0 || readlane_i(capl, r) > 65535) { flags |= RCPSP_FLAG_RESOURCE; continue; }
      const uint16_t *ur = usage + (size_t)r * Hs;
      int t0 = readlane_i(last, r);
      t0 = t0 < 0 ? 0 : t0;
      for (;; t0 += 64) {                              // ends: every slot from H on is free
        const int t = t0 + lane;
        const bool ok = t >= H || (int)ur[t] <= room;
        const uint64_t f = __ballot(ok);
        if (f) { t0 += __builtin_ctzll(f); break; }
      }
      arrange = max(arrange, t0);
    }
    // rcpsp/aco.py:53-55: the predecessors' ends (earlist_start without any), then the clamp to [., latest_start]
    const int est = rd >= 0 ? rd : (rd == -1 ? 0 : esj);
    arrange = min(max(arrange, est), lsj);
    arrange = __builtin_amdgcn_readfirstlane(arrange);
    if (arrange < 0 || arrange > H) { flags |= RCPSP_FLAG_RESOURCE; arrange = arrange < 0 ? 0 : H; }
    // request(): the clock of a resource never goes back, and what is in use never exceeds the capacity (the reference
    // asserts both; after the clamp to latest_start either may fail, which is flagged here)
    if (vl > 0 && arrange < last) flags |= RCPSP_FLAG_RESOURCE;
    if (vl > 0) last = arrange;
    for (uint64_t m = need; m; m &= m - 1) {
      const int r = __builtin_ctzll(m);
      const int v = readlane_i(vl, r), cr = readlane_i(capl, r);
      uint16_t *ur = usage + (size_t)r * Hs;
      for (int t = arrange + lane; t < arrange + d; t += 64) {
        if (t < H) {
          const int u = (int)ur[t] + v;
          ur[t] = (uint16_t)(u > 65535 ? 65535 : u);
          if (u > cr) flags |= RCPSP_FLAG_RESOURCE;
        } else flags |= RCPSP_FLAG_RESOURCE;           // beyond the horizon the caller declared
      }
    }
    const int end = arrange + d;
    if (lane == 0) {
      fin[j] = end;
      if (starts_out) starts_out[(size_t)j * A] = arrange;
    }
    if (j == n - 1) c_out = arrange;
    const int e0 = max(sptr[j], 0), e1 = min(sptr[j + 1], q.E);
    for (int e = e0 + lane; e < e1; e += 64) {
      const int k = sidx[e];
      if (k >= 0 && k < n) {
        if (fin[k] >= 0) flags |= RCPSP_FLAG_ORDER;
        const int old = ready[k];
        ready[k] = old > end ? old : end;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  *cost = c_out;
  // the lanes' flag bits, combined
  const int f4 = __ballot((flags & RCPSP_FLAG_ORDER) != 0) ? RCPSP_FLAG_ORDER : 0;
  const int f8 = __ballot((flags & RCPSP_FLAG_RESOURCE) != 0) ? RCPSP_FLAG_RESOURCE : 0;
  return f4 | f8;
}

}  // namespace daco
