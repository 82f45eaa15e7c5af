// daco_host.h -- what the C entry points share: the layout of every workspace that more than one of them carves, the rule for
// 16-byte row vectors, and the tail of a launch (status, events).  Host code only; each layout is written down here once, its
// exported size function and every entry point that reads or writes the buffer go through it.  (align256 itself is in
// daco_device.h: the 2-opt and HGS tables are laid out with it on the device too.)
#pragma once
#include "daco_device.h"
#include "daco_head_rows.h"
#include "../../include/deepaco_hip.h"

namespace daco {

// chunks per lane actually instantiated (compile-time loop bounds): the row is padded with
// zeros up to the next instantiated size; zero padding never changes a sum or a draw.
inline int inst_chunks(int n) {
  const int vec = vec_for_n(n), need = ld_for_n(n) / (64 * vec);
  static const int avail[] = {1, 2, 3, 4, 6, 8, 12, 16};
  for (int c : avail) if (c >= need) return c;
  return -1;
}
inline int ld_alloc(int n) { return inst_chunks(n) * 64 * vec_for_n(n); }

// rows of two [.][n][n] matrices can be read as aligned 16-byte vectors: n % 4 == 0, aligned bases and instance strides
inline bool rows_vec4(int n, const float *a, long a_bstride, const float *b, long b_bstride) {
  return (n & 3) == 0 && (a_bstride & 3) == 0 && (b_bstride & 3) == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
}

// ------------------------------------------------------------------ probability workspace of the dense samplers
// P | 1/P (the race on Philox draws only) | aux (the sibling constructions' padded matrix), each [B][n][ld_alloc(n)] f32
struct ProbWs {
  float *P, *R, *aux;
  static size_t mat_bytes(int B, int n) { return align256((size_t)B * n * ld_alloc(n) * sizeof(float)); }
  static int mats(int mode) { return mode == DACO_RACE_PHILOX ? 2 : 1; }
  static size_t bytes(int B, int n, int mode, bool aux = false) { return (mats(mode) + (aux ? 1 : 0)) * mat_bytes(B, n); }
  static ProbWs carve(const void *base, int B, int n, int mode) {
    char *p = (char *)base;
    const size_t mat = mat_bytes(B, n);
    return {(float *)p, mode == DACO_RACE_PHILOX ? (float *)(p + mat) : nullptr, (float *)(p + mats(mode) * mat)};
  }
};

// RCPSP: P | 1/P | adjacency | tau | eta^beta, the same padded matrices (all five whatever the mode)
struct RcpspWs {
  float *P, *R, *adj, *tau, *etab;
  static size_t bytes(int B, int n) { return 5 * ProbWs::mat_bytes(B, n); }
  static RcpspWs carve(void *base, int B, int n) {
    char *p = (char *)base;
    const size_t mat = ProbWs::mat_bytes(B, n);
    return {(float *)p, (float *)(p + mat), (float *)(p + 2 * mat), (float *)(p + 3 * mat), (float *)(p + 4 * mat)};
  }
};

// ------------------------------------------------------------------ directed successor table (CVRP sampler -> pheromone update)
// next [B][n][A] successor per (node, ant) | hubmask [B][A][ceil(n/32)] per-ant set of depot successors | lens [B][A] route length
struct DirectedTable {
  uint32_t *next, *hubmask;
  int32_t *lens;
  static size_t next_bytes(int B, int n, int A) { return (size_t)B * n * A * sizeof(uint32_t); }
  static size_t hubmask_bytes(int B, int n, int A) { return (size_t)B * A * ((n + 31) / 32) * sizeof(uint32_t); }
  static size_t bytes(int B, int n, int A) {
    return align256(next_bytes(B, n, A)) + align256(hubmask_bytes(B, n, A)) + align256((size_t)B * A * sizeof(int32_t));
  }
  static DirectedTable carve(const void *base, int B, int n, int A) {
    char *p = (char *)base, *h = p + align256(next_bytes(B, n, A));
    return {(uint32_t *)p, (uint32_t *)h, (int32_t *)(h + align256(hubmask_bytes(B, n, A)))};
  }
};

// ------------------------------------------------------------------ workspace of the head-row samplers (129 <= n <= 1024)
// dense rows P [B][n][ld] | head rows (daco_pheromone_update_heads writes both) | u16 tours [B][A][ld] (n > 512: as they are
// built; n <= 512: written by a call that asks for no int64 paths) | general tail: tau^alpha [B][n][n] | eta^beta [B or 1][n][n]
struct HeadWs {
  int ld;
  float *P;
  char *hrow;
  uint16_t *tours16;
  float *tau_pow, *eta_pow;                // only in a workspace of bytes_general()
  static int ld_for(int n) { return n <= 512 ? 512 : 1024; }   // (the row walks of the kernel's two instantiations read 512 / 1024 candidates)
  static size_t dense_bytes(int B, int n) { return align256((size_t)B * n * ld_for(n) * sizeof(float)); }
  static size_t tours_offset(int B, int n) { return dense_bytes(B, n) + align256((size_t)B * n * sp_head_row_bytes(SP_KH_MAX / 16)); }
  static size_t bytes(int B, int n, int A) { return tours_offset(B, n) + align256(((size_t)B * A + 16) * ld_for(n) * sizeof(uint16_t)); }
  static size_t pow_bytes(int B, int n) { return align256((size_t)B * n * n * sizeof(float)); }
  static size_t bytes_general(int B, int n, int A) { return bytes(B, n, A) + 2 * pow_bytes(B, n); }
  static HeadWs carve(void *base, int B, int n, int A) {
    char *p = (char *)base, *tail = p + bytes(B, n, A);
    return {ld_for(n), (float *)p, p + dense_bytes(B, n), (uint16_t *)(p + tours_offset(B, n)), (float *)tail, (float *)(tail + pow_bytes(B, n))};
  }
};

// ------------------------------------------------------------------ the tail of a launch
// DACO_OK, or daco_last_error() = "<what> launch: <the runtime's words>" and DACO_E_HIP
inline int launch_status(hipError_t e, const char *what) {
  if (e == hipSuccess) return DACO_OK;
  set_error("%s launch: %s", what, hipGetErrorString(e));
  return DACO_E_HIP;
}
// the status of the launches since the last check
inline int launch_status(const char *what) { return launch_status(hipGetLastError(), what); }

// the caller's optional timing events: which = "ev_begin" before the sampler's launch, "ev_end" after it
inline int record_event(void *ev, hipStream_t s, const char *which) {
  if (ev && hipEventRecord((hipEvent_t)ev, s) != hipSuccess) { set_error("hipEventRecord(%s) failed", which); return DACO_E_HIP; }
  return DACO_OK;
}

}  // namespace daco
