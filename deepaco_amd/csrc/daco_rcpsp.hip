// daco_rcpsp.hip -- the resource-constrained project scheduling colony of rcpsp/aco.py on the device.
//
// Reference behaviour replaced:
//   update_cost (rcpsp/aco.py:222-236): every ant's activity list decoded by SSGS_ordered (:42-63), one ant at a time in
//     interpreted Python through per-resource event queues re-sorted on every request (rcpsp_inst.py:57-90)
//     -> rcpsp_schedule_kernel, or the tail of the construction kernel: one wavefront per (project, ant), daco_rcpsp.h;
//   construct_solutions (:176-213): n-1 draws from activity 0 under precedence constraints, with the direct, summation and
//     balanced evaluation of Merkle et al. (:190-206) -> PROB_RCPSP of the construction template (daco_sample_kernel.h),
//     launched through its launch_sample with the decoder's LDS plan; the draw code, modes, noise layout and Philox counters
//     are those of daco_sibling_sample;
//   the best-so-far bookkeeping of update_cost and the deposit list of update_pheromone (:238-256) -> rcpsp_track_kernel, which
//     lays out [best-so-far route | iteration-best ant or every ant] with their weights for daco_pheromone_update
//     (symmetric = 0, hub = -1), whose sequential per-row adds reproduce the reference's index_put order bit for bit;
//   autograd through Categorical.log_prob of :207-213 -> rcpsp_backward_kernel.
//
// Limits (DACO_E_TOOLARGE beyond): n <= 256 activities, R <= 8 resources, horizon <= 8192 time slots (the horizon is
// max(latest_start + duration); with the reference's default time windows that is the sum of all durations), capacities
// <= 65535.  One wavefront's LDS is 2n + 8n + 2 R horizon bytes: PSPLIB j120 takes 7 KB, the largest plan 130 KB (one
// wavefront per workgroup then).  The construction kernel decodes its own routes while four such plans fit 64 KB (every
// PSPLIB set does); beyond that daco_rcpsp_sample launches the decoder kernel after it.
#include "daco_sample_kernel.h"

namespace daco {

constexpr size_t RCPSP_LDS_PLAIN = 64 * 1024, RCPSP_LDS_MAX = 160 * 1024;

__global__ void __launch_bounds__(256)
rcpsp_schedule_kernel(const RcpspDev q, int B, int n, int A, const int64_t *routes, int32_t *flags) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rc_smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
  const long idx = (long)blockIdx.x * wpb + wave;
  if (idx >= (long)B * A) return;                       // (no workgroup barrier below)
  const int b = (int)(idx / A), a = (int)(idx - (long)b * A);
  unsigned char *lds = rc_smem + (size_t)wave * rcpsp_wave_lds(n, q.R, q.H);
  uint16_t *route = reinterpret_cast<uint16_t *>(lds);
  bool bad = false;
  for (int i = lane; i < n; i += 64) {
    const int64_t v = routes[((size_t)b * n + i) * A + a];
    bad = bad || v < 0 || v >= n;
    route[i] = (uint16_t)(v < 0 || v >= n ? 0 : v);
  }
  if (__ballot(bad)) {                                  // not activity ids: nothing is decoded
    if (lane == 0) { q.costs[(size_t)b * A + a] = -1; if (flags) atomicOr(flags + b, RCPSP_FLAG_ORDER); }
    return;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  int cost = 0;
  const int f = ssgs_wave(q, n, b, A, lds, lane, q.starts ? q.starts + (size_t)b * n * A + a : nullptr, &cost);
  if (lane == 0) {
    q.costs[(size_t)b * A + a] = cost;
    if (f && flags) atomicOr(flags + b, f);
  }
}

static hipError_t launch_schedule(const RcpspDev &q, int B, int n, int A, const int64_t *routes, int32_t *flags, hipStream_t s) {
  const size_t pw_ = rcpsp_wave_lds(n, q.R, q.H);
  const int wpb = 4 * pw_ <= RCPSP_LDS_PLAIN ? 4 : (2 * pw_ <= RCPSP_LDS_MAX ? 2 : 1);
  const size_t dyn = wpb * pw_;
  if (dyn > RCPSP_LDS_PLAIN)
    (void)hipFuncSetAttribute((const void *)rcpsp_schedule_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
  const long waves = (long)B * A;
  hipLaunchKernelGGL(rcpsp_schedule_kernel, dim3((unsigned)((waves + wpb - 1) / wpb)), dim3(64 * wpb), dyn, s, q, B, n, A, routes, flags);
  return hipGetLastError();
}

// ------------------------------------------------------------------ best-so-far bookkeeping and the deposit list
// One wavefront per project.  rcpsp/aco.py:228-236 (first minimum; strictly better replaces the record; max = Q n / cost in
// float64) and :242-252: column 0 = the best-so-far route with weight f32(Q / best_cost) (a float64 quotient), then the
// iteration-best ant (elitist) or every ant in index order with the float32 quotient Q / cost.
// alias != 0 reproduces the reference's best_solution.route, a VIEW of row `bestindex` of self.routes: from the second
// iteration on it reads whatever that ant drew last.
__global__ void __launch_bounds__(64)
rcpsp_track_kernel(int n, int A, const int64_t *routes, const int32_t *starts, const int32_t *costs, double Q, int elitist, int alias,
                   float tmin, int32_t *best_cost, int32_t *best_idx, int64_t *best_route, int32_t *best_sched,
                   int64_t *upd_routes, float *upd_weights, float *clamp_min, float *clamp_max) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int32_t *cb = costs + (size_t)b * A;
  float bk = __builtin_inff();
  int bi = 0x7fffffff;
  for (int a = lane; a < A; a += 64) {                  // (a lane's indices ascend: strict < keeps its first minimum)
    const float c = (float)cb[a];                       // costs are below 2^24: exact
    if (c < bk) { bk = c; bi = a; }
  }
  const KeyIdx r = wave_arg<false>(bk, bi);
  const int ibest = r.idx, icost = cb[ibest];
  const bool improved = icost < best_cost[b];
  const int cost_now = improved ? icost : best_cost[b];
  const int idx_now = improved ? ibest : best_idx[b];
  const int C = elitist ? 2 : A + 1;
  const int64_t *rb = routes + (size_t)b * n * A;
  for (int i = lane; i < n; i += 64) {
    const int64_t v = (improved || alias) ? rb[(size_t)i * A + idx_now] : best_route[(size_t)b * n + i];
    best_route[(size_t)b * n + i] = v;
    if (improved && best_sched) best_sched[(size_t)b * n + i] = starts[((size_t)b * n + i) * A + ibest];
    int64_t *u = upd_routes + ((size_t)b * n + i) * C;
    u[0] = v;
    if (elitist) u[1] = rb[(size_t)i * A + ibest];
    else for (int a = 0; a < A; ++a) u[1 + a] = rb[(size_t)i * A + a];
  }
  float *w = upd_weights + (size_t)b * C;
  if (lane == 0) {
    w[0] = (float)(Q / (double)cost_now);
    if (elitist) w[1] = (float)Q / (float)icost;
    if (improved) { best_cost[b] = icost; best_idx[b] = ibest; }
    if (clamp_min) {
      // the reference clamps from above first, then from below (:255-256); daco_pheromone_update from below first: the
      // two agree unless max < min, where the reference leaves min everywhere -- as does an upper bound raised to min
      const float mx = (float)(Q * (double)n / (double)cost_now);
      clamp_min[b] = tmin;
      clamp_max[b] = mx < tmin ? tmin : mx;
    }
  }
  if (!elitist) for (int a = lane; a < A; a += 64) w[1 + a] = (float)Q / (float)cb[a];
}

// ------------------------------------------------------------------ gradient of the log-probabilities w.r.t. the heuristic
// Every term of a rule's weight is proportional to eta[prev][k]^beta: w_k = base_k eta^beta with base_k = tau^alpha (direct),
// s^alpha (summation) or c tau^alpha + (1 - c) s^alpha (balanced), so
//   d log p / d eta[prev][k] = beta ( [k = pick] / eta - w_k / (eta S) ),   0 where the probability was clamped,
// with the conventions of dprob_deta at eta = 0.  One wavefront per (project, ant) replays the route: lane l owns the
// candidates l + 64 c.  A row of grad_eta is touched by one step of an ant only (an activity is left once), so the adds of
// one wavefront never meet; across ants they do: hardware f32 atomics, reproducible to rounding.
__global__ void __launch_bounds__(256)
rcpsp_backward_kernel(int B, int n, int A, const float *indeg, const float *adj, const float *tau, long tau_bs, const float *eta,
                      long eta_bs, float alpha, float beta, int rule, float gamma, float cdir, float csum, const int64_t *routes,
                      const float *rowsum, const float *grad_logp, float *grad_eta) {
  constexpr int CHK = RCPSP_MAX_N / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bpi = (A + 3) >> 2;
  const int b = blockIdx.x / bpi, a = (blockIdx.x - b * bpi) * 4 + wave;
  if (a >= A) return;
  const float *tb = tau + (size_t)b * tau_bs, *eb = eta + (size_t)b * eta_bs, *ab = adj + (size_t)b * n * n;
  const int64_t *path = routes + (size_t)b * n * A + a;
  const float *rs = rowsum + (size_t)b * (n - 1) * A + a, *gl = grad_logp + (size_t)b * (n - 1) * A + a;
  float *grad = grad_eta + (size_t)b * n * n;
  float cnt[CHK], ssum[CHK];
  uint32_t vis = 0;
  int prev = (int)path[0];
  prev = prev < 0 || prev >= n ? 0 : prev;
  if ((prev & 63) == lane) vis |= 1u << (prev >> 6);
#pragma unroll
  for (int c = 0; c < CHK; ++c) {
    const int k = lane + 64 * c;
    ssum[c] = 0.0f;
    cnt[c] = k < n ? indeg[(size_t)b * n + k] - ab[(size_t)prev * n + k] : 1.0f;
  }
  for (int t = 1; t < n; ++t) {
    int j = (int)path[(size_t)t * A];
    j = j < 0 || j >= n ? 0 : j;
    const float g = gl[(size_t)(t - 1) * A], S = rs[(size_t)(t - 1) * A];
    const float *trow = tb + (size_t)prev * n, *erow = eb + (size_t)prev * n;
    float wk[CHK], base[CHK], ek[CHK];
    bool open[CHK];
#pragma unroll
    for (int c = 0; c < CHK; ++c) {
      const int k = lane + 64 * c, kc = k < n ? k : 0;
      const float tk = trow[kc];
      ek[c] = erow[kc];
      ssum[c] = gamma * ssum[c] + tk;
      open[c] = k < n && !((vis >> c) & 1u) && cnt[c] == 0.0f;
      const float eb_ = pw(ek[c], beta);
      if (rule == 0) { base[c] = pw(tk, alpha); wk[c] = base[c] * eb_; }
      else {
        const float sw = pw(ssum[c], alpha);
        base[c] = rule == 1 ? sw : cdir * pw(tk, alpha) + csum * sw;
        wk[c] = rule == 1 ? sw * eb_ : cdir * (pw(tk, alpha) * eb_) + csum * (sw * eb_);
      }
    }
    if (g != 0.0f) {
      float wj = 0.0f;
#pragma unroll
      for (int c = 0; c < CHK; ++c) wj = (j >> 6) == c ? wk[c] : wj;
      wj = readlane_f(wj, j & 63);
      const float pr = wj / S;
      if (pr > DACO_EPS_F32 && pr < 1.0f - DACO_EPS_F32) {      // inside the clamp: gradient flows
        const float cg = g / S;
        float *grow = grad + (size_t)prev * n;
#pragma unroll
        for (int c = 0; c < CHK; ++c) {
          const int k = lane + 64 * c;
          if (open[c]) {
            const float e = ek[c];
            const float dw = e != 0.0f ? beta * (wk[c] / e) : (beta == 1.0f ? base[c] : (beta > 1.0f ? 0.0f : __builtin_inff()));
            float val = -cg * dw;
            if (k == j) val += g * beta / e;
            unsafeAtomicAdd(grow + k, val);
          }
        }
      }
    }
    if ((j & 63) == lane) vis |= 1u << (j >> 6);
#pragma unroll
    for (int c = 0; c < CHK; ++c) {
      const int k = lane + 64 * c;
      if (k < n) cnt[c] = cnt[c] - ab[(size_t)j * n + k];
    }
    prev = j;
  }
}

static bool rcpsp_rule(double gamma, double c, int *rule, float *g, float *cdir, float *csum) {
  // rcpsp/aco.py:190,196,201: gamma is a float32 tensor there, c a Python float
  *g = (float)gamma;
  *cdir = (float)c;
  *csum = (float)(1.0 - c);
  *rule = (*g < 0.05f || c == 1.0) ? 0 : (c == 0.0 ? 1 : 2);
  return gamma == gamma && c == c && gamma >= 0.0 && c >= 0.0 && c <= 1.0;
}

}  // namespace daco

using namespace daco;

static int rcpsp_check_sizes(const char *who, int B, int n, int A, int R, int horizon, int E) {
  if (B <= 0 || n < 2 || A <= 0 || R < 1 || horizon < 1 || E < 1) {
    set_error("%s: bad argument (B=%d n=%d A=%d R=%d horizon=%d E=%d)", who, B, n, A, R, horizon, E);
    return DACO_E_BADARG;
  }
  if (n > DACO_RCPSP_MAX_N || R > DACO_RCPSP_MAX_R || horizon > DACO_RCPSP_MAX_HORIZON) {
    set_error("%s: n=%d R=%d horizon=%d exceed the plan (n <= %d, R <= %d, horizon <= %d)", who, n, R, horizon, DACO_RCPSP_MAX_N,
              DACO_RCPSP_MAX_R, DACO_RCPSP_MAX_HORIZON);
    return DACO_E_TOOLARGE;
  }
  return DACO_OK;
}

static_assert(DACO_RCPSP_MAX_N == RCPSP_MAX_N && DACO_RCPSP_MAX_R == RCPSP_MAX_R && DACO_RCPSP_MAX_HORIZON == RCPSP_MAX_H, "limits");
static_assert(DACO_RCPSP_FLAG_ORDER == RCPSP_FLAG_ORDER && DACO_RCPSP_FLAG_RESOURCE == RCPSP_FLAG_RESOURCE, "flag bits");

static RcpspDev rcpsp_dev(int R, int horizon, int E, const int32_t *duration, const int32_t *resources, const int32_t *capacity,
                          const int32_t *earliest_start, const int32_t *latest_start, const int32_t *succ_ptr, const int32_t *succ_idx,
                          int32_t *starts, int32_t *costs) {
  RcpspDev q;
  q.R = R; q.H = horizon; q.E = E; q.dur = duration; q.req = resources; q.cap = capacity; q.es = earliest_start; q.ls = latest_start;
  q.sptr = succ_ptr; q.sidx = succ_idx; q.starts = starts; q.costs = costs;
  return q;
}

extern "C" int daco_rcpsp_schedule(void *stream, int B, int n, int A, int R, int horizon, int E, const int32_t *duration,
                                   const int32_t *resources, const int32_t *capacity, const int32_t *earliest_start,
                                   const int32_t *latest_start, const int32_t *succ_ptr, const int32_t *succ_idx,
                                   const int64_t *routes, int32_t *starts, int32_t *costs, int32_t *flags) {
  if (const int rc = rcpsp_check_sizes("daco_rcpsp_schedule", B, n, A, R, horizon, E)) return rc;
  if (!duration || !resources || !capacity || !earliest_start || !latest_start || !succ_ptr || !succ_idx || !routes || !costs) {
    set_error("daco_rcpsp_schedule: null pointer");
    return DACO_E_BADARG;
  }
  const RcpspDev q = rcpsp_dev(R, horizon, E, duration, resources, capacity, earliest_start, latest_start, succ_ptr, succ_idx, starts, costs);
  return launch_status(launch_schedule(q, B, n, A, routes, flags, (hipStream_t)stream), "rcpsp_schedule_kernel");
}

extern "C" size_t daco_rcpsp_workspace_bytes(int B, int n) {
  if (B <= 0 || n < 2 || n > DACO_RCPSP_MAX_N) return 0;
  return RcpspWs::bytes(B, n);
}

extern "C" int daco_rcpsp_sample(void *stream, int B, int n, int A, int R, int horizon, int E, const int32_t *duration,
                                 const int32_t *resources, const int32_t *capacity, const int32_t *earliest_start,
                                 const int32_t *latest_start, const int32_t *succ_ptr, const int32_t *succ_idx,
                                 const float *indegree, const float *adjacency, const float *tau, long tau_bstride,
                                 const float *eta, long eta_bstride, float alpha, float beta, double gamma, double c, int mode,
                                 const float *noise, uint64_t seed, uint64_t iter, uint32_t ant_gid0, int64_t *routes,
                                 float *logp, float *rowsum, int32_t *starts, int32_t *costs, int32_t *flags, void *workspace,
                                 size_t workspace_bytes) {
  if (const int rc = rcpsp_check_sizes("daco_rcpsp_sample", B, n, A, R, horizon, E)) return rc;
  if (!duration || !resources || !capacity || !earliest_start || !latest_start || !succ_ptr || !succ_idx || !indegree || !adjacency ||
      !tau || !eta || !routes || !costs || !workspace) {
    set_error("daco_rcpsp_sample: null pointer");
    return DACO_E_BADARG;
  }
  if (mode == DACO_SCAN_WAVE) mode = DACO_SCAN;
  if (mode < 0 || mode > 2) { set_error("daco_rcpsp_sample: bad mode %d", mode); return DACO_E_BADARG; }
  if (mode == DACO_RACE_NOISE && !noise) { set_error("daco_rcpsp_sample: DACO_RACE_NOISE needs a noise tensor"); return DACO_E_BADARG; }
  int rule;
  float g32, cdir, csum;
  if (!rcpsp_rule(gamma, c, &rule, &g32, &cdir, &csum)) { set_error("daco_rcpsp_sample: gamma >= 0 and 0 <= c <= 1 required"); return DACO_E_BADARG; }
  if (rule != 0 && !(alpha > 0.0f)) { set_error("daco_rcpsp_sample: the summation rule needs alpha > 0 (closed candidates are 0^alpha)"); return DACO_E_BADARG; }
  const size_t need = daco_rcpsp_workspace_bytes(B, n);
  if (workspace_bytes < need) { set_error("daco_rcpsp_sample: workspace %zu < %zu bytes", workspace_bytes, need); return DACO_E_WORKSPACE; }
  hipStream_t s = (hipStream_t)stream;
  const int vec = vec_for_n(n), ld = ld_alloc(n);
  const RcpspWs ws = RcpspWs::carve(workspace, B, n);
  float *const Rm = mode == DACO_RACE_PHILOX ? ws.R : nullptr;
  launch_prob_matrix(B, n, ld, tau, tau_bstride, eta, eta_bstride, alpha, beta, ws.P, Rm, s);
  launch_pad_matrix(B, n, ld, adjacency, (long)n * n, ws.adj, 0.0f, s);
  if (rule != 0) {                                      // x^1 = x and x^0 = 1 exactly (pw): tau itself and eta^beta, padded
    launch_prob_matrix(B, n, ld, tau, tau_bstride, eta, eta_bstride, 1.0f, 0.0f, ws.tau, nullptr, s);
    launch_prob_matrix(B, n, ld, tau, tau_bstride, eta, eta_bstride, 0.0f, beta, ws.etab, nullptr, s);
  }
  if (const int rc = launch_status("prob_matrix_kernel / pad_matrix_kernel")) return rc;
  SampleParams sp = sample_params(B, n, A, ld, 1, ws.P, Rm, noise, seed, iter, ant_gid0, routes, logp, rowsum, flags);
  sp.norm_passes = 1; sp.Lmax = n; sp.noise_steps = n - 1;
  sp.aux_vec = indegree; sp.aux_mat = ws.adj;
  sp.alpha = alpha; sp.beta = beta;
  sp.rc = rcpsp_dev(R, horizon, E, duration, resources, capacity, earliest_start, latest_start, succ_ptr, succ_idx, starts, costs);
  sp.rc.rule = rule; sp.rc.gamma = g32; sp.rc.cdir = cdir; sp.rc.csum = csum; sp.rc.taup = ws.tau; sp.rc.etab = ws.etab;
  const size_t dyn4 = 4 * rcpsp_wave_lds(n, R, horizon);
  sp.rc.fused = dyn4 <= RCPSP_LDS_PLAIN;
  const size_t dyn = sp.rc.fused ? dyn4 : 0;
  const bool lp = logp != nullptr;
  hipError_t e = vec == 1 ? launch_sample<1, 1, PROB_RCPSP>(sp, mode, lp, s, dyn)          // n <= 256: one chunk per lane
               : (vec == 2 ? launch_sample<2, 1, PROB_RCPSP>(sp, mode, lp, s, dyn) : launch_sample<4, 1, PROB_RCPSP>(sp, mode, lp, s, dyn));
  if (const int rc = launch_status(e, "rcpsp construction kernel")) return rc;
  if (sp.rc.fused) return DACO_OK;
  return launch_status(launch_schedule(sp.rc, B, n, A, routes, flags, s), "rcpsp_schedule_kernel");
}

extern "C" int daco_rcpsp_backward(void *stream, int B, int n, int A, const float *indegree, const float *adjacency,
                                   const float *tau, long tau_bstride, const float *eta, long eta_bstride, float alpha, float beta,
                                   double gamma, double c, const int64_t *routes, const float *rowsum, const float *grad_logp,
                                   float *grad_eta) {
  if (B <= 0 || n < 2 || A <= 0 || !indegree || !adjacency || !tau || !eta || !routes || !rowsum || !grad_logp || !grad_eta) {
    set_error("daco_rcpsp_backward: bad argument (B=%d n=%d A=%d)", B, n, A);
    return DACO_E_BADARG;
  }
  if (n > DACO_RCPSP_MAX_N) { set_error("daco_rcpsp_backward: n=%d exceeds %d", n, DACO_RCPSP_MAX_N); return DACO_E_TOOLARGE; }
  int rule;
  float g32, cdir, csum;
  if (!rcpsp_rule(gamma, c, &rule, &g32, &cdir, &csum)) { set_error("daco_rcpsp_backward: gamma >= 0 and 0 <= c <= 1 required"); return DACO_E_BADARG; }
  hipLaunchKernelGGL(rcpsp_backward_kernel, dim3((unsigned)(B * ((A + 3) / 4))), dim3(256), 0, (hipStream_t)stream, B, n, A, indegree,
                     adjacency, tau, tau_bstride, eta, eta_bstride, alpha, beta, rule, g32, cdir, csum, routes, rowsum, grad_logp, grad_eta);
  return launch_status("rcpsp_backward_kernel");
}

extern "C" int daco_rcpsp_track(void *stream, int B, int n, int A, const int64_t *routes, const int32_t *starts, const int32_t *costs,
                                double Q, int elitist, int alias, int min_max, float tmin, int32_t *best_cost, int32_t *best_idx,
                                int64_t *best_route, int32_t *best_schedule, int64_t *upd_routes, float *upd_weights,
                                float *clamp_min, float *clamp_max) {
  if (B <= 0 || n < 2 || A <= 0 || !routes || !costs || !best_cost || !best_idx || !best_route || !upd_routes || !upd_weights ||
      (best_schedule && !starts) || (min_max && (!clamp_min || !clamp_max))) {
    set_error("daco_rcpsp_track: bad argument (B=%d n=%d A=%d)", B, n, A);
    return DACO_E_BADARG;
  }
  hipLaunchKernelGGL(rcpsp_track_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, n, A, routes, starts, costs, Q, elitist,
                     alias, tmin, best_cost, best_idx, best_route, best_schedule, upd_routes, upd_weights,
                     min_max ? clamp_min : nullptr, min_max ? clamp_max : nullptr);
  return launch_status("rcpsp_track_kernel");
}
