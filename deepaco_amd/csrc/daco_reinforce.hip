// daco_reinforce.hip -- the REINFORCE tail between a sampler and its backward, one launch each way.
//
// Reference behaviour replaced (per train_instance of cvrp/train.ipynb:44-49 and of the train cells / files of smtwtp, sop,
// pctsp, op, bpp and mkp, for B instances at once):
//   baseline = objs.mean(); reinforce_loss = torch.sum((objs - baseline) * log_probs.sum(dim=0)) / n_ants      (minimising)
//   reinforce_loss = torch.sum((baseline - objs) * log_probs.sum(dim=0)) / n_ants                              (op, mkp)
// and autograd's way back through it.  In the batched steps this tail was about eighteen small torch launches: a row mask
// from the longest route, a masked product and sum over [B, R, A], the mean, the advantage, two more reductions, and the
// same again backward.  include/deepaco_hip.h states the arithmetic; tests/reinforce_spec.py restates it in numpy.
//
// Mapping: log_probs are [B][R][A], ants innermost, so ONE LANE PER ANT walks r upward: a row is one coalesced load per
// wavefront and the sequential order of s[a] is the lane's own program order.  One workgroup (256 lanes) per instance; an
// instance with more than 256 ants is walked in chunks of 256 ants, in order.  The rows of eight steps are fetched before
// the first of them is added (sibling_objective_kernel's scheme): the adds stay in order, the loads do not wait for each
// other.  The two sums over the ants are sequential in a by contract: the chunk's 256 values go through LDS and lane 0
// adds them in order.  No atomics, no workspace, no private arrays indexed at run time.
// The backward is elementwise: every word of [b][.][.] is written once, (g adv) / A on the live rows and +0.0f past them.
//
// Rounding: a product is rounded before it is added.  The library is built with -ffp-contract=off (csrc/Makefile); the
// pragma below says it again for this file, so that another build line cannot fuse adv * s into the running sum.
#include "daco_host.h"

#pragma clang fp contract(off)

namespace daco {

constexpr int RF_T = 256;      // lanes per workgroup = ants per chunk
constexpr int RF_U = 8;        // rows fetched ahead

__global__ void __launch_bounds__(RF_T)
reinforce_kernel(int R, int A, const float *__restrict__ obj, const float *__restrict__ log_probs,
                 const int32_t *__restrict__ lens, int d, float sign, float *__restrict__ loss, float *__restrict__ adv,
                 int32_t *__restrict__ live_out) {
  __shared__ float part[RF_T];
  __shared__ int wmax[RF_T / 64];
  __shared__ float mean_sh;
  const int b = blockIdx.x, tid = threadIdx.x;
  const float *o = obj + (size_t)b * A;
  const float *lp = log_probs + (size_t)b * R * A;

  // ---- live rows: the longest ant's draws
  int live = R;
  if (lens) {
    int mx = INT32_MIN;
    for (int a = tid; a < A; a += RF_T) mx = max(mx, lens[(size_t)b * A + a]);
#pragma unroll
    for (int off = 32; off; off >>= 1) mx = max(mx, __shfl_xor(mx, off, 64));
    if ((tid & 63) == 0) wmax[tid >> 6] = mx;
    __syncthreads();
    mx = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
    const long l = (long)mx - (long)d;
    live = l < 0 ? 0 : (l > R ? R : (int)l);
  }

  // ---- baseline: sum_a obj, a ascending, then / A
  float acc = 0.0f;
  for (int a0 = 0; a0 < A; a0 += RF_T) {
    const int cnt = min(RF_T, A - a0);
    if (tid < cnt) part[tid] = o[a0 + tid];
    __syncthreads();
    if (tid == 0)
      for (int i = 0; i < cnt; ++i) acc = acc + part[i];
    __syncthreads();
  }
  if (tid == 0) mean_sh = acc / (float)A;
  __syncthreads();
  const float mean = mean_sh;

  // ---- per ant: s = sum of the live rows (r ascending), adv; per instance: sum_a adv * s (a ascending)
  float lacc = 0.0f;
  for (int a0 = 0; a0 < A; a0 += RF_T) {
    const int cnt = min(RF_T, A - a0);
    if (tid < cnt) {
      const int a = a0 + tid;
      const float *p = lp + a;
      float s = 0.0f;
      for (int r0 = 0; r0 < live; r0 += RF_U) {
        float v[RF_U];
#pragma unroll
        for (int j = 0; j < RF_U; ++j) v[j] = r0 + j < live ? p[(size_t)(r0 + j) * A] : 0.0f;
#pragma unroll
        for (int j = 0; j < RF_U; ++j) {
          if (r0 + j >= live) break;
          s = s + v[j];
        }
      }
      const float ad = sign * (o[a] - mean);
      adv[(size_t)b * A + a] = ad;
      part[tid] = ad * s;
    }
    __syncthreads();
    if (tid == 0)
      for (int i = 0; i < cnt; ++i) lacc = lacc + part[i];
    __syncthreads();
  }
  if (tid == 0) {
    loss[b] = lacc / (float)A;
    live_out[b] = live;
  }
}

// grid (B, slabs): a workgroup owns a contiguous run of instance b's R A words
__global__ void __launch_bounds__(RF_T)
reinforce_backward_kernel(int R, int A, const float *__restrict__ g, const float *__restrict__ adv,
                          const int32_t *__restrict__ live, float *__restrict__ grad) {
  const int b = blockIdx.x;
  const size_t total = (size_t)R * A;
  const size_t per = (total + gridDim.y - 1) / gridDim.y;
  const size_t lo = (size_t)blockIdx.y * per;
  const size_t hi = lo + per < total ? lo + per : total;
  int lv = live[b];
  lv = lv < 0 ? 0 : (lv > R ? R : lv);
  const size_t n_live = (size_t)lv * A;
  const float gb = g[b], fA = (float)A;
  const float *ad = adv + (size_t)b * A;
  float *out = grad + (size_t)b * total;
  // the ant of word i is i % A: kept by steps of 256 % A, so the loop holds no 64-bit division
  const unsigned uA = (unsigned)A, step = (unsigned)RF_T % uA;
  unsigned a = (unsigned)((lo + threadIdx.x) % (size_t)A);
  for (size_t i = lo + threadIdx.x; i < hi; i += RF_T) {
    out[i] = i < n_live ? (gb * ad[a]) / fA : 0.0f;
    a += step;
    if (a >= uA) a -= uA;
  }
}

}  // namespace daco

using namespace daco;

extern "C" long daco_reinforce(void *stream, int B, int R, int A, const float *obj, const float *log_probs, const int32_t *lens,
                               int d, int sign, float *loss, float *adv, int32_t *live) {
  if (B <= 0 || R <= 0 || A <= 0 || d < 0 || (sign != 1 && sign != -1)) {
    set_error("daco_reinforce: bad argument (B=%d R=%d A=%d d=%d sign=%d)", B, R, A, d, sign);
    return DACO_E_BADARG;
  }
  if (!obj || !log_probs || !loss || !adv || !live) {
    set_error("daco_reinforce: bad argument (a null pointer: obj, log_probs, loss, adv and live are required)");
    return DACO_E_BADARG;
  }
  hipLaunchKernelGGL(reinforce_kernel, dim3((unsigned)B), dim3(RF_T), 0, (hipStream_t)stream, R, A, obj, log_probs, lens, d,
                     (float)sign, loss, adv, live);
  return launch_status("reinforce_kernel");
}

extern "C" long daco_reinforce_backward(void *stream, int B, int R, int A, const float *g, const float *adv, const int32_t *live,
                                        float *grad_log_probs) {
  if (B <= 0 || R <= 0 || A <= 0) {
    set_error("daco_reinforce_backward: bad argument (B=%d R=%d A=%d)", B, R, A);
    return DACO_E_BADARG;
  }
  if (!g || !adv || !live || !grad_log_probs) {
    set_error("daco_reinforce_backward: bad argument (a null pointer: g, adv, live and grad_log_probs are required)");
    return DACO_E_BADARG;
  }
  // slabs of at least 4096 words, at most 64 per instance and 2048 workgroups in all
  const size_t total = (size_t)R * A;
  size_t slabs = (total + 4095) / 4096;
  const size_t cap = (size_t)B >= 2048 ? 1 : 2048 / (size_t)B;
  if (slabs > 64) slabs = 64;
  if (slabs > cap) slabs = cap;
  if (slabs < 1) slabs = 1;
  hipLaunchKernelGGL(reinforce_backward_kernel, dim3((unsigned)B, (unsigned)slabs), dim3(RF_T), 0, (hipStream_t)stream, R, A, g,
                     adv, live, grad_log_probs);
  return launch_status("reinforce_backward_kernel");
}
