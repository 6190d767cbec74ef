// Fused clipped-surrogate PPO loss: the loss, every logged statistic and the
// gradients w.r.t. logprobs and values in ONE launch of ONE workgroup.
//
// The eager PPOConfig.loss is ~80 tiny ATen kernels over [B, R] fp32 tensors
// of a few KB each, plus ~40 more in autograd's mirror; every one of them is a
// launch and a hop in a serial dependency chain.  All statistics are
// reductions over the same elements and the gradient is an elementwise
// function of data already in registers plus 1/n, so nothing here needs more
// than one workgroup:
//
//   pass 1   n, the first-order sums, mins and maxes      -> block reduction
//   pass 2   centered second moments for the three stds (mean first, then
//            ((x - mean) * mask)^2, as get_tensor_stats does; never
//            E[x^2] - E[x]^2) and the gradient writes      -> block reduction
//   finalize thread 0 writes the loss and the 21 statistics
//
// Reductions are wave shuffles plus fixed-order sums of the per-wave partials
// in LDS: no floating-point atomics, bit-reproducible from run to run.
//
// Each elementwise formula is written in the eager code's operation order and
// FMA contraction is off for this file, so every per-element value (and so
// every comparison, tie and gradient element) rounds as the ATen kernels
// round it; only the summation order differs from eager.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include <limits>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int PPO_MAX_WAVES = 16;  // one workgroup of up to 1024 threads

// first-order sums of pass 1
enum {
  S_N = 0,    // sum(mask)
  S_VF,       // sum(max(vf_loss1, vf_loss2) * mask)
  S_VFCLIP,   // sum((vf_loss2 > vf_loss1) * mask)
  S_KL,       // sum((ratio - 1) - log_ratio)   over ALL elements
  S_PG,       // sum(max(pg_loss1, pg_loss2) * mask)
  S_PGCLIP,   // sum((pg_loss2 > pg_loss1) * mask)
  S_V,        // sum(values * mask)
  S_OV,       // sum(old_values * mask)
  S_RET,      // sum(returns * mask)
  S_VERR,     // sum(((values - returns) * mask)^2)
  S_RATIO,    // sum(ratio * mask)
  NSUM
};

// layout of the statistics vector: the key order PPOConfig.loss returns
enum {
  O_TOTAL = 0, O_POLICY, O_VALUE,
  O_V_MEAN, O_V_MIN, O_V_MAX, O_V_STD, O_V_ERR, O_V_CLIPFRAC,
  O_OV_MEAN, O_OV_MIN, O_OV_MAX, O_OV_STD,
  O_RET_MEAN, O_RET_MIN, O_RET_MAX, O_RET_STD,
  O_KL, O_PG_CLIPFRAC, O_RATIO, O_PADDING,
  NOUT
};

// a [B, R] operand addressed through its strides (in elements): the trainer
// passes slices such as logprobs[:, start:end], never copies of them
template <typename T>
struct View2 {
  const T* p;
  long s0, s1;
  DEV T at(int b, int r) const { return p[b * s0 + r * s1]; }
};

struct PPOLossArgs {
  View2<float> logprobs, values, old_logprobs, old_values, advantages, returns;
  View2<int64_t> mask;
  int B, R;
  float clip_lo, clip_hi;  // 1 -/+ cliprange
  float cliprange_value, vf_coef;
};

// everything pass 1 and pass 2 need of one element, in eager's rounding
struct Elem {
  float m;     // float(mask)
  bool on;     // mask.bool()
  float v, ov, ret, neg_adv;
  float d1, d2;          // values - returns, values_clipped - returns
  float l1, l2;          // vf_loss1, vf_loss2
  float lr, ratio, rc;   // log_ratio, ratio, clamp(ratio)
  float p1, p2;          // pg_loss1, pg_loss2
  bool v_inside, r_inside;  // clamp passes the gradient (closed interval)
};

DEV Elem load_elem(const PPOLossArgs& a, int i) {
  const int b = i / a.R, r = i - b * a.R;
  Elem e;
  const int64_t mk = a.mask.at(b, r);
  e.m = (float)mk;
  e.on = mk != 0;
  e.v = a.values.at(b, r);
  e.ov = a.old_values.at(b, r);
  e.ret = a.returns.at(b, r);
  e.neg_adv = -a.advantages.at(b, r);

  const float vlo = e.ov - a.cliprange_value, vhi = e.ov + a.cliprange_value;
  const float vc = fminf(fmaxf(e.v, vlo), vhi);
  e.v_inside = e.v >= vlo && e.v <= vhi;
  e.d1 = e.v - e.ret;
  e.d2 = vc - e.ret;
  e.l1 = e.d1 * e.d1;
  e.l2 = e.d2 * e.d2;

  e.lr = (a.logprobs.at(b, r) - a.old_logprobs.at(b, r)) * e.m;
  e.ratio = expf(e.lr);
  e.rc = fminf(fmaxf(e.ratio, a.clip_lo), a.clip_hi);
  e.r_inside = e.ratio >= a.clip_lo && e.ratio <= a.clip_hi;
  e.p1 = e.neg_adv * e.ratio;
  e.p2 = e.neg_adv * e.rc;
  return e;
}

DEV float wave_min(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off));
  return v;
}

// Block reductions of K values at once.  The xor butterfly leaves the same
// bits in every lane; lane 0 of each wave parks them in LDS and every thread
// then folds the per-wave partials in wave order.
enum class Red { Sum, Min, Max };

template <Red OP, int K>
DEV void block_reduce(float (&v)[K], float* lds, int nwaves) {
  const int wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float w = OP == Red::Sum ? wave_sum(v[k]) : OP == Red::Min ? wave_min(v[k]) : wave_max(v[k]);
    if (lane == 0) lds[k * PPO_MAX_WAVES + wid] = w;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float r = lds[k * PPO_MAX_WAVES];
    for (int w = 1; w < nwaves; ++w) {
      const float x = lds[k * PPO_MAX_WAVES + w];
      r = OP == Red::Sum ? r + x : OP == Red::Min ? fminf(r, x) : fmaxf(r, x);
    }
    v[k] = r;
  }
  __syncthreads();
}

// autograd's torch.max(a, b) backward: the whole gradient to the larger side,
// half to each on an exact tie
DEV float max_share(float self, float other) {
  return self > other ? 1.f : self == other ? 0.5f : 0.f;
}

__global__ void __launch_bounds__(1024)
ppo_loss_kernel(const PPOLossArgs a, float* __restrict__ loss, float* __restrict__ out,
                float* __restrict__ dlogprobs, float* __restrict__ dvalues) {
  __shared__ float lds[NSUM * PPO_MAX_WAVES];
  const int N = a.B * a.R;
  const int nwaves = blockDim.x / WAVE;
  const float inf = std::numeric_limits<float>::infinity();

  // ---- pass 1: n and the first-order sums, mins, maxes ----------------------
  float s[NSUM];
#pragma unroll
  for (int k = 0; k < NSUM; ++k) s[k] = 0.f;
  float mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
  for (int i = threadIdx.x; i < N; i += blockDim.x) {
    const Elem e = load_elem(a, i);
    s[S_N] += e.m;
    s[S_VF] += fmaxf(e.l1, e.l2) * e.m;
    s[S_VFCLIP] += (e.l2 > e.l1 ? 1.f : 0.f) * e.m;
    s[S_KL] += (e.ratio - 1.f) - e.lr;
    s[S_PG] += fmaxf(e.p1, e.p2) * e.m;
    s[S_PGCLIP] += (e.p2 > e.p1 ? 1.f : 0.f) * e.m;
    s[S_V] += e.v * e.m;
    s[S_OV] += e.ov * e.m;
    s[S_RET] += e.ret * e.m;
    const float ve = e.d1 * e.m;
    s[S_VERR] += ve * ve;
    s[S_RATIO] += e.ratio * e.m;
    if (e.on) {
      mn[0] = fminf(mn[0], e.v);
      mx[0] = fmaxf(mx[0], e.v);
      mn[1] = fminf(mn[1], e.ov);
      mx[1] = fmaxf(mx[1], e.ov);
      mn[2] = fminf(mn[2], e.ret);
      mx[2] = fmaxf(mx[2], e.ret);
    }
  }
  block_reduce<Red::Sum>(s, lds, nwaves);
  block_reduce<Red::Min>(mn, lds, nwaves);
  block_reduce<Red::Max>(mx, lds, nwaves);

  const float n = s[S_N];
  const float mean[3] = {s[S_V] / n, s[S_OV] / n, s[S_RET] / n};
  // the upstream gradient is 1: loss = pg_loss + vf_coef * vf_loss,
  // pg_loss = S_pg / n, vf_loss = (0.5 * S_vf) / n
  const float g_pg = 1.f / n;
  const float g_vf = (a.vf_coef / n) * 0.5f;

  // ---- pass 2: centered second moments and the gradients --------------------
  float c[3] = {0.f, 0.f, 0.f};
  for (int i = threadIdx.x; i < N; i += blockDim.x) {
    const Elem e = load_elem(a, i);
    const float cv = (e.v - mean[0]) * e.m;
    const float co = (e.ov - mean[1]) * e.m;
    const float cr = (e.ret - mean[2]) * e.m;
    c[0] += cv * cv;
    c[1] += co * co;
    c[2] += cr * cr;

    // d loss / d logprobs: max -> (p1 = -adv * ratio, p2 = -adv * clamp(ratio))
    // -> ratio = exp(log_ratio) -> log_ratio = (logprobs - old) * mask
    const float gm_pg = g_pg * e.m;
    const float gr1 = (gm_pg * max_share(e.p1, e.p2)) * e.neg_adv;
    const float gr2 = e.r_inside ? (gm_pg * max_share(e.p2, e.p1)) * e.neg_adv : 0.f;
    dlogprobs[i] = ((gr1 + gr2) * e.ratio) * e.m;

    // d loss / d values: max -> (l1 = d1^2, l2 = d2^2), d2 through the clamp
    const float gm_vf = g_vf * e.m;
    const float gv1 = (gm_vf * max_share(e.l1, e.l2)) * (2.f * e.d1);
    const float gv2 = e.v_inside ? (gm_vf * max_share(e.l2, e.l1)) * (2.f * e.d2) : 0.f;
    dvalues[i] = gv1 + gv2;
  }
  block_reduce<Red::Sum>(c, lds, nwaves);

  // ---- finalize -------------------------------------------------------------
  if (threadIdx.x == 0) {
    const float pg_loss = s[S_PG] / n;
    const float vf_loss = (0.5f * s[S_VF]) / n;
    const float total = pg_loss + a.vf_coef * vf_loss;
    const float denom = fmaxf(n - 1.f, 1.f);
    *loss = total;
    out[O_TOTAL] = total;
    out[O_POLICY] = pg_loss;
    out[O_VALUE] = vf_loss;
    out[O_V_MEAN] = mean[0];
    out[O_V_MIN] = mn[0];
    out[O_V_MAX] = mx[0];
    out[O_V_STD] = sqrtf(c[0] / denom);
    out[O_V_ERR] = s[S_VERR] / n;
    out[O_V_CLIPFRAC] = s[S_VFCLIP] / n;
    out[O_OV_MEAN] = mean[1];
    out[O_OV_MIN] = mn[1];
    out[O_OV_MAX] = mx[1];
    out[O_OV_STD] = sqrtf(c[1] / denom);
    out[O_RET_MEAN] = mean[2];
    out[O_RET_MIN] = mn[2];
    out[O_RET_MAX] = mx[2];
    out[O_RET_STD] = sqrtf(c[2] / denom);
    out[O_KL] = s[S_KL] / (float)N;
    out[O_PG_CLIPFRAC] = s[S_PGCLIP] / n;
    out[O_RATIO] = s[S_RATIO] / n;
    // ATen divides a tensor by a host scalar as a multiply by its reciprocal
    out[O_PADDING] = 1.f - n * (1.f / (float)N);
  }
}

template <typename T>
View2<T> view2(const at::Tensor& t) {
  return {t.data_ptr<T>(), (long)t.stride(0), (long)t.stride(1)};
}

}  // namespace

// -> {loss [], stats [21], grads [2, B, R]} with grads[0] = d loss / d logprobs
// and grads[1] = d loss / d values for an upstream gradient of 1
std::vector<at::Tensor> ppo_loss(const at::Tensor& logprobs, const at::Tensor& values,
                                 const at::Tensor& old_logprobs, const at::Tensor& old_values,
                                 const at::Tensor& advantages, const at::Tensor& returns,
                                 const at::Tensor& mask, double cliprange, double cliprange_value,
                                 double vf_coef) {
  TORCH_CHECK(logprobs.is_cuda() && logprobs.dim() == 2, "ppo_loss: logprobs must be a 2-d GPU tensor");
  for (const at::Tensor* t : {&logprobs, &values, &old_logprobs, &old_values, &advantages, &returns}) {
    TORCH_CHECK(t->is_cuda() && t->dtype() == at::kFloat && t->sizes() == logprobs.sizes() &&
                    t->device() == logprobs.device(),
                "ppo_loss: every float input must be fp32 [B, R] on one device");
  }
  TORCH_CHECK(mask.is_cuda() && mask.dtype() == at::kLong && mask.sizes() == logprobs.sizes() &&
                  mask.device() == logprobs.device(),
              "ppo_loss: mask must be int64 [B, R] on the inputs' device");
  const long B = logprobs.size(0), R = logprobs.size(1);
  TORCH_CHECK(B * R > 0 && B * R < std::numeric_limits<int>::max(), "ppo_loss: bad element count");
  const int N = (int)(B * R);

  auto opts = logprobs.options();
  auto loss = at::empty({}, opts);
  auto stats = at::empty({NOUT}, opts);
  auto grads = at::empty({2, B, R}, opts);

  PPOLossArgs a;
  a.logprobs = view2<float>(logprobs);
  a.values = view2<float>(values);
  a.old_logprobs = view2<float>(old_logprobs);
  a.old_values = view2<float>(old_values);
  a.advantages = view2<float>(advantages);
  a.returns = view2<float>(returns);
  a.mask = view2<int64_t>(mask);
  a.B = (int)B;
  a.R = (int)R;
  // python computes 1 -/+ cliprange in double and ATen rounds the scalar once
  a.clip_lo = (float)(1.0 - cliprange);
  a.clip_hi = (float)(1.0 + cliprange);
  a.cliprange_value = (float)cliprange_value;
  a.vf_coef = (float)vf_coef;

  const int block = std::min(1024, (N + WAVE - 1) / WAVE * WAVE);
  auto stream = c10::hip::getCurrentHIPStream();
  ppo_loss_kernel<<<1, block, 0, stream>>>(a, loss.data_ptr<float>(), stats.data_ptr<float>(),
                                           grads.data_ptr<float>(),
                                           grads.data_ptr<float>() + (size_t)N);
  HIP_CHECK_LAST();
  return {loss, stats, grads};
}
