// Per-token attention for encoder-decoder (T5) generation: the flash-decode
// loop of attn_decode.hip with the seq2seq modes of the flash kernels.
//
// One kernel template, two uses per decoder layer and token:
//   self step  (APPEND, optional RELB): the block appends its head's new K/V row
//     to the preallocated cache [B, H, S, D] at the DEVICE-side *cache_idx, then
//     attends over keys 0..pos inclusive with the Toeplitz relative-position
//     bias (common.h rel_bias_score, the flash kernels' definition);
//   cross step (optional KMASK): q [B, H, 1, D] against the prompt's K/V
//     [B, H, Tk, D] under an arbitrary uint8 key mask; masked keys are skipped
//     (never loaded), so whatever lies behind the mask cannot leak.
// Nothing about the step is a host value, so a captured graph replays it for
// every token.  T5 has no GQA: Hq == Hkv.  bf16, 16 B/lane K/V loads, one
// 256-thread block per (b, h), per-key-group online softmax merged through LDS.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include <cstdint>

#include "attn_host.h"
#include "common.h"

namespace {

constexpr int BLOCK = 256;
constexpr int NWAVES = BLOCK / WAVE;

// The mode flags are template parameters: a mode that is off leaves no
// instruction behind (its arguments are then null / 0 and never read).
template <int D, bool APPEND, bool RELB, bool KMASK>
__global__ void s2s_decode_kernel(const bf16_t* __restrict__ q,
                                  const bf16_t* __restrict__ k_new /* [B,H,D], iff APPEND */,
                                  const bf16_t* __restrict__ v_new, bf16_t* kc, bf16_t* vc,
                                  const long* __restrict__ cache_idx /* iff APPEND */,
                                  const float* __restrict__ rel_bias /* [H, L], iff RELB */,
                                  int bias_len, int bias_zero,
                                  const unsigned char* __restrict__ key_mask /* [B,S], iff KMASK */,
                                  bf16_t* __restrict__ out, int H, int S, float scale) {
  constexpr int G = D / 8;          // lanes cooperating on one key (16 B each)
  constexpr int KPW = WAVE / G;     // keys per wave per iteration
  constexpr int NPART = NWAVES * KPW;  // independent (m, s, o) partials
  static_assert(WAVE % G == 0 && D <= BLOCK, "head dim must tile a wave");

  const int b = blockIdx.x / H;
  const int h = blockIdx.x % H;
  const size_t row = (size_t)b * H + h;

  const int lane = threadIdx.x % WAVE;
  const int wid = threadIdx.x / WAVE;
  const int kgrp = lane / G;
  const int d0 = (lane % G) * 8;

  int n = S;    // keys 0..n-1 are candidates
  int pos = 0;  // the query's position (APPEND)
  if constexpr (APPEND) {
    // The host cannot check a device value: a cache index outside [0, S)
    // appends nothing and attends to nothing (the output is zeros).  `ok` is
    // block-uniform, so every thread reaches the barrier.
    const long p = *cache_idx;
    const bool ok = p >= 0 && p < (long)S;
    pos = ok ? (int)p : 0;
    n = ok ? pos + 1 : 0;
    if (ok && wid < 2 && lane < G) {  // wave 0: the K row, wave 1: the V row
      const bf16_t* src = (wid == 0 ? k_new : v_new) + row * D + lane * 8;
      bf16_t* dst = (wid == 0 ? kc : vc) + (row * S + pos) * D + lane * 8;
      *reinterpret_cast<short8v*>(dst) = *reinterpret_cast<const short8v*>(src);
    }
    // the fresh row is read back below through this CU's L1 (intra-block
    // global read-after-write, as in fused_decode_attn_kernel)
    __syncthreads();
  }

  const bf16_t* kbase = kc + row * S * D;
  const bf16_t* vbase = vc + row * S * D;
  const float* brow = RELB ? rel_bias + (size_t)h * bias_len : nullptr;
  const unsigned char* mrow = KMASK ? key_mask + (size_t)b * S : nullptr;

  float qf[8];
  load8<bf16_t>(q + row * D + d0, qf);
#pragma unroll
  for (int i = 0; i < 8; ++i) qf[i] *= scale;

  float m = -INFINITY, s = 0.f;
  float o[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = 0.f;

  for (int sbase = wid * KPW; sbase < n; sbase += NWAVES * KPW) {
    const int key = sbase + kgrp;
    bool visible = key < n;
    if constexpr (KMASK) visible = visible && mrow[visible ? key : 0] != 0;
    if (visible) {  // uniform over the G lanes of a key: the shuffles below stay inside them
      float kf[8], vf[8];
      load8<bf16_t>(kbase + (size_t)key * D + d0, kf);
      load8<bf16_t>(vbase + (size_t)key * D + d0, vf);
      float partial = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) partial += qf[i] * kf[i];
#pragma unroll
      for (int off = G / 2; off > 0; off >>= 1) partial += __shfl_xor(partial, off);
      const float score =
          RELB ? rel_bias_score(partial, brow, bias_len, key, pos, bias_zero) : partial;
      // branchless online update (first visible key: m = -inf -> corr = 0)
      const float mnew = fmaxf(m, score);
      const float corr = (m > -INFINITY) ? __expf(m - mnew) : 0.f;
      const float pw = __expf(score - mnew);
      s = s * corr + pw;
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = o[i] * corr + pw * vf[i];
      m = mnew;
    }
  }

  // merge the NPART partial accumulators via LDS
  __shared__ float ms_buf[NPART][2];
  __shared__ float o_buf[NPART][D];
  const int part = wid * KPW + kgrp;
  if (lane % G == 0) {
    ms_buf[part][0] = m;
    ms_buf[part][1] = s;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) o_buf[part][d0 + i] = o[i];
  __syncthreads();

  // final combine: thread t handles output dim t; no visible key -> zeros
  if (threadIdx.x < D) {
    float mstar = -INFINITY;
#pragma unroll
    for (int p = 0; p < NPART; ++p) mstar = fmaxf(mstar, ms_buf[p][0]);
    float sstar = 0.f, acc = 0.f;
#pragma unroll
    for (int p = 0; p < NPART; ++p) {
      const float mp = ms_buf[p][0];
      if (mp == -INFINITY) continue;
      const float w = __expf(mp - mstar);
      sstar += ms_buf[p][1] * w;
      acc += o_buf[p][threadIdx.x] * w;
    }
    const float res = (sstar > 0.f) ? acc / sstar : 0.f;
    out[row * D + threadIdx.x].u = f2bf(res);
  }
}

// host side: a bf16 tensor the kernel reads or writes with 16 B accesses
void check_bf16(const at::Tensor& t, const at::Tensor& like, const char* op, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device(), op, ": ", what,
              " must live on the same GPU as q");
  TORCH_CHECK(t.dtype() == at::kBFloat16, op, ": ", what, " must be bf16, got ", t.dtype());
  TORCH_CHECK(t.is_contiguous(), op, ": ", what, " must be contiguous");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, op, ": ", what,
              " must be 16-byte aligned");
}

bf16_t* bf16_ptr(const at::Tensor& t) { return reinterpret_cast<bf16_t*>(t.data_ptr()); }

}  // namespace

at::Tensor seq2seq_decode_attention(const at::Tensor& q, const at::Tensor& k_new,
                                    const at::Tensor& v_new, at::Tensor& k_cache,
                                    at::Tensor& v_cache, const at::Tensor& cache_idx,
                                    const c10::optional<at::Tensor>& rel_bias, long bias_zero,
                                    double scale) {
  const char* op = "seq2seq_decode_attention";
  TORCH_CHECK(q.is_cuda(), op, ": q must live on the GPU");
  TORCH_CHECK(q.dim() == 3, op, ": q must be [B, H, D]");
  TORCH_CHECK(k_cache.dim() == 4, op, ": k_cache must be [B, H, S, D]");
  const long B = q.size(0), H = q.size(1), D = q.size(2);
  const long S = k_cache.size(2);
  TORCH_CHECK(k_cache.size(1) == H, op, ": T5 attention has no grouped heads, Hq (", H,
              ") must equal Hkv (", k_cache.size(1), ")");
  TORCH_CHECK(k_cache.size(0) == B && k_cache.size(3) == D && S > 0, op,
              ": k_cache must be [B, H, S, D] with S > 0 matching q [B, H, D]");
  TORCH_CHECK(v_cache.sizes() == k_cache.sizes(), op, ": v_cache must have k_cache's shape");
  TORCH_CHECK(k_new.sizes() == q.sizes() && v_new.sizes() == q.sizes(), op,
              ": k_new and v_new must have q's shape [B, H, D]");
  check_bf16(q, q, op, "q");
  check_bf16(k_new, q, op, "k_new");
  check_bf16(v_new, q, op, "v_new");
  check_bf16(k_cache, q, op, "k_cache");
  check_bf16(v_cache, q, op, "v_cache");
  TORCH_CHECK(cache_idx.is_cuda() && cache_idx.device() == q.device() &&
                  cache_idx.dtype() == at::kLong && cache_idx.numel() == 1,
              op, ": cache_idx must be a one-element int64 tensor on the same GPU as q");
  const float* rb = nullptr;
  int L = 0;
  if (rel_bias.has_value()) {
    TORCH_CHECK(rel_bias->dtype() == at::kFloat && rel_bias->is_contiguous() &&
                    rel_bias->dim() == 2 && rel_bias->size(0) == H && rel_bias->size(1) > 0,
                op, ": rel_bias must be contiguous fp32 [H, L]");
    TORCH_CHECK(rel_bias->device() == q.device(), op,
                ": rel_bias must live on the same device as the inputs");
    L = (int)rel_bias->size(1);
    TORCH_CHECK(bias_zero >= 0 && bias_zero < L, op, ": bias_zero ", bias_zero,
                " lies outside rel_bias [H, ", L, "]");
    rb = rel_bias->data_ptr<float>();
  }
  auto out = at::empty({B, H, 1, D}, q.options());
  // an unsupported head dim is an error at B == 0 too
  if (B == 0) {
    dispatch_head_dim(kSeq2SeqDecodeHeadDims, (int)D, op, [](auto) {});
    return out;
  }
  auto stream = c10::hip::getCurrentHIPStream();
  const int grid = (int)(B * H);
  dispatch_head_dim(kSeq2SeqDecodeHeadDims, (int)D, op, [&](auto d) {
    dispatch_bool(rb != nullptr, [&](auto rl) {
      s2s_decode_kernel<decltype(d)::value, true, decltype(rl)::value, false>
          <<<grid, BLOCK, 0, stream>>>(bf16_ptr(q), bf16_ptr(k_new), bf16_ptr(v_new),
                                       bf16_ptr(k_cache), bf16_ptr(v_cache),
                                       cache_idx.data_ptr<long>(), rb, L, (int)bias_zero, nullptr,
                                       bf16_ptr(out), (int)H, (int)S, (float)scale);
    });
  });
  HIP_CHECK_LAST();
  return out;
}

at::Tensor seq2seq_cross_decode_attention(const at::Tensor& q, const at::Tensor& k,
                                          const at::Tensor& v,
                                          const c10::optional<at::Tensor>& key_mask,
                                          double scale) {
  const char* op = "seq2seq_cross_decode_attention";
  TORCH_CHECK(q.is_cuda(), op, ": q must live on the GPU");
  TORCH_CHECK(q.dim() == 4 && q.size(2) == 1, op, ": q must be [B, H, 1, D]");
  TORCH_CHECK(k.dim() == 4, op, ": k must be [B, H, Tk, D]");
  const long B = q.size(0), H = q.size(1), D = q.size(3);
  const long Tk = k.size(2);
  TORCH_CHECK(k.size(1) == H, op, ": T5 attention has no grouped heads, Hq (", H,
              ") must equal Hkv (", k.size(1), ")");
  TORCH_CHECK(k.size(0) == B && k.size(3) == D && Tk > 0, op,
              ": k must be [B, H, Tk, D] with Tk > 0 matching q [B, H, 1, D]");
  TORCH_CHECK(v.sizes() == k.sizes(), op, ": v must have k's shape");
  check_bf16(q, q, op, "q");
  check_bf16(k, q, op, "k");
  check_bf16(v, q, op, "v");
  const unsigned char* km = nullptr;
  if (key_mask.has_value()) {
    TORCH_CHECK(key_mask->dtype() == at::kByte && key_mask->is_contiguous() &&
                    key_mask->dim() == 2 && key_mask->size(0) == B && key_mask->size(1) == Tk,
                op, ": key_mask must be contiguous uint8 [B, Tk]");
    TORCH_CHECK(key_mask->device() == q.device(), op,
                ": key_mask must live on the same device as the inputs");
    km = key_mask->data_ptr<unsigned char>();
  }
  auto out = at::empty_like(q);
  if (B == 0) {
    dispatch_head_dim(kSeq2SeqDecodeHeadDims, (int)D, op, [](auto) {});
    return out;
  }
  auto stream = c10::hip::getCurrentHIPStream();
  const int grid = (int)(B * H);
  dispatch_head_dim(kSeq2SeqDecodeHeadDims, (int)D, op, [&](auto d) {
    dispatch_bool(km != nullptr, [&](auto mk) {
      s2s_decode_kernel<decltype(d)::value, false, false, decltype(mk)::value>
          <<<grid, BLOCK, 0, stream>>>(bf16_ptr(q), nullptr, nullptr, bf16_ptr(k), bf16_ptr(v),
                                       nullptr, nullptr, 0, 0, km, bf16_ptr(out), (int)H, (int)Tk,
                                       (float)scale);
    });
  });
  HIP_CHECK_LAST();
  return out;
}
