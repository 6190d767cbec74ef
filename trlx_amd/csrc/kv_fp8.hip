// fp8 KV cache, the quantizing store: new K and V rows [B, Hkv, T, D] (bf16)
// become OCP e4m3 codes plus one fp32 scale per (batch row, KV head, key).
//
// Cache format (public: docs/kernels.md; ops/reference.py kv_quantize_fp8 is the
// bit-level definition and this kernel reproduces every code and scale of it):
//   k8, v8            uint8 [B, Hkv, S, D]   e4m3 codes (the code space of adamw8
//                                            and torch.float8_e4m3fn)
//   k_scale, v_scale  fp32  [B, Hkv, S]
//   one row x[0:D]:   scale = absmax(x) / 448 (one fp32 division);
//                     code[d] = e4m3_rne(clamp(x[d] / scale, +-448)), so no NaN
//                     code is ever produced; an all-zero row: scale 0, codes 0;
//                     x ~ e4m3(code) * scale.
// Scales are per KEY: the cache is append-only, so no stored key is ever
// requantized and there is no calibration pass.
//
// Plan.  One launch quantizes K and V: 2 * B * Hkv * T rows, LPR = D/8 lanes to a
// row.  A lane loads 16 B (8 bf16); the row absmax is log2(LPR) xor-shuffles
// inside the lane group (the offsets stay below LPR, so they never leave it);
// v_cvt_pk_fp8_f32 encodes two values per instruction; the lane stores 8 B of
// codes and lane 0 of the group the scale.  A wave covers 64 / LPR rows per trip
// and rows are walked grid-stride; the trip count depends on blockIdx only, so
// every lane takes part in every shuffle.  A lane group past the last row
// re-reads the last row and stores nothing.
//
// Token t of the input goes to cache position start + t, where start is a host
// int (prefill), a device int64 scalar (the captured decode step's cache_idx) or
// a device int64 per batch row.  The position is clamped into [0, S) before the
// store.  No LDS, no atomics, and in the device-index forms no host value that
// changes between steps: the launch captures into the decode hipGraph.
//
// Input batch / head / token strides are arbitrary (the D stride is 1), so the
// tensors qkv_prep returns, or slices of a fused qkv tensor, are read in place.
// VEC = false is the same body with element-wise accesses, taken when a base
// pointer or a stride breaks the 16 B (codes: 8 B) alignment.
//
// FMA contraction is off for the file, as in adamw8.hip: the definition is a
// sequence of single fp32 roundings.
#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>

#include "attn_host.h"
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int KS_BLOCK = 256;
constexpr int KS_EPL = 8;  // elements per lane
constexpr int KS_BLOCKS_PER_CU = 8;
constexpr float KS_E4M3_MAX = 448.f;

typedef __attribute__((ext_vector_type(2))) unsigned int ks_uint2;

struct KvStoreSide {
  const bf16_t* src;    // [B, Hkv, T, D] with the strides below (elements)
  long sb, sh, st;
  unsigned char* codes;  // [B, Hkv, S, D]
  float* scale;          // [B, Hkv, S]
};

template <int D, bool VEC>
__global__ __launch_bounds__(KS_BLOCK) void kv_store_fp8_kernel(
    KvStoreSide kside, KvStoreSide vside, const long* __restrict__ start_dev /* null: host */,
    int start_stride /* 0: one scalar, 1: one per batch row */, long start_host, int B, int Hkv,
    int T, int S) {
  constexpr int LPR = D / KS_EPL;          // lanes per row
  constexpr int RPB = KS_BLOCK / LPR;      // rows per block and trip
  const long side_rows = (long)B * Hkv * T;
  const long nrows = 2 * side_rows;
  const int sub = threadIdx.x % LPR;
  for (long base = (long)blockIdx.x * RPB; base < nrows; base += (long)gridDim.x * RPB) {
    const long want = base + threadIdx.x / LPR;
    const bool live = want < nrows;
    const long row = live ? want : nrows - 1;
    const bool is_v = row >= side_rows;
    const KvStoreSide& sd = is_v ? vside : kside;
    const long r = is_v ? row - side_rows : row;
    const int t = (int)(r % T);
    const int h = (int)((r / T) % Hkv);
    const int b = (int)(r / ((long)T * Hkv));

    const bf16_t* src = sd.src + b * sd.sb + h * sd.sh + t * sd.st + sub * KS_EPL;
    float x[KS_EPL];
    if constexpr (VEC) {
      load8<bf16_t>(src, x);
    } else {
#pragma unroll
      for (int j = 0; j < KS_EPL; ++j) x[j] = ScalarIO<bf16_t>::load(src + j);
    }
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < KS_EPL; ++j) amax = fmaxf(amax, fabsf(x[j]));
#pragma unroll
    for (int off = LPR / 2; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off));
    const float scale = amax / KS_E4M3_MAX;

    float y[KS_EPL];
#pragma unroll
    for (int j = 0; j < KS_EPL; ++j) {
      const float q = scale > 0.f ? x[j] / scale : 0.f;
      y[j] = fminf(fmaxf(q, -KS_E4M3_MAX), KS_E4M3_MAX);
    }
    ks_uint2 w;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      int c = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * half + 0], y[4 * half + 1], 0, false);
      c = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * half + 2], y[4 * half + 3], c, true);
      w[half] = (unsigned)c;
    }

    const long start = start_dev ? start_dev[(long)b * start_stride] : start_host;
    long pos = start + t;
    pos = pos < 0 ? 0 : (pos > S - 1 ? (long)S - 1 : pos);
    const long crow = ((long)b * Hkv + h) * S + pos;
    if (live) {
      unsigned char* dst = sd.codes + crow * D + sub * KS_EPL;
      if constexpr (VEC) {
        *reinterpret_cast<ks_uint2*>(dst) = w;
      } else {
#pragma unroll
        for (int j = 0; j < KS_EPL; ++j) dst[j] = (unsigned char)(w[j >> 2] >> (8 * (j & 3)));
      }
      if (sub == 0) sd.scale[crow] = scale;
    }
  }
}

bool ks_aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

KvStoreSide ks_side(const at::Tensor& x, at::Tensor& codes, at::Tensor& scale) {
  return {reinterpret_cast<const bf16_t*>(x.data_ptr()), x.stride(0), x.stride(1), x.stride(2),
          codes.data_ptr<uint8_t>(), scale.data_ptr<float>()};
}

bool ks_vec_ok(const KvStoreSide& s) {
  return ks_aligned(s.src, 16) && s.sb % KS_EPL == 0 && s.sh % KS_EPL == 0 &&
         s.st % KS_EPL == 0 && ks_aligned(s.codes, 8);
}

}  // namespace

// start_dev: none (start_host is the first cache position), an int64 scalar, or
// int64 [B] (one first position per batch row).
void kv_store_fp8(const at::Tensor& k, const at::Tensor& v, at::Tensor& k8, at::Tensor& k_scale,
                  at::Tensor& v8, at::Tensor& v_scale,
                  const c10::optional<at::Tensor>& start_dev, long start_host) {
  const char* op = "kv_store_fp8";
  TORCH_CHECK(k.is_cuda() && v.is_cuda() && k.dtype() == at::kBFloat16 &&
                  v.dtype() == at::kBFloat16 && k.dim() == 4 && v.sizes() == k.sizes() &&
                  k.device() == v.device(),
              op, ": k and v must be bf16 [B,Hkv,T,D] of one shape on the GPU");
  const long B = k.size(0), Hkv = k.size(1), T = k.size(2), D = k.size(3);
  TORCH_CHECK(k.stride(3) == 1 && v.stride(3) == 1, op,
              ": k and v need a unit stride over the head dim");
  for (const at::Tensor* c : {&k8, &v8})
    TORCH_CHECK(c->is_cuda() && c->device() == k.device() && c->dtype() == at::kByte &&
                    c->is_contiguous() && c->dim() == 4 && c->size(0) == B && c->size(1) == Hkv &&
                    c->size(3) == D && c->size(2) == k8.size(2),
                op, ": k8 and v8 must be contiguous uint8 [B,Hkv,S,D] on k's device");
  const long S = k8.size(2);
  for (const at::Tensor* s : {&k_scale, &v_scale})
    TORCH_CHECK(s->is_cuda() && s->device() == k.device() && s->dtype() == at::kFloat &&
                    s->is_contiguous() && s->dim() == 3 && s->size(0) == B && s->size(1) == Hkv &&
                    s->size(2) == S,
                op, ": k_scale and v_scale must be contiguous fp32 [B,Hkv,S] on k's device");
  TORCH_CHECK(S > 0 && S < (1L << 31), op, ": cache length out of range");
  const long* sdev = nullptr;
  int sstride = 0;
  if (start_dev.has_value()) {
    TORCH_CHECK(start_dev->is_cuda() && start_dev->device() == k.device() &&
                    start_dev->dtype() == at::kLong && start_dev->is_contiguous() &&
                    (start_dev->numel() == 1 || start_dev->numel() == B),
                op, ": a device start must be contiguous int64 with 1 or B elements");
    sdev = start_dev->data_ptr<long>();
    sstride = start_dev->numel() == 1 ? 0 : 1;
  } else {
    TORCH_CHECK(start_host >= 0 && start_host + T <= S, op, ": positions ", start_host, "..",
                start_host + T, " do not fit the cache length ", S);
  }
  const long nrows = 2 * B * Hkv * T;
  if (nrows == 0) return;

  const KvStoreSide ks = ks_side(k, k8, k_scale), vs = ks_side(v, v8, v_scale);
  const bool vec = ks_vec_ok(ks) && ks_vec_ok(vs);
  const long cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  auto stream = c10::hip::getCurrentHIPStream();
  dispatch_head_dim(kKvFp8HeadDims, (int)D, op, [&](auto d) {
    constexpr int kD = decltype(d)::value;
    constexpr int RPB = KS_BLOCK / (kD / KS_EPL);
    const long blocks = std::min<long>((nrows + RPB - 1) / RPB, cus * KS_BLOCKS_PER_CU);
    dispatch_bool(vec, [&](auto vc) {
      kv_store_fp8_kernel<kD, decltype(vc)::value><<<(unsigned)blocks, KS_BLOCK, 0, stream>>>(
          ks, vs, sdev, sstride, start_host, (int)B, (int)Hkv, (int)T, (int)S);
    });
  });
  HIP_CHECK_LAST();
}
