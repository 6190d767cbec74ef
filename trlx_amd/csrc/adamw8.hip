// 8-bit AdamW over flat parameter arenas: the step of adamw.hip with the two
// moments carried as blockwise-scaled OCP e4m3 bytes (6 + 1/32 B of optimizer
// state per parameter instead of 12).
//
// State format (public: docs/kernels.md, ops/reference.py adamw8_step is the
// bit-level definition).  Per arena or ZeRO shard of n elements, quantization
// block QB = 256 consecutive elements, nb = ceil(n / 256):
//   master  fp32 [n]   as in adamw.hip (fp32 params without ZeRO: p itself)
//   m8      uint8 [n], m_scale fp32 [nb]:  m = e4m3(m8) * m_scale[i / 256],
//           m_scale = absmax_block(m) * (1/448); encode = round-to-nearest-even
//           of m / m_scale clamped to +-448; an all-zero block: scale 0, codes 0
//   u8      uint8 [n], u_scale fp32 [nb]:  u = sqrt(v) >= 0, scaled like m, which
//           halves the exponent range a block has to fit into e4m3.  Encode is
//           STOCHASTIC rounding in plain arithmetic:
//             y = min(u / u_scale, 448), e = max(floor(log2 y), -6) (exponent
//             bits), step = 2^(e-3), q = min(floor(y / step + r) * step, 448),
//             which is an e4m3 value, so the hardware convert encodes it exactly
//             (the min: the fp32 sum y / step + r can round 14 + r up to 15);
//             r = (h >> 40) * 2^-24, h = splitmix64(key ^ splitmix64(idx)),
//             key = splitmix64(seed ^ 0x9e3779b97f4a7c15 * step_count),
//             idx = index_base + i: the element's index in the unsharded arena.
//           v moves 0.1 % per step against a 6-12 % grid: the fp32 scale carries
//           the uniform decay, the unbiased rounding carries the rest.
// Step per element, fp32, in this order, FMA contraction off for the file:
//   g = grad * grad_scale;  m' = b1 m + (1-b1) g;  v' = b2 (u u) + (1-b2) (g g)
//   w -= (lr wd) w;  w -= lr (m'/bc1) / (sqrt(v'/bc2) + eps);  u' = sqrt(v')
// The update uses this step's fp32 m', v': only the carried state is quantized.
//
// Plan (a pure stream: 16 B moved per bf16 parameter against adamw.hip's 28):
//  - A lane holds 8 consecutive elements: one 16 B grad load (bf16), two 16 B
//    master loads, one 8 B load each of m8 and u8, stores of the same widths and
//    one 16 B param store.  32 lanes are one quantization block, a wave owns two
//    per trip, a 256-thread block a tile of 2048 elements; tiles are walked
//    grid-stride by grid = min(tiles, 8 blocks per CU).
//  - A wave owns whole quantization blocks, so the two absmax reductions are 5
//    xor-shuffles over its 32-lane half: no LDS, no barrier, no atomics, no
//    second pass for the scales.
//  - Every load of a trip is issued before the first use, unconditionally: a
//    lane whose vector does not lie wholly below n loads vector 0 instead and
//    stores nothing.  The one lane of the arena that straddles n re-reads its
//    elements one by one (index clamped to n - 1) and stores them one by one.
//    Elements past n enter the absmax as 0, so a short tail block is scaled by
//    its real elements only.
//  - VEC = false is the same body with element-wise accesses throughout: for
//    n < 8 and for bases that are not 16 B (codes: 8 B) aligned, as a ZeRO
//    shard offset into a bf16 arena can make p and g.
//  - Decode and encode are v_cvt_pk_f32_fp8 / v_cvt_pk_fp8_f32, two values per
//    instruction; no codebook, no lookup.
// Resource usage and timings: profiles/adamw8_notes.md.
#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>

#include <cmath>

#include "common.h"
#include "dispatch.h"

#pragma clang fp contract(off)

namespace {

constexpr int BLOCK = 256;
constexpr int EPL = 8;             // elements per lane
constexpr int QB = 256;            // quantization block = 32 lanes
constexpr int TILE = BLOCK * EPL;  // ops.ADAMW8_TILE is the same number
constexpr int BLOCKS_PER_CU = 8;   // ops.ADAMW8_BLOCKS_PER_CU
constexpr float E4M3_MAX = 448.f;
constexpr float INV_E4M3_MAX = 1.f / 448.f;

typedef __attribute__((ext_vector_type(2))) float float2v;
typedef __attribute__((ext_vector_type(2))) unsigned int uint2v;

// element i of the lane, or the last element of the arena where i lies past it
DEV long clamped(long i, long n) { return i < n ? i : n - 1; }

template <typename T, bool VEC>
DEV void load_lane(const T* __restrict__ src, long vbase, long base, long n, float* out) {
  if constexpr (VEC) {
    load8<T>(src + vbase, out);
  } else {
#pragma unroll
    for (int j = 0; j < EPL; ++j) out[j] = ScalarIO<T>::load(src + clamped(base + j, n));
  }
}

DEV uint2v load_codes_scalar(const unsigned char* __restrict__ src, long base, long n) {
  uint2v w = {0u, 0u};
#pragma unroll
  for (int j = 0; j < EPL; ++j) w[j >> 2] |= (unsigned)src[clamped(base + j, n)] << (8 * (j & 3));
  return w;
}

template <bool VEC>
DEV uint2v load_codes(const unsigned char* __restrict__ src, long vbase, long base, long n) {
  if constexpr (VEC) return *reinterpret_cast<const uint2v*>(src + vbase);
  else return load_codes_scalar(src, base, n);
}

// 8 e4m3 bytes -> 8 floats
DEV void decode8(uint2v w, float* out) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float2v lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[h], false);
    const float2v hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[h], true);
    out[4 * h + 0] = lo[0];
    out[4 * h + 1] = lo[1];
    out[4 * h + 2] = hi[0];
    out[4 * h + 3] = hi[1];
  }
}

// 8 floats (|y| <= 448) -> 8 e4m3 bytes, round-to-nearest-even
DEV uint2v encode8(const float* y) {
  uint2v w;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    int r = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * h + 0], y[4 * h + 1], 0, false);
    r = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * h + 2], y[4 * h + 3], r, true);
    w[h] = (unsigned)r;
  }
  return w;
}

// max over the lane's 32-lane half: the xor offsets below 32 never leave it
DEV float half_wave_max(float v) {
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}

// y in [0, 448] rounded down or up to the e4m3 grid with P(up) = the fraction.
// y / step + r is itself rounded to fp32 (ulp 2^-20 in [8, 16)), so an r within
// 2^-21 of 1 carries a y ON the grid one step up: into the next binade, which is
// an e4m3 value, except from 448 (every block's absmax) to 480, which is not
// and would encode as NaN.  Hence the min with 448.
DEV float stochastic_round(float y, unsigned long long key, unsigned long long idx) {
  const int e = max((int)(__float_as_uint(y) >> 23) - 127, -6);
  const float inv_step = __uint_as_float((unsigned)(130 - e) << 23);  // 2^(3-e)
  const float step = __uint_as_float((unsigned)(124 + e) << 23);      // 2^(e-3)
  const unsigned long long h = splitmix64(key ^ splitmix64(idx));
  const float r = (float)(unsigned)(h >> 40) * 0x1p-24f;
  return fminf(floorf(y * inv_step + r) * step, E4M3_MAX);
}

template <typename T>
DEV void store_lane(T* __restrict__ dst, long base, long n, bool full, bool vec, const float* v) {
  if (vec && full) {
    store8<T>(dst + base, v);
  } else {
#pragma unroll
    for (int j = 0; j < EPL; ++j)
      if (base + j < n) ScalarIO<T>::store(dst + base + j, v[j]);
  }
}

DEV void store_codes(unsigned char* __restrict__ dst, long base, long n, bool full, bool vec,
                     uint2v w) {
  if (vec && full) {
    *reinterpret_cast<uint2v*>(dst + base) = w;
  } else {
#pragma unroll
    for (int j = 0; j < EPL; ++j)
      if (base + j < n) dst[base + j] = (unsigned char)(w[j >> 2] >> (8 * (j & 3)));
  }
}

struct Adamw8Args {
  float lr, b1, omb1, b2, omb2, eps, lrwd, bc1, bc2, gscale;
  unsigned long long key, index_base;
};

// PT: parameter storage type, G: gradient type (as adamw_kernel).  p is null
// where the master IS the parameter arena (fp32 params without ZeRO).
template <typename PT, typename G, bool VEC>
__global__ __launch_bounds__(BLOCK) void adamw8_kernel(
    PT* __restrict__ p, float* __restrict__ master, const G* __restrict__ g,
    unsigned char* __restrict__ m8, float* __restrict__ m_scale, unsigned char* __restrict__ u8,
    float* __restrict__ u_scale, long n, Adamw8Args a) {
  const long stride = (long)gridDim.x * TILE;
  // the trip count depends on blockIdx only: every lane of a wave takes part in
  // every shuffle
  for (long tile = (long)blockIdx.x * TILE; tile < n; tile += stride) {
    const long base = tile + (long)threadIdx.x * EPL;
    const bool full = base + EPL <= n;
    const bool partial = !full && base < n;
    const long vbase = full ? base : 0;
    const long qb = clamped(base, n) / QB;

    float gv[EPL], w[EPL], mv[EPL], uv[EPL];
    load_lane<G, VEC>(g, vbase, base, n, gv);
    load_lane<float, VEC>(master, vbase, base, n, w);
    uint2v mc = load_codes<VEC>(m8, vbase, base, n);
    uint2v uc = load_codes<VEC>(u8, vbase, base, n);
    // A lane at or past n has loaded other lanes' data (vector 0, the last
    // block's scales), which another wave may be storing in this same launch:
    // those values are never used, its m', u' are zeroed and it stores nothing.
    const float ms = m_scale[qb], us = u_scale[qb];
    if (VEC && partial) {
      load_lane<G, false>(g, 0, base, n, gv);
      load_lane<float, false>(master, 0, base, n, w);
      mc = load_codes_scalar(m8, base, n);
      uc = load_codes_scalar(u8, base, n);
    }
    decode8(mc, mv);
    decode8(uc, uv);

    float un[EPL];
    float am = 0.f, au = 0.f;
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
      const float gi = gv[j] * a.gscale;
      const float ui = uv[j] * us;
      float mi = a.b1 * (mv[j] * ms) + a.omb1 * gi;
      const float vi = a.b2 * (ui * ui) + a.omb2 * (gi * gi);
      float wi = w[j];
      wi -= a.lrwd * wi;
      wi -= a.lr * (mi / a.bc1) / (sqrtf(vi / a.bc2) + a.eps);
      w[j] = wi;
      float uj = sqrtf(vi);
      if (base + j >= n) mi = 0.f, uj = 0.f;
      mv[j] = mi;
      un[j] = uj;
      am = fmaxf(am, fabsf(mi));
      au = fmaxf(au, uj);
    }
    const float nms = half_wave_max(am) * INV_E4M3_MAX;
    const float nus = half_wave_max(au) * INV_E4M3_MAX;

    float ym[EPL], yu[EPL];
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
      const float y = nms > 0.f ? mv[j] / nms : 0.f;
      ym[j] = fminf(fmaxf(y, -E4M3_MAX), E4M3_MAX);
      const float z = nus > 0.f ? fminf(un[j] / nus, E4M3_MAX) : 0.f;
      yu[j] = stochastic_round(z, a.key, a.index_base + (unsigned long long)(base + j));
    }
    mc = encode8(ym);
    uc = encode8(yu);

    store_lane<float>(master, base, n, full, VEC, w);
    if (p != nullptr) store_lane<PT>(p, base, n, full, VEC, w);
    store_codes(m8, base, n, full, VEC, mc);
    store_codes(u8, base, n, full, VEC, uc);
    if ((threadIdx.x & 31) == 0 && base < n) {
      m_scale[qb] = nms;
      u_scale[qb] = nus;
    }
  }
}

bool aligned(const void* ptr, uintptr_t a) { return reinterpret_cast<uintptr_t>(ptr) % a == 0; }

}  // namespace

void fused_adamw8(at::Tensor& p, at::Tensor& master, const at::Tensor& g, at::Tensor& m8,
                  at::Tensor& m_scale, at::Tensor& u8, at::Tensor& u_scale, long step, double lr,
                  double beta1, double beta2, double eps, double weight_decay, double grad_scale,
                  long seed, long index_base) {
  const char* op = "fused_adamw8";
  TORCH_CHECK(p.is_cuda() && p.is_contiguous() && master.is_contiguous() && g.is_contiguous() &&
                  m8.is_contiguous() && u8.is_contiguous() && m_scale.is_contiguous() &&
                  u_scale.is_contiguous(),
              op, ": every tensor must be contiguous and on the GPU");
  for (const at::Tensor* t : std::initializer_list<const at::Tensor*>{&master, &g, &m8, &m_scale,
                                                                      &u8, &u_scale})
    TORCH_CHECK(t->device() == p.device(), op, ": every tensor must be on p's device");
  TORCH_CHECK(master.dtype() == at::kFloat, op, ": master must be float32");
  TORCH_CHECK(m8.dtype() == at::kByte && u8.dtype() == at::kByte, op,
              ": m8 and u8 must be uint8 (e4m3 codes)");
  TORCH_CHECK(m_scale.dtype() == at::kFloat && u_scale.dtype() == at::kFloat, op,
              ": m_scale and u_scale must be float32");
  const long n = p.numel();
  const long nb = (n + QB - 1) / QB;
  TORCH_CHECK(master.numel() == n && g.numel() == n && m8.numel() == n && u8.numel() == n, op,
              ": master, g, m8 and u8 must have p's ", n, " elements");
  TORCH_CHECK(m_scale.numel() == nb && u_scale.numel() == nb, op,
              ": m_scale and u_scale must have one entry per 256 elements, ", nb);
  TORCH_CHECK(step >= 1 && index_base >= 0, op, ": step must be >= 1 and index_base >= 0");
  if (n == 0) return;

  Adamw8Args a;
  a.lr = (float)lr;
  a.b1 = (float)beta1;
  a.omb1 = 1.f - a.b1;
  a.b2 = (float)beta2;
  a.omb2 = 1.f - a.b2;
  a.eps = (float)eps;
  a.lrwd = a.lr * (float)weight_decay;
  a.bc1 = (float)(1.0 - std::pow(beta1, (double)step));
  a.bc2 = (float)(1.0 - std::pow(beta2, (double)step));
  a.gscale = (float)grad_scale;
  a.key = splitmix64_host((unsigned long long)seed ^
                          (0x9e3779b97f4a7c15ull * (unsigned long long)step));
  a.index_base = (unsigned long long)index_base;

  const long tiles = (n + TILE - 1) / TILE;
  const long cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const int grid = (int)std::min<long>(tiles, cus * BLOCKS_PER_CU);
  const bool alias = p.data_ptr() == master.data_ptr();
  TORCH_CHECK(!alias || p.dtype() == at::kFloat, op, ": only a float32 p can be its own master");
  const bool vec = n >= EPL && aligned(p.data_ptr(), 16) && aligned(master.data_ptr(), 16) &&
                   aligned(g.data_ptr(), 16) && aligned(m8.data_ptr(), 8) &&
                   aligned(u8.data_ptr(), 8);
  auto stream = c10::hip::getCurrentHIPStream();

  auto launch = [&](auto pt, auto gt) {
    using PT = decltype(pt);
    using GT = decltype(gt);
    PT* pp = alias ? nullptr : static_cast<PT*>(p.data_ptr());
    dispatch_bool(vec, [&](auto v) {
      adamw8_kernel<PT, GT, decltype(v)::value><<<grid, BLOCK, 0, stream>>>(
          pp, master.data_ptr<float>(), static_cast<const GT*>(g.data_ptr()),
          m8.data_ptr<uint8_t>(), m_scale.data_ptr<float>(), u8.data_ptr<uint8_t>(),
          u_scale.data_ptr<float>(), n, a);
    });
  };
  const bool pb = p.dtype() == at::kBFloat16, gb = g.dtype() == at::kBFloat16;
  TORCH_CHECK((pb || p.dtype() == at::kFloat) && (gb || g.dtype() == at::kFloat), op,
              ": p and g must be bfloat16 or float32");
  if (pb && gb) launch(bf16_t{}, bf16_t{});
  else if (pb) launch(bf16_t{}, float{});
  else if (gb) launch(float{}, bf16_t{});
  else launch(float{}, float{});
  HIP_CHECK_LAST();
}
