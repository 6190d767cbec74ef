// Shared device helpers for the trlx_amd gfx950 kernels.
//
// Written natively for CDNA4 (wave64, 32-bank LDS, MFMA) per
// /opt/skills/guides/cdna_hip_programming.md — no CUDA-compat shims.
#pragma once

#include <hip/hip_runtime.h>

#define WAVE 64
#define DEV __device__ __forceinline__

typedef __attribute__((ext_vector_type(2))) short short2v;
typedef __attribute__((ext_vector_type(4))) short short4v;
typedef __attribute__((ext_vector_type(8))) short short8v;
typedef __attribute__((ext_vector_type(4))) float float4v;

// ---- bf16 <-> f32 -----------------------------------------------------------

DEV float bf2f(unsigned short u) {
  union {
    float f;
    unsigned int i;
  } x;
  x.i = ((unsigned int)u) << 16;
  return x.f;
}

DEV unsigned short f2bf(float f) {
  union {
    float f;
    unsigned int i;
  } x;
  x.f = f;
  if ((x.i & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;  // NaN
  unsigned int lsb = (x.i >> 16) & 1u;
  x.i += 0x7fffu + lsb;  // round to nearest even
  return (unsigned short)(x.i >> 16);
}

// ---- scalar load/store traits ----------------------------------------------

template <typename T>
struct ScalarIO;

template <>
struct ScalarIO<float> {
  DEV static float load(const float* p) { return *p; }
  DEV static void store(float* p, float v) { *p = v; }
};

struct bf16_t {
  unsigned short u;
};

template <>
struct ScalarIO<bf16_t> {
  DEV static float load(const bf16_t* p) { return bf2f(p->u); }
  DEV static void store(bf16_t* p, float v) { p->u = f2bf(v); }
};

// vectorized 8-element load of T into float[8]
template <typename T>
DEV void load8(const T* p, float* out);

template <>
DEV void load8<float>(const float* p, float* out) {
  const float4v* v = reinterpret_cast<const float4v*>(p);
  float4v a = v[0], b = v[1];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    out[i] = a[i];
    out[i + 4] = b[i];
  }
}

template <>
DEV void load8<bf16_t>(const bf16_t* p, float* out) {
  short8v s = *reinterpret_cast<const short8v*>(p);
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = bf2f((unsigned short)s[i]);
}

template <typename T>
DEV void store8(T* p, const float* in);

template <>
DEV void store8<float>(float* p, const float* in) {
  float4v a, b;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    a[i] = in[i];
    b[i] = in[i + 4];
  }
  float4v* v = reinterpret_cast<float4v*>(p);
  v[0] = a;
  v[1] = b;
}

template <>
DEV void store8<bf16_t>(bf16_t* p, const float* in) {
  short8v s;
#pragma unroll
  for (int i = 0; i < 8; ++i) s[i] = (short)f2bf(in[i]);
  *reinterpret_cast<short8v*>(p) = s;
}

// ---- wave / block reductions ------------------------------------------------

DEV float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

DEV float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}

// block-level sum over NWAVES waves (block size = NWAVES*64); buf: NWAVES floats
template <int NWAVES>
DEV float block_sum(float v, float* buf) {
  v = wave_sum(v);
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (lane == 0) buf[wid] = v;
  __syncthreads();
  float r = 0.f;
#pragma unroll
  for (int i = 0; i < NWAVES; ++i) r += buf[i];
  __syncthreads();
  return r;
}

template <int NWAVES>
DEV float block_max(float v, float* buf) {
  v = wave_max(v);
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (lane == 0) buf[wid] = v;
  __syncthreads();
  float r = -INFINITY;
#pragma unroll
  for (int i = 0; i < NWAVES; ++i) r = fmaxf(r, buf[i]);
  __syncthreads();
  return r;
}

// online-logsumexp pair (m = running max, s = sum of exp(x - m))
struct MS {
  float m, s;
};

DEV MS ms_combine(MS a, MS b) {
  MS r;
  r.m = fmaxf(a.m, b.m);
  // exp(-inf - -inf) guard: if both -inf, s stays 0
  float ea = (a.m == -INFINITY) ? 0.f : __expf(a.m - r.m);
  float eb = (b.m == -INFINITY) ? 0.f : __expf(b.m - r.m);
  r.s = a.s * ea + b.s * eb;
  return r;
}

DEV MS wave_ms(MS v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    MS o;
    o.m = __shfl_xor(v.m, off);
    o.s = __shfl_xor(v.s, off);
    v = ms_combine(v, o);
  }
  return v;
}

// ---- ALiBi -------------------------------------------------------------------

// scaled score + slope * (key - key_start) in fp32 (Bloom: the bias depends
// on the key position only).  The flash forward, both flash backward kernels
// and the decode kernels all call this one helper: the backward recomputes P
// from the saved logsumexp, so the biased score must round identically there
// (explicit fma, int->float conversion before the multiply).
DEV float alibi_score(float score, float slope, int key, int kstart) {
  return __builtin_fmaf(slope, (float)(key - kstart), score);
}

// ---- T5 relative-position bias ------------------------------------------------

// scaled score + bias_row[key - qpos + bias_zero] in fp32.  The T5 bias depends
// on key - query position only, so one head's [Tq, Tk] bias is a Toeplitz
// vector bias_row[0..L) with relative position 0 at index bias_zero
// (ops.t5_rel_bias).  The flash forward and both flash backward kernels call
// this one helper, so the backward's recomputed P matches the saved logsumexp.
// Lanes that stand for rows >= Tq or keys >= Tk (masked later) compute an
// index outside [0, L): the index is clamped BEFORE the load, never after.
DEV float rel_bias_score(float score, const float* __restrict__ bias_row, int L, int key,
                         int qpos, int bias_zero) {
  const int idx = min(max(key - qpos + bias_zero, 0), L - 1);
  return score + bias_row[idx];
}

// The seq2seq kernel arguments travel as a trailing parameter PACK: the causal
// instantiations have an empty pack and so exactly the argument list (and
// kernarg segment, which steers how the compiler merges the scalar argument
// loads) they had before these modes existed.
struct S2SView {
  const float* rel_bias;          // [Hq, bias_len]
  int bias_len, bias_zero;
  const unsigned char* key_mask;  // [B, Tk]
  int Tk;                         // backward only: keys when Tq != Tk
};
// A kernel checks its pack with s2s_pack_ok: empty exactly when no seq2seq flag
// is set, otherwise the 4 (forward) or 5 (backward) arguments below, so a
// mismatched launch is a compile error and never a silently null view.
constexpr bool s2s_pack_ok(bool any_flag, int pack_size, int expected) {
  return any_flag ? pack_size == expected : pack_size == 0;
}
DEV S2SView s2s_view() { return {nullptr, 0, 0, nullptr, 0}; }
DEV S2SView s2s_view(const float* rel_bias, int bias_len, int bias_zero,
                     const unsigned char* key_mask, int Tk = 0) {
  return {rel_bias, bias_len, bias_zero, key_mask, Tk};
}

// ---- counter-based RNG (splitmix64) -----------------------------------------

DEV unsigned long long splitmix64(unsigned long long z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// uniform in (0, 1): 24 high bits, never exactly 0
DEV float rng_uniform(unsigned long long seed, unsigned long long a, unsigned long long b) {
  unsigned long long h = splitmix64(seed ^ splitmix64(a ^ splitmix64(b)));
  return ((h >> 40) + 1.0f) * (1.0f / 16777217.0f);
}

inline unsigned long long splitmix64_host(unsigned long long z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// host side: validate an optional ALiBi slope vector (fp32, contiguous, same
// device as `like`, one slope per QUERY head) and return its pointer, or null
// when no bias was given.  (every kernel file includes ATen before common.h)
inline const float* alibi_slopes_ptr(const c10::optional<at::Tensor>& slopes,
                                     const at::Tensor& like, long num_q_heads,
                                     const char* op) {
  if (!slopes.has_value()) return nullptr;
  TORCH_CHECK(slopes->dtype() == at::kFloat && slopes->is_contiguous(), op,
              ": alibi_slopes must be contiguous fp32");
  TORCH_CHECK(slopes->device() == like.device(), op,
              ": alibi_slopes must live on the same device as the inputs");
  TORCH_CHECK(slopes->numel() == num_q_heads, op, ": alibi_slopes needs one slope per query head (",
              num_q_heads, "), got ", slopes->numel());
  return slopes->data_ptr<float>();
}

// host side: the seq2seq (T5) modes of the flash kernels — non-causal,
// Toeplitz relative bias, arbitrary key mask.  Validates the optional inputs
// and returns raw pointers (null = mode off).  `any` says whether a seq2seq
// instantiation is needed at all; those exist at head dims 64 and 128 only.
struct Seq2SeqArgs {
  const float* rel_bias = nullptr;  // [Hq, L] fp32
  int bias_len = 0;                 // L
  int bias_zero = 0;                // index of relative position 0
  const unsigned char* key_mask = nullptr;  // [B, Tk], nonzero = visible
  bool any = false;
};

inline Seq2SeqArgs seq2seq_args(const c10::optional<at::Tensor>& rel_bias, long bias_zero,
                                const c10::optional<at::Tensor>& key_mask, bool causal,
                                bool has_key_starts, bool has_alibi, const at::Tensor& like,
                                long B, long num_q_heads, long Tq, long Tk, long start_pos,
                                long D, const char* op) {
  Seq2SeqArgs a;
  if (rel_bias.has_value()) {
    TORCH_CHECK(!has_alibi, op, ": rel_bias and alibi_slopes are mutually exclusive");
    TORCH_CHECK(rel_bias->dtype() == at::kFloat && rel_bias->is_contiguous() &&
                    rel_bias->dim() == 2 && rel_bias->size(0) == num_q_heads,
                op, ": rel_bias must be contiguous fp32 [Hq, L]");
    TORCH_CHECK(rel_bias->device() == like.device(), op,
                ": rel_bias must live on the same device as the inputs");
    const long L = rel_bias->size(1);
    TORCH_CHECK(bias_zero - (start_pos + Tq - 1) >= 0 && bias_zero + Tk - 1 < L, op,
                ": rel_bias [Hq, ", L, "] with bias_zero ", bias_zero,
                " does not cover queries ", start_pos, "..", start_pos + Tq - 1, " x keys 0..",
                Tk - 1);
    a.rel_bias = rel_bias->data_ptr<float>();
    a.bias_len = (int)L;
    a.bias_zero = (int)bias_zero;
  }
  if (key_mask.has_value()) {
    TORCH_CHECK(!has_key_starts, op, ": key_mask and key_starts are mutually exclusive");
    TORCH_CHECK(key_mask->dtype() == at::kByte && key_mask->is_contiguous() &&
                    key_mask->dim() == 2 && key_mask->size(0) == B && key_mask->size(1) == Tk,
                op, ": key_mask must be contiguous uint8 [B, Tk]");
    TORCH_CHECK(key_mask->device() == like.device(), op,
                ": key_mask must live on the same device as the inputs");
    TORCH_CHECK(Tk > 0, op, ": key_mask needs at least one key");
    a.key_mask = key_mask->data_ptr<unsigned char>();
  }
  a.any = a.rel_bias != nullptr || a.key_mask != nullptr || !causal;
  if (a.any) {
    TORCH_CHECK(!has_alibi, op, ": key_mask / non-causal attention do not combine with alibi_slopes");
    TORCH_CHECK(D == 64 || D == 128, op,
                ": rel_bias / key_mask / non-causal attention need head dim 64 or 128, got ", D);
  }
  return a;
}

#define HIP_CHECK_LAST()                                          \
  do {                                                             \
    hipError_t e = hipGetLastError();                              \
    TORCH_CHECK(e == hipSuccess, "HIP error: ", hipGetErrorString(e)); \
  } while (0)
