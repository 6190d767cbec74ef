// Fused LM-head GEMM + online logsumexp + label gather (SURVEY.md K1+K5;
// supersedes the single-buffered tile kernel in lm_logprobs.hip for
// H % 64 == 0).  The 256x256x64 minimum-2-phase MFMA mainloop, its LDS swizzle
// and the workgroup remap are lm_tile.h's and lm_tile_mainloop.inc's (the
// schedule is derived there);
// this file adds the label staging and the epilogue: acc -> LDS fp32 tile
// (two 128-row halves, padded stride 257), then a per-row two-pass scan (max,
// then sum-exp with 4 independent accumulator chains) by 4 threads x 64 cols
// per row.  The register-direct epilogue (per-fragment shfl_xor chains +
// predicated stores) cost 432 us of an 870 us kernel; this one ~75 us.
//
// Measured (N=5248, V=50257, H=768, MI355X): 511 us = 792 TF vs 685 us for
// hipBLASLt GEMM + fused logprob-gather (1.34x); N=1312: 157 vs 221 us
// (1.41x).  Numerics exact vs fp32 torch reference (max err 2.9e-6).
//
// Shapes: hidden [N, H] bf16 (H % 64 == 0), weight [V, H] bf16 row-major
// (NT GEMM), labels [N] i64 -> out [N] f32.  Inference-only.
#include <c10/hip/HIPStream.h>

#include "lm_tile.h"

namespace {

using namespace lm_tile;

// online-logsumexp pair (m = running max, s = sum of exp(x - m)) and its
// merge.  Not common.h's ms_combine: that one rounds differently (fmaxf and
// two exp).  The const references keep the reduce kernels' instructions
// as they were with the merge written out (by value, one compare flips).
struct MSv2 {
  float m, s;
};

DEV MSv2 ms_merge(const MSv2& a, const MSv2& o) {
  MSv2 t = a;
  if (o.m > t.m) {
    t.s = (t.m > -INFINITY ? t.s * __expf(t.m - o.m) : 0.f) + o.s;
    t.m = o.m;
  } else if (o.m > -INFINITY) {
    t.s += o.s * __expf(o.m - t.m);
  }
  return t;
}

// Dynamic LDS.  K-loop:   [ A buf0 | A buf1 | B buf0 | B buf1 | ... | labels ]
//               epilogue: [ c_lds fp32 [128][CPAD] | cpart [128][4][2] | labels ]
// c_lds overwrites the A/B buffers (time-disjoint); the labels are staged
// before the K-loop, so they sit above both.
constexpr int CPAD = 257;  // fp32 row stride: 257 % 32 == 1, so row-per-lane
                           // reads walk all banks
constexpr int CPART_OFF = 128 * CPAD * (int)sizeof(float);
constexpr int LAB_OFF = CPART_OFF + 128 * 4 * 2 * (int)sizeof(float);
constexpr int V2_LDS = AB_BYTES + 8192 + BM * (int)sizeof(long);  // 141312
static_assert(LAB_OFF >= AB_BYTES && LAB_OFF + BM * (int)sizeof(long) <= V2_LDS,
              "labels above the A/B buffers and the epilogue tile, inside the launch's LDS");

// BIAS: z = x @ w^T + bias[v] (the ILQL Q heads, linear_gather_lse_fwd).  The
// bias joins the accumulators on their way into the LDS C tile — a lane's
// four columns (one per j) are the same for every i and r, so it loads four
// floats once — and the row scan and the label gather then see z.  With
// BIAS off the pointer is never read and the kernel is the lm_head one.
template <bool BIAS>
__global__ __launch_bounds__(BLOCK) void lm_logprobs_v2_kernel(
    const bf16_t* __restrict__ hidden, const bf16_t* __restrict__ weight,
    float* __restrict__ partials,  // [nV][N][2]
    float* __restrict__ label_logit, const long* __restrict__ labels, int N, int H, int V,
    int nV, int nM,
    const float* __restrict__ bias) {  // [V], BIAS only; last, so the
                                       // other arguments keep their slots
  extern __shared__ char smem[];
  char* a_base = smem;
  char* b_base = smem + 2 * TILE_BYTES;
  float* c_lds = reinterpret_cast<float*>(smem);
  float* cpart = reinterpret_cast<float*>(smem + CPART_OFF);  // [128][4][2]
  long* lab_s = reinterpret_cast<long*>(smem + LAB_OFF);      // [256]

  const TileCoord tc = tile_coord(nV, nM);
  const int vt = tc.vt, row0 = tc.row0, col0 = tc.col0;

  const int tid = threadIdx.x;
  const int lane = tid % WAVE;
  const int wid = tid / WAVE;
  const int wave_m = wid >> 2;          // 0..1 -> rows wave_m*128
  const int wave_n = wid & 3;           // 0..3 -> cols wave_n*64

  // stage labels for this row tile
  for (int i = tid; i < BM; i += BLOCK) {
    const int n = row0 + i;
    lab_s[i] = (n < N) ? labels[n] : -1;
  }

  f32x4 acc[8][4];
#include "lm_tile_mainloop.inc"
  const int max_brow = V - 1;

  // ---- epilogue: acc -> LDS transpose (two row-halves), then a
  // cooperative per-row scan.  The register-direct version (per-row 4-step
  // shfl_xor chains + a predicated global store per fragment value) measured
  // 432 us of the 870 us kernel at N=5248 — half the runtime; this layout
  // costs ~2 LDS round-trips of the C tile and scans rows with plain
  // contiguous reads (4 threads x 64 cols per row).
  const int n_valid_cols = V - col0;    // may exceed 256 (then all valid)
  const int row_in_half = tid & 127;    // one row per lane across 2 waves-of-rows
  const int qc0 = (tid >> 7) * 64;      // this thread's column span
  float bj[4] = {0.f, 0.f, 0.f, 0.f};   // this lane's four C columns' bias
  if constexpr (BIAS) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      bj[j] = bias[min(col0 + wave_n * 64 + j * 16 + (lane & 15), max_brow)];
  }
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    __builtin_amdgcn_s_barrier();
    if (wave_m == half) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int rr = i * 16 + (lane >> 4) * 4 + r;
            const int cc = wave_n * 64 + j * 16 + (lane & 15);
            if constexpr (BIAS)
              c_lds[rr * CPAD + cc] = acc[i][j][r] + bj[j];
            else
              c_lds[rr * CPAD + cc] = acc[i][j][r];
          }
    }
    __builtin_amdgcn_s_barrier();
    const int tile_row = half * 128 + row_in_half;
    const int n = row0 + tile_row;
    const long lab = lab_s[tile_row];
    const float* row = c_lds + row_in_half * CPAD;
    const int cend = min(qc0 + 64, n_valid_cols);
    // pass 1: max (4 independent chains) + label gather
    float mx0 = -INFINITY, mx1 = -INFINITY, mx2 = -INFINITY, mx3 = -INFINITY;
    for (int c = qc0; c + 4 <= cend; c += 4) {
      mx0 = fmaxf(mx0, row[c]);
      mx1 = fmaxf(mx1, row[c + 1]);
      mx2 = fmaxf(mx2, row[c + 2]);
      mx3 = fmaxf(mx3, row[c + 3]);
    }
    for (int c = qc0 + ((cend - qc0) & ~3); c < cend; ++c) mx0 = fmaxf(mx0, row[c]);
    const float mx = fmaxf(fmaxf(mx0, mx1), fmaxf(mx2, mx3));
    if (lab >= col0 + qc0 && lab < col0 + cend && n < N)
      label_logit[n] = row[lab - col0];
    // pass 2: sum exp(v - mx), 4 independent accumulator chains
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int c = qc0; c + 4 <= cend; c += 4) {
      s0 += __expf(row[c] - mx);
      s1 += __expf(row[c + 1] - mx);
      s2 += __expf(row[c + 2] - mx);
      s3 += __expf(row[c + 3] - mx);
    }
    for (int c = qc0 + ((cend - qc0) & ~3); c < cend; ++c) s0 += __expf(row[c] - mx);
    MSv2 ms{cend > qc0 ? mx : -INFINITY, (s0 + s1) + (s2 + s3)};
    // combine the 4 spans per row (threads tid, tid+128, ... — different
    // waves, so a block barrier orders the exchange)
    cpart[(row_in_half * 4 + (tid >> 7)) * 2] = ms.m;
    cpart[(row_in_half * 4 + (tid >> 7)) * 2 + 1] = ms.s;
    __builtin_amdgcn_s_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)");
    if (tid < 128 && n < N) {
      MSv2 t{-INFINITY, 0.f};
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4)
        t = ms_merge(t, {cpart[(row_in_half * 4 + q4) * 2], cpart[(row_in_half * 4 + q4) * 2 + 1]});
      float* dst = partials + ((size_t)vt * N + n) * 2;
      dst[0] = t.m;
      dst[1] = t.s;
    }
  }
}

// SPLIT: the label value already sits in its own output (label_logit), so
// only the logsumexp is written — the two outputs of linear_gather_lse_fwd.
template <bool SPLIT>
__global__ void lm_logprobs_v2_reduce(const float* __restrict__ partials,
                                      const float* __restrict__ label_logit,
                                      float* __restrict__ out, float* __restrict__ lse_out,
                                      int N, int nV) {
  const int wpb = blockDim.x / WAVE;
  const int n = blockIdx.x * wpb + threadIdx.x / WAVE;
  if (n >= N) return;
  const int lane = threadIdx.x % WAVE;
  MSv2 ms{-INFINITY, 0.f};
  for (int t = lane; t < nV; t += WAVE) {
    const float* p = partials + ((size_t)t * N + n) * 2;
    ms = ms_merge(ms, {p[0], p[1]});
  }
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    MSv2 o;
    o.m = __shfl_xor(ms.m, d, WAVE);
    o.s = __shfl_xor(ms.s, d, WAVE);
    ms = ms_merge(ms, o);
  }
  if (lane == 0) {
    const float lse = ms.m + logf(ms.s);
    if constexpr (SPLIT) {
      lse_out[n] = lse;
    } else {
      out[n] = label_logit[n] - lse;
      if (lse_out) lse_out[n] = lse;
    }
  }
}

// One host path for both entry points: bias == nullptr is the lm_head op
// (out = label logit - lse), otherwise out = z at the label and lse apart.
std::vector<at::Tensor> launch_v2(const at::Tensor& hidden, const at::Tensor& weight,
                                  const float* bias, const at::Tensor& labels, bool want_lse) {
  const auto [N, H, V, nV, nM] = check_operands("lm_logprobs_v2", hidden, weight, labels);
  const bool split = bias != nullptr;
  auto fopt = hidden.options().dtype(at::kFloat);
  // split: the main kernel writes the label value straight into `out`
  // (zero where no tile owns the label, as label_logit below)
  auto out = split ? at::zeros({N}, fopt) : at::empty({N}, fopt);
  auto lse = want_lse ? at::empty({N}, fopt) : at::empty({0}, fopt);
  if (N == 0) return {out, lse};
  auto partials = at::empty({nV, (long)N, 2}, fopt);
  auto label_logit = split ? out : at::zeros({N}, fopt);
  auto stream = c10::hip::getCurrentHIPStream();
  if (split)
    allow_dynamic_lds<&lm_logprobs_v2_kernel<true>, V2_LDS>();
  else
    allow_dynamic_lds<&lm_logprobs_v2_kernel<false>, V2_LDS>();
  dim3 grid(nV, nM);
  auto* kern = split ? &lm_logprobs_v2_kernel<true> : &lm_logprobs_v2_kernel<false>;
  kern<<<grid, BLOCK, V2_LDS, stream>>>(
      reinterpret_cast<const bf16_t*>(hidden.data_ptr()),
      reinterpret_cast<const bf16_t*>(weight.data_ptr()), partials.data_ptr<float>(),
      label_logit.data_ptr<float>(), labels.data_ptr<long>(), N, H, V, nV, nM, bias);
  const int wpb = 256 / WAVE;
  if (split)
    lm_logprobs_v2_reduce<true><<<(N + wpb - 1) / wpb, 256, 0, stream>>>(
        partials.data_ptr<float>(), nullptr, nullptr, lse.data_ptr<float>(), N, nV);
  else
    lm_logprobs_v2_reduce<false><<<(N + wpb - 1) / wpb, 256, 0, stream>>>(
        partials.data_ptr<float>(), label_logit.data_ptr<float>(), out.data_ptr<float>(),
        want_lse ? lse.data_ptr<float>() : nullptr, N, nV);
  HIP_CHECK_LAST();
  return {out, lse};
}

}  // namespace

std::vector<at::Tensor> lm_logprobs_v2_with_lse(const at::Tensor& hidden,
                                                const at::Tensor& weight,
                                                const at::Tensor& labels, bool want_lse) {
  return launch_v2(hidden, weight, nullptr, labels, want_lse);
}

at::Tensor lm_logprobs_v2(const at::Tensor& hidden, const at::Tensor& weight,
                          const at::Tensor& labels) {
  return lm_logprobs_v2_with_lse(hidden, weight, labels, false)[0];
}

// (val, lse) of z = x @ w^T + bias: val[n] = z[n, idx[n]], lse[n] =
// logsumexp_v z[n, v].  idx outside [0, V) gives val 0.
std::vector<at::Tensor> linear_gather_lse_fwd(const at::Tensor& x, const at::Tensor& w,
                                              const at::Tensor& bias, const at::Tensor& idx) {
  TORCH_CHECK(bias.is_cuda() && bias.dtype() == at::kFloat && bias.is_contiguous() &&
              bias.numel() == w.size(0));
  return launch_v2(x, w, bias.data_ptr<float>(), idx, true);
}
