// Backward of the fused lm_head+logprobs training op (SURVEY.md K1+K5):
// dlogits[n,v] = dlp[n] * (1{v==labels[n]} - softmax(logits)[n,v]),
// with logits RECOMPUTED tile-by-tile from (hidden, weight) and the saved
// per-row logsumexp — the forward (lm_logprobs_v2) never materialized them.
// The caller contracts dlogits with W / hidden via hipBLASLt for dh and dW.
//
// The 256x256x64 MFMA mainloop is lm_tile_mainloop.inc, shared with the forward; the
// epilogue writes the bf16 dlogits tile straight from the accumulators
// (adjacent lanes hold adjacent columns -> 32 B-coalesced stores).
#include <c10/hip/HIPStream.h>

#include "lm_tile.h"

namespace {

using namespace lm_tile;

// Dynamic LDS: [ A buf0 | A buf1 | B buf0 | B buf1 | labels [256] | row_s [256][RS] ]
constexpr int LAB_OFF = AB_BYTES;
constexpr int ROW_OFF = LAB_OFF + BM * (int)sizeof(long);
constexpr int CE_LDS = AB_BYTES + 2048 + BM * 2 * (int)sizeof(float);
constexpr int GL_LDS = AB_BYTES + 2048 + BM * 3 * (int)sizeof(float);  // GATHER_LSE
static_assert(ROW_OFF + BM * 2 * (int)sizeof(float) <= CE_LDS &&
                  ROW_OFF + BM * 3 * (int)sizeof(float) <= GL_LDS,
              "row_s inside the launch's LDS");

// GATHER_LSE: the backward of linear_gather_lse (the ILQL Q heads), whose two
// outputs carry independent upstream gradients:
//   z = x @ w^T + bias,  dz[n,v] = g_lse[n] * exp(z[n,v] - lse[n])
//                                 + g_val[n] * 1{v == idx[n]}
// `dlp` is then g_val and `g_lse` the second per-row coefficient, staged next
// to it in row_s; the bias joins acc in the epilogue (a lane's four columns
// are fixed, so four loads).  Off, bias and g_lse are never read and this is
// the CE backward above — the g_val = g, g_lse = -g case in one coefficient.
template <bool GATHER_LSE>
__global__ __launch_bounds__(BLOCK) void ce_dlogits_kernel(
    const bf16_t* __restrict__ hidden, const bf16_t* __restrict__ weight,
    const long* __restrict__ labels, const float* __restrict__ lse,
    const float* __restrict__ dlp, bf16_t* __restrict__ dlogits, int N, int H, int V, int nV,
    int nM, const float* __restrict__ bias, const float* __restrict__ g_lse) {
  // (the GATHER_LSE arguments come last, so the others keep their slots)
  constexpr int RS = GATHER_LSE ? 3 : 2;  // row_s floats per row
  extern __shared__ char smem[];
  char* a_base = smem;
  char* b_base = smem + 2 * TILE_BYTES;
  long* lab_s = reinterpret_cast<long*>(smem + LAB_OFF);    // [256]
  float* row_s = reinterpret_cast<float*>(smem + ROW_OFF);  // [256][RS]: lse, dlp(, g_lse)

  const TileCoord tc = tile_coord(nV, nM);
  const int row0 = tc.row0, col0 = tc.col0;

  const int tid = threadIdx.x;
  const int lane = tid % WAVE;
  const int wid = tid / WAVE;
  const int wave_m = wid >> 2;
  const int wave_n = wid & 3;

  for (int i = tid; i < BM; i += BLOCK) {
    const int n = row0 + i;
    lab_s[i] = (n < N) ? labels[n] : -1;
    row_s[i * RS] = (n < N) ? lse[n] : 0.f;
    row_s[i * RS + 1] = (n < N) ? dlp[n] : 0.f;
    if constexpr (GATHER_LSE) row_s[i * RS + 2] = (n < N) ? g_lse[n] : 0.f;
  }

  f32x4 acc[8][4];
#include "lm_tile_mainloop.inc"
  const int max_br = V - 1;

  // epilogue: dlogits = dlp * (1{label} - exp(logit - lse)), straight from acc
  const int cgrp = lane >> 4;
  const int ccol0 = wave_n * 64 + (lane & 15);
  float bj[4] = {0.f, 0.f, 0.f, 0.f};
  if constexpr (GATHER_LSE) {
#pragma unroll
    for (int j = 0; j < 4; ++j) bj[j] = bias[min(col0 + ccol0 + j * 16, max_br)];
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int trow = wave_m * 128 + i * 16 + cgrp * 4 + r;
      const int n = row0 + trow;
      if (n >= N) continue;
      const float l = row_s[trow * RS];
      const float g = row_s[trow * RS + 1];
      float gl = 0.f;
      if constexpr (GATHER_LSE) gl = row_s[trow * RS + 2];
      const long lab = lab_s[trow];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int v = col0 + ccol0 + j * 16;
        if (v >= V) continue;
        float d;
        if constexpr (GATHER_LSE) {
          float p = __expf(acc[i][j][r] + bj[j] - l);
          d = gl * p + (v == lab ? g : 0.f);
        } else {
          float p = __expf(acc[i][j][r] - l);
          d = g * ((v == lab ? 1.f : 0.f) - p);
        }
        ScalarIO<bf16_t>::store(dlogits + (size_t)n * V + v, d);
      }
    }
  }
}

// bias == nullptr: the CE backward; otherwise the gather+lse backward.  dlp is
// g_val there; both may be strided.
at::Tensor launch_dlogits(const at::Tensor& hidden, const at::Tensor& weight, const float* bias,
                          const at::Tensor& labels, const at::Tensor& lse,
                          const at::Tensor& dlp, const float* g_lse) {
  const auto [N, H, V, nV, nM] = check_operands("ce_dlogits", hidden, weight, labels);
  TORCH_CHECK(lse.is_cuda() && lse.dtype() == at::kFloat && lse.is_contiguous() &&
              lse.numel() == N);
  TORCH_CHECK(dlp.is_cuda() && dlp.dtype() == at::kFloat && dlp.numel() == N);
  auto dlogits = at::empty({N, V}, hidden.options());
  if (N == 0) return dlogits;
  const auto g = dlp.contiguous();  // held until the launch is queued
  auto stream = c10::hip::getCurrentHIPStream();
  if (bias)
    allow_dynamic_lds<&ce_dlogits_kernel<true>, GL_LDS>();
  else
    allow_dynamic_lds<&ce_dlogits_kernel<false>, CE_LDS>();
  dim3 grid(nV, nM);
  auto* kern = bias ? &ce_dlogits_kernel<true> : &ce_dlogits_kernel<false>;
  kern<<<grid, BLOCK, bias ? GL_LDS : CE_LDS, stream>>>(
      reinterpret_cast<const bf16_t*>(hidden.data_ptr()),
      reinterpret_cast<const bf16_t*>(weight.data_ptr()), labels.data_ptr<long>(),
      lse.data_ptr<float>(), g.data_ptr<float>(),
      reinterpret_cast<bf16_t*>(dlogits.data_ptr()), N, H, V, nV, nM, bias, g_lse);
  HIP_CHECK_LAST();
  return dlogits;
}

}  // namespace

at::Tensor ce_dlogits(const at::Tensor& hidden, const at::Tensor& weight,
                      const at::Tensor& labels, const at::Tensor& lse, const at::Tensor& dlp) {
  return launch_dlogits(hidden, weight, nullptr, labels, lse, dlp, nullptr);
}

at::Tensor linear_gather_lse_bwd(const at::Tensor& x, const at::Tensor& w,
                                 const at::Tensor& bias, const at::Tensor& idx,
                                 const at::Tensor& lse, const at::Tensor& g_val,
                                 const at::Tensor& g_lse) {
  TORCH_CHECK(bias.is_cuda() && bias.dtype() == at::kFloat && bias.is_contiguous() &&
              bias.numel() == w.size(0));
  TORCH_CHECK(g_lse.is_cuda() && g_lse.dtype() == at::kFloat && g_lse.numel() == x.size(0));
  auto gl = g_lse.contiguous();
  return launch_dlogits(x, w, bias.data_ptr<float>(), idx, lse, g_val, gl.data_ptr<float>());
}
