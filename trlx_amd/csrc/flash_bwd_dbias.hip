// Flash attention BACKWARD, third kernel: the gradient of the T5 relative-
// position bias (the Toeplitz vector rel_bias [Hq, L] of ops.t5_rel_bias).
//
//   bias[h, q, k]    = rel_bias[h, k - q + bias_zero]
//   d_rel_bias[h, i] = sum over b and visible (q, k) with k - q + bias_zero == i
//                      of dS[b, h, q, k]
//   dS = P (dP - Drow),  P = exp(S - lse),  dP = dO V^T,  Drow = rowsum(dO * O)
//
// with S recomputed exactly as flash_bwd_dq_kernel does it (bf16 scale*Q
// A-fragments, rel_bias_score, the same visibility test).  Autograd carries
// the result through the embedding lookup of t5_rel_bias to the table.
//
// Ownership: a block owns DIAGONALS, not queries — 64 consecutive bias indices
// i0..i0+63 of one head, for the batch rows b = chunk, chunk + NB, ... of its
// batch chunk.  Every dS element of those diagonals and batch rows is added by
// this block alone, in a fixed order: no atomics, no two blocks add into the
// same element, and the result is bit-identical from run to run.  The host
// adds the NB per-chunk partials (partial.sum(0)); NB depends on the shapes only.
//
// Work split: the (batch row, 16-query group) pairs of a block are dealt
// round-robin to its four waves.  For queries qw..qw+15 the keys on the block's
// 64 diagonals are the 79-key window starting at qw + (i0 - bias_zero): five
// 16-key sub-tiles, a 16x80 fragment of S and dP of which 80 % lies on owned
// diagonals.  Query groups and sub-tiles whose keys miss [0, Tk) (or, CAUSAL,
// lie wholly above the diagonal) are skipped; causal tiles with i0 > bias_zero
// hold no visible pair and only write their zeros.
//
// Operand movement: there is no dV/dK/dQ accumulation here, so K and V need
// no transposed LDS staging.  The B operand of v_mfma_f32_16x16x32_bf16 for
// Q K^T and dO V^T is 8 consecutive d of one key per lane: one 16 B load from
// row-major K / V.  Q and dO are the wave's A-fragments, loaded per group.
// Every global row index is clamped ABSOLUTELY into the tensor (see
// load_afrag in flash_backward.hip); clamped rows are masked out of P.
//
// Reduction: the fp32 dS fragment (never rounded to bf16) goes to a wave-
// private LDS tile [16][80 + 1]; lane j then adds the 16 elements (r, r + j)
// of diagonal i0 + j — word address 82 r + j, conflict-free across the lanes —
// into ONE register that it keeps for the whole kernel.  At the end the four
// waves' partials are added in wave order through LDS.
// D=64: 85-96 VGPRs, D=128: 107-117 (the compiler issues the K/V loads of
// several sub-tiles ahead of the MFMAs); 21760 B static LDS, no scratch, four
// to five waves per SIMD (profiles/t5_bias_grad_notes.md).
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include "attn_host.h"

// The device code of this file is compiled without the packed fp32 VALU
// instructions (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32): every fp32 step
// after the MFMA is one scalar-per-lane instruction.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "common.h"

namespace {

constexpr int DB_BLOCK = 256;
constexpr int DB_WAVES = DB_BLOCK / WAVE;
constexpr int DB_DIAGS = 64;      // diagonals a block owns (one per lane)
constexpr int DB_WIN = 80;        // keys of a 16-query group's window: 5 sub-tiles
constexpr int DB_LD = DB_WIN + 1;  // row stride of the dS tile in words

typedef __attribute__((ext_vector_type(8))) short bf16x8_db;
typedef __attribute__((ext_vector_type(4))) float f32x4_db;

// per-lane: one 16-row MFMA operand fragment for the full head dim, row =
// first + (lane & 15) clamped absolutely into [0, rowmax], k-slice =
// (lane >> 4) * 8.  As an A operand the rows are queries, as a B operand keys.
template <int D>
DEV void load_frag(const bf16_t* __restrict__ src, int first, int rowmax, int lane,
                   bf16x8_db* frag, float mul) {
  const int row = min(max(first + (lane & 15), 0), rowmax);
  const int g8 = (lane >> 4) * 8;
#pragma unroll
  for (int dch = 0; dch < D / 32; ++dch) {
    bf16x8_db v8 = *reinterpret_cast<const bf16x8_db*>(src + (size_t)row * D + dch * 32 + g8);
    if (mul != 1.f) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v8[j] = (short)f2bf(bf2f((unsigned short)v8[j]) * mul);
    }
    frag[dch] = v8;
  }
}

// orders a wave's own LDS writes and reads of its private tile (the LDS
// executes one wave's accesses in order; this keeps the compiler from moving
// them across)
DEV void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <int D, bool CAUSAL, bool KMASK>
__global__ __launch_bounds__(DB_BLOCK) void flash_bwd_dbias_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
    const bf16_t* __restrict__ dout, const float* __restrict__ lse,
    const float* __restrict__ drow, const float* __restrict__ rel_bias /* [Hq, L] */,
    const unsigned char* __restrict__ key_mask /* [B, Tk]; read iff KMASK */,
    float* __restrict__ partial /* [NB, Hq, L] */, int B, int Hq, int Hkv, int Tq, int Tk, int L,
    int bias_zero, float scale) {
  const int i0 = blockIdx.x * DB_DIAGS;
  const int h = blockIdx.y;
  const int chunk = blockIdx.z;
  const int NB = gridDim.z;
  const int hkv = h / (Hq / Hkv);

  const int lane = threadIdx.x % WAVE;
  const int wid = threadIdx.x / WAVE;
  const int c = lane & 15;
  const int quad = lane >> 4;

  __shared__ float ds_lds[DB_WAVES][16 * DB_LD];
  __shared__ float red_lds[DB_WAVES][DB_DIAGS];

  // key - query of the block's first diagonal: query qrow meets diagonal
  // i0 + j at key qrow + delta + j
  const int delta = i0 - bias_zero;
  // 16-query groups whose window [qw + delta, qw + delta + 78] meets [0, Tk)
  const int q_lo = -delta - (DB_WIN - 2);
  const int q_hi = Tk - 1 - delta;
  const int g_lo = q_lo <= 0 ? 0 : (q_lo + 15) / 16;
  const int g_hi = q_hi < 0 ? -1 : min((Tq - 1) / 16, q_hi / 16);
  // causal: the block's lowest diagonal must reach key <= query
  const int ngroups = (CAUSAL && delta > 0) ? 0 : max(g_hi - g_lo + 1, 0);
  const int nrows = (B - chunk + NB - 1) / NB;  // batch rows chunk, chunk + NB, ...

  float acc = 0.f;  // this lane's diagonal i0 + lane, for the whole kernel
  float* tile = ds_lds[wid];
  const float* bias_row = rel_bias + (size_t)h * L;

  for (int item = wid; item < nrows * ngroups; item += DB_WAVES) {
    const int b = chunk + (item / ngroups) * NB;
    const int qw = (g_lo + item % ngroups) * 16;
    const size_t qbase = ((size_t)b * Hq + h) * (size_t)Tq;
    const size_t kbase = ((size_t)b * Hkv + hkv) * (size_t)Tk;

    bf16x8_db q_frag[D / 32], do_frag[D / 32];
    load_frag<D>(q + qbase * D, qw, Tq - 1, lane, q_frag, scale);
    load_frag<D>(dout + qbase * D, qw, Tq - 1, lane, do_frag, 1.f);
    float L_r[4], D_r[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qrow = min(qw + quad * 4 + r, Tq - 1);
      L_r[r] = lse[qbase + qrow];
      D_r[r] = drow[qbase + qrow];
    }

#pragma unroll
    for (int t = 0; t < DB_WIN / 16; ++t) {
      const int kb = qw + delta + t * 16;  // first key of the sub-tile
      f32x4_db ds = {0.f, 0.f, 0.f, 0.f};
      // wave-uniform: some key in [0, Tk) and, causal, some key <= some query
      if (kb + 15 >= 0 && kb < Tk && (!CAUSAL || kb <= qw + 15)) {
        bf16x8_db k_frag[D / 32], v_frag[D / 32];
        load_frag<D>(k + kbase * D, kb, Tk - 1, lane, k_frag, 1.f);
        load_frag<D>(v + kbase * D, kb, Tk - 1, lane, v_frag, 1.f);
        f32x4_db s = {0.f, 0.f, 0.f, 0.f};
        f32x4_db dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dch = 0; dch < D / 32; ++dch) {
          s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(q_frag[dch], k_frag[dch], s, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(do_frag[dch], v_frag[dch], dp, 0, 0, 0);
        }
        // element r: query = qw + quad*4 + r, key = kb + c
        const int key = kb + c;
        bool kvis = true;  // index clamped: keys outside [0, Tk) are masked anyway
        if constexpr (KMASK) kvis = key_mask[(size_t)b * Tk + min(max(key, 0), Tk - 1)] != 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qrow = qw + quad * 4 + r;
          const bool valid = key >= 0 && key < Tk && (!CAUSAL || key <= qrow) && qrow < Tq && kvis;
          const float sc = rel_bias_score(s[r], bias_row, L, key, qrow, bias_zero);
          ds[r] = (valid && L_r[r] < INFINITY) ? __expf(sc - L_r[r]) * (dp[r] - D_r[r]) : 0.f;
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) tile[(quad * 4 + r) * DB_LD + t * 16 + c] = ds[r];
    }
    wave_lds_fence();
    // diagonal i0 + lane crosses the fragment at (r, r + lane)
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) sum += tile[r * (DB_LD + 1) + lane];
    acc += sum;
    wave_lds_fence();  // the next group overwrites the tile
  }

  red_lds[wid][lane] = acc;
  __syncthreads();
  if (wid == 0) {
    float total = red_lds[0][lane];
#pragma unroll
    for (int w = 1; w < DB_WAVES; ++w) total += red_lds[w][lane];
    if (i0 + lane < L) partial[((size_t)chunk * Hq + h) * L + i0 + lane] = total;
  }
}

// Batch chunks: enough blocks for sixteen per CU of the 256, never more than B.
// The diagonals near relative position 0 cross every query and those at the
// ends almost none, so block times differ by the tile; four resident blocks
// per CU are dealt out several times over and the long tiles do not set the
// kernel time.  A pure function of the shapes, so the summation order — and
// with it every bit of the result — is the same on every call.
int dbias_batch_chunks(long B, long Hq, long L) {
  const long tiles = (L + DB_DIAGS - 1) / DB_DIAGS * Hq;
  const long want = (16 * 256 + tiles - 1) / tiles;
  return (int)std::min(B, std::max(1L, want));
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// d loss / d rel_bias [Hq, L] fp32 of ops.seq2seq_attention, from the tensors
// the forward saved: the third backward kernel next to flash_prefill_bwd.
at::Tensor flash_bwd_dbias(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                           const at::Tensor& out, const at::Tensor& dout, const at::Tensor& lse,
                           const at::Tensor& rel_bias, long bias_zero,
                           const c10::optional<at::Tensor>& key_mask, bool causal, double scale) {
  const char* op = "flash_bwd_dbias";
  TORCH_CHECK(q.is_cuda() && q.dtype() == at::kBFloat16 && q.dim() == 4 && q.is_contiguous(), op,
              ": q must be contiguous bf16 [B,Hq,Tq,D]");
  TORCH_CHECK(k.is_cuda() && v.is_cuda() && k.dtype() == at::kBFloat16 &&
                  v.dtype() == at::kBFloat16 && k.dim() == 4 && k.is_contiguous() &&
                  v.is_contiguous(),
              op, ": k and v must be contiguous bf16 [B,Hkv,Tk,D]");
  const int B = q.size(0), Hq = q.size(1), Tq = q.size(2), D = q.size(3);
  const int Hkv = k.size(1), Tk = k.size(2);
  TORCH_CHECK(B > 0 && Tq > 0 && Tk > 0, op, ": empty input");
  TORCH_CHECK(!causal || Tk == Tq, op, ": training path only (Tk == T)");
  TORCH_CHECK(k.size(0) == B && Hkv > 0 && Hq % Hkv == 0 && k.size(3) == D &&
                  v.sizes() == k.sizes(),
              op, ": k / v shape");
  TORCH_CHECK(out.sizes() == q.sizes() && dout.sizes() == q.sizes() && out.is_cuda() &&
                  dout.is_cuda() && out.dtype() == at::kBFloat16 &&
                  dout.dtype() == at::kBFloat16,
              op, ": out and dout must be bf16 of q's shape");
  TORCH_CHECK(lse.is_cuda() && lse.dtype() == at::kFloat && lse.is_contiguous() &&
                  lse.numel() == (long)B * Hq * Tq,
              op, ": lse must be contiguous fp32 [B,Hq,Tq]");
  const Seq2SeqArgs s2s = seq2seq_args(rel_bias, bias_zero, key_mask, causal, false, false, q, B,
                                       Hq, Tq, Tk, 0, D, op);
  const int L = s2s.bias_len;
  const int NB = dbias_batch_chunks(B, Hq, L);
  auto partial = at::empty({NB, Hq, L}, q.options().dtype(at::kFloat));
  auto dc = dout.contiguous();
  auto drow = (dc.to(at::kFloat) * out.to(at::kFloat)).sum(-1).contiguous();  // [B,Hq,Tq]
  auto stream = c10::hip::getCurrentHIPStream();
  dim3 grid((L + DB_DIAGS - 1) / DB_DIAGS, Hq, NB);
  dispatch_head_dim(kSeq2SeqFlashHeadDims, D, op, [&](auto d) {
    dispatch_bool(causal, [&](auto ca) {
      dispatch_bool(s2s.key_mask != nullptr, [&](auto km) {
        flash_bwd_dbias_kernel<decltype(d)::value, decltype(ca)::value, decltype(km)::value>
            <<<grid, DB_BLOCK, 0, stream>>>(
                reinterpret_cast<const bf16_t*>(q.data_ptr()),
                reinterpret_cast<const bf16_t*>(k.data_ptr()),
                reinterpret_cast<const bf16_t*>(v.data_ptr()),
                reinterpret_cast<const bf16_t*>(dc.data_ptr()), lse.data_ptr<float>(),
                drow.data_ptr<float>(), s2s.rel_bias, s2s.key_mask, partial.data_ptr<float>(), B,
                Hq, Hkv, Tq, Tk, L, s2s.bias_zero, (float)scale);
      });
    });
  });
  HIP_CHECK_LAST();
  return partial.sum(0);
}
