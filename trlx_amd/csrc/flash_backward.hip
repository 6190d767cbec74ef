// Flash attention BACKWARD (training path of SURVEY.md K2).
//
// Completes the flash attention story: with this, training forwards use the
// online-softmax kernel too and the [B, H, T, T] score tensor never
// materializes anywhere (at seq 2048 / batch 8 / 16 heads the bf16 scores
// alone are 1 GiB per layer per direction).
//
// Standard two-kernel recomputation scheme (deterministic, no atomics):
//   pre:  Drow = rowsum(dO * O)                       (torch, [B,Hq,T] fp32)
//   dKV:  one block per (b, hkv, 64-key tile): for each causal q-tile,
//         recompute S^T = K (scale*Q)^T, P^T = exp(S^T - L) from the saved
//         row logsumexp L, dP^T = V dO^T, dS^T = P^T (dP^T - Drow), then
//         dV += P^T dO and dK += dS^T (scale*Q); GQA sums over the query
//         heads of the group before the single write.  No atomics.
//   dQ:   one block per (b, hq, 64-query tile): recompute S/P per key-tile,
//         dP = dO V^T, dS = P (dP - Drow), dQ += scale * dS K.
//
// Register/LDS layout (the static-LDS budget is 64 KB, so the straight
// "stage everything in both layouts" plan does not fit at D=128):
//   * A-operands of every mfma are the wave's OWN 16 rows (keys in dKV,
//     queries in dQ) x full D — loaded once from global into VGPRs
//     (D/32 bf16x8 fragments) and reused for every tile.
//   * The contraction-side tensors are staged TRANSPOSED in LDS
//     ([D, 64+8]): the natural ds_read_b128 layout for the dV/dK/dQ
//     accumulation mfmas (B rows = d), and strided 2-byte reads rebuild the
//     row-major B fragments for the S / dP recomputation.
//   * P^T / dS^T / dS relayout (D-fragment -> A-operand) goes through a
//     wave-private [16, 64+8] LDS buffer, reused sequentially — same trick
//     as the forward's P relayout (flash_prefill.hip).
// Head dims: 64, 96, 128, 256.  D=96 is the same plan (D/32 = 3 k-steps).  At
// D=256 the two transposed staging tiles at 64 rows are 73.7 KB, so the
// staged tile narrows to 32 rows ([D, 32+8] x 2 + p_lds = 46 KB static);
// each block still owns 64 keys (dKV) or 64 queries (dQ) in registers and
// just takes twice as many staging steps.  Both new head dims measured slower
// than the materializing path in training (profiles/headdim_notes.md), so
// models take them only when asked (ops.flash_enabled): the O(T)-memory path.
// Masking (causal + left-pad key_starts) matches the forward; fully-masked
// query rows carry L = +inf so P == 0 and they contribute nothing.
// Seq2seq (T5) modes at head dims 64 / 128 mirror the forward's: non-causal
// (dKV sweeps every q-tile, dQ every key tile), rectangular Tq != Tk, the
// Toeplitz relative bias and the arbitrary key mask inside the recomputed P.
// The learned bias itself gets no gradient here.
// Precondition (as for left-pad key_starts): K and V rows at masked keys are
// FINITE.  A masked key enters dS as p * (dP - Drow) with p == 0, which is
// exact for any finite K/V (the tests fill them with 1e4) and NaN for inf/NaN.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include "attn_host.h"
#include "common.h"

namespace {

constexpr int BBLOCK = 256;
constexpr int BT = 64;  // rows a block owns in registers (keys in dKV, queries in dQ)
// rows of the contraction-side tile staged per step: 64, narrowed to 32 at
// D=256 where two [D, 64+8] tiles (73.7 KB) exceed the static-LDS limit
constexpr int bwd_st(int D) { return D > 128 ? 32 : 64; }
// dKV keeps k_frag + v_frag (D/4 VGPRs) and dv_acc + dk_acc (D/2 VGPRs)
// resident: 192 of the 256 registers a wave gets at two waves per SIMD when
// D=256, and the tile loop's working set on top of that spills.  That one
// instantiation asks for one wave per SIMD (512 registers, no scratch).
constexpr int dkv_waves(int D) { return D > 128 ? 1 : 2; }

typedef __attribute__((ext_vector_type(8))) short bf16x8_fb;
typedef __attribute__((ext_vector_type(4))) float f32x4_fb;

// block-wide: stage a [ST, D] bf16 tile TRANSPOSED into tds [D, ST+8],
// scaling by mul; rows past `nrows` clamp to the last valid row (their
// columns are masked out of P later).  Callers pass nrows >= 1.
template <int D, int ST>
DEV void stage_tileT(const bf16_t* __restrict__ src, long row0, long nrows,
                     unsigned short* __restrict__ tds, float mul) {
  constexpr int KPAD = ST + 8;
  for (int i = threadIdx.x; i < ST * (D / 8); i += BBLOCK) {
    const int row = i / (D / 8);
    const int col = (i % (D / 8)) * 8;
    const bf16_t* p = src + (size_t)(row0 + min((long)row, nrows - 1)) * D + col;
    bf16x8_fb v8 = *reinterpret_cast<const bf16x8_fb*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = bf2f((unsigned short)v8[j]);
      tds[(col + j) * KPAD + row] = f2bf(mul == 1.f ? f : f * mul);
    }
  }
}

// per-lane: load this wave's 16-row A-operand fragments (row = lane&15,
// k-slice = (lane>>4)*8) for the full head dim into registers.  rowmax is
// the ABSOLUTE last valid row (inclusive): a wave whose 16-row group starts
// past the end must clamp globally, not relatively — a relative clamp read
// up to 60 rows past the tensor and page-faulted the llama (D=128) bench
// when the allocation ended at the tensor.
template <int D>
DEV void load_afrag(const bf16_t* __restrict__ src, long row0, long rowmax, int lane,
                    bf16x8_fb* frag, float mul) {
  const long row = min(row0 + (long)(lane & 15), rowmax);
  const int g8 = (lane >> 4) * 8;
#pragma unroll
  for (int dch = 0; dch < D / 32; ++dch) {
    bf16x8_fb v8 = *reinterpret_cast<const bf16x8_fb*>(src + (size_t)row * D + dch * 32 + g8);
    if (mul != 1.f) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v8[j] = (short)f2bf(bf2f((unsigned short)v8[j]) * mul);
    }
    frag[dch] = v8;
  }
}

// strided B-operand fragment from a transposed [D, KPAD] tile: output row =
// tile row `col` (query/key index), k-slice elements d = dch*32 + g8 + j.
template <int KPAD>
DEV bf16x8_fb load_bfragT(const unsigned short* __restrict__ tds, int col, int dch, int g8) {
  bf16x8_fb r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (short)tds[(dch * 32 + g8 + j) * KPAD + col];
  return r;
}

// ALIBI is a template parameter in both kernels (as in the forward): the
// no-bias instantiations compile to exactly the code they were without it.
// So are the seq2seq (T5) modes CAUSAL / RELB / KMASK (see flash_prefill.hip);
// their kernel arguments are the trailing pack S2S, empty for the causal
// instantiations.  Rectangular attention (Tq != Tk, cross-
// attention) exists only with CAUSAL off: q/dout/lse/drow/dq are [.., Tq, ..]
// and k/v/dk/dv are [.., Tk, ..].  Causal training keeps Tq == Tk (checked on
// the host), and the causal instantiations keep using the one T for both.
template <int D, bool ALIBI, bool CAUSAL = true, bool RELB = false, bool KMASK = false,
          typename... S2S>
__global__ __launch_bounds__(BBLOCK, dkv_waves(D)) void flash_bwd_dkv_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
    const bf16_t* __restrict__ dout, const float* __restrict__ lse,
    const float* __restrict__ drow, const int* __restrict__ key_starts,
    const float* __restrict__ alibi_slopes /* [Hq]; read iff ALIBI */,
    bf16_t* __restrict__ dk, bf16_t* __restrict__ dv, int B, int Hq, int Hkv,
    int Tq /* queries; also the keys when CAUSAL */, float scale,
    S2S... s2s_args /* rel_bias, bias_len, bias_zero, key_mask, Tk (common.h s2s_view) */) {
  static_assert(s2s_pack_ok(!CAUSAL || RELB || KMASK, sizeof...(S2S), 5),
                "seq2seq arguments: (rel_bias, bias_len, bias_zero, key_mask, Tk) iff a mode is on");
  const S2SView s2s = s2s_view(s2s_args...);
  const float* __restrict__ rel_bias = s2s.rel_bias;          // read iff RELB
  const unsigned char* __restrict__ key_mask = s2s.key_mask;  // read iff KMASK
  const int bias_len = s2s.bias_len, bias_zero = s2s.bias_zero;
  constexpr int ST = bwd_st(D);  // queries staged per step
  constexpr int KPAD = ST + 8;
  const int Tk = CAUSAL ? Tq : s2s.Tk;
  const int kt = blockIdx.x * BT;
  const int hkv = blockIdx.y;
  const int b = blockIdx.z;
  if (kt >= Tk) return;
  const int rep = Hq / Hkv;
  const int kstart = key_starts ? key_starts[b] : 0;

  const int lane = threadIdx.x % WAVE;
  const int wid = threadIdx.x / WAVE;
  const int c = lane & 15;
  const int g8 = (lane >> 4) * 8;
  const int krow0 = wid * 16;  // this wave's 16 keys within the tile

  __shared__ unsigned short qT_lds[D * KPAD];
  __shared__ unsigned short doT_lds[D * KPAD];
  __shared__ float l_lds[ST];
  __shared__ float d_lds[ST];
  __shared__ unsigned short p_lds[BBLOCK / WAVE][16 * KPAD];

  // K/V A-fragments for this wave's 16 keys, resident for the whole kernel
  bf16x8_fb k_frag[D / 32], v_frag[D / 32];
  load_afrag<D>(k + ((size_t)b * Hkv + hkv) * (size_t)Tk * D, kt + krow0, (long)Tk - 1, lane,
                k_frag, 1.f);
  load_afrag<D>(v + ((size_t)b * Hkv + hkv) * (size_t)Tk * D, kt + krow0, (long)Tk - 1, lane,
                v_frag, 1.f);
  // this lane's 4 keys are fixed for the whole kernel: read their mask once
  // (index clamped to the last key; keys >= Tk are masked by `key < Tk`)
  bool kvis[4] = {true, true, true, true};
  if constexpr (KMASK) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      kvis[r] = key_mask[(size_t)b * Tk + min(kt + krow0 + (lane >> 4) * 4 + r, Tk - 1)] != 0;
  }

  f32x4_fb dv_acc[D / 16], dk_acc[D / 16];
#pragma unroll
  for (int d = 0; d < D / 16; ++d) {
    dv_acc[d] = {0.f, 0.f, 0.f, 0.f};
    dk_acc[d] = {0.f, 0.f, 0.f, 0.f};
  }

  for (int hq = hkv * rep; hq < (hkv + 1) * rep; ++hq) {
    const float slope = ALIBI ? alibi_slopes[hq] : 0.f;  // per QUERY head
    // causal: q-tiles at/after the diagonal; otherwise every q-tile
    for (int qt = CAUSAL ? kt : 0; qt < Tq; qt += ST) {
      __syncthreads();
      stage_tileT<D, ST>(q + ((size_t)b * Hq + hq) * (size_t)Tq * D, qt, Tq - qt, qT_lds, scale);
      stage_tileT<D, ST>(dout + ((size_t)b * Hq + hq) * (size_t)Tq * D, qt, Tq - qt, doT_lds,
                         1.f);
      for (int i = threadIdx.x; i < ST; i += BBLOCK) {
        const int qrow = min(qt + i, Tq - 1);
        l_lds[i] = lse[((size_t)b * Hq + hq) * Tq + qrow];
        d_lds[i] = drow[((size_t)b * Hq + hq) * Tq + qrow];
      }
      __syncthreads();

      // S^T / dP^T fragments [this wave's 16 keys x ST queries]
      f32x4_fb pt[ST / 16], dst[ST / 16];
#pragma unroll
      for (int qq = 0; qq < ST / 16; ++qq) {
        f32x4_fb st = {0.f, 0.f, 0.f, 0.f};
        f32x4_fb dpt = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dch = 0; dch < D / 32; ++dch) {
          bf16x8_fb qf = load_bfragT<KPAD>(qT_lds, qq * 16 + c, dch, g8);
          st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k_frag[dch], qf, st, 0, 0, 0);
          bf16x8_fb df = load_bfragT<KPAD>(doT_lds, qq * 16 + c, dch, g8);
          dpt = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v_frag[dch], df, dpt, 0, 0, 0);
        }
        // element r: key = kt + krow0 + (lane>>4)*4 + r, query = qt + qq*16 + c
        const int qpos = qt + qq * 16 + c;
        const float L = l_lds[qq * 16 + c];
        const float Dr = d_lds[qq * 16 + c];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = kt + krow0 + (lane >> 4) * 4 + r;
          const bool valid = key < Tk && key >= kstart && (!CAUSAL || key <= qpos) &&
                             qpos < Tq && kvis[r];
          // same biased score the forward folded into L
          if constexpr (ALIBI) st[r] = alibi_score(st[r], slope, key, kstart);
          if constexpr (RELB)
            st[r] = rel_bias_score(st[r], rel_bias + (size_t)hq * bias_len, bias_len, key, qpos,
                                   bias_zero);
          const float p = (valid && L < INFINITY) ? __expf(st[r] - L) : 0.f;
          st[r] = p;
          dpt[r] = p * (dpt[r] - Dr);
        }
        pt[qq] = st;
        dst[qq] = dpt;
      }

      unsigned short* pw = p_lds[wid];  // wave-private: no block barrier needed
      // dV += P^T dO  (A = P^T via relayout, B = doT natural rows = d)
#pragma unroll
      for (int qq = 0; qq < ST / 16; ++qq)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          pw[((lane >> 4) * 4 + r) * KPAD + qq * 16 + c] = f2bf(pt[qq][r]);
#pragma unroll
      for (int d = 0; d < D / 16; ++d)
#pragma unroll
        for (int qch = 0; qch < ST; qch += 32) {
          bf16x8_fb pf = *reinterpret_cast<const bf16x8_fb*>(&pw[c * KPAD + qch + g8]);
          bf16x8_fb dof =
              *reinterpret_cast<const bf16x8_fb*>(&doT_lds[(d * 16 + c) * KPAD + qch + g8]);
          dv_acc[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, dof, dv_acc[d], 0, 0, 0);
        }
      // dK += dS^T (scale*Q)  (A = dS^T via relayout, B = qT natural)
#pragma unroll
      for (int qq = 0; qq < ST / 16; ++qq)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          pw[((lane >> 4) * 4 + r) * KPAD + qq * 16 + c] = f2bf(dst[qq][r]);
#pragma unroll
      for (int d = 0; d < D / 16; ++d)
#pragma unroll
        for (int qch = 0; qch < ST; qch += 32) {
          bf16x8_fb sf = *reinterpret_cast<const bf16x8_fb*>(&pw[c * KPAD + qch + g8]);
          bf16x8_fb qtf =
              *reinterpret_cast<const bf16x8_fb*>(&qT_lds[(d * 16 + c) * KPAD + qch + g8]);
          dk_acc[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sf, qtf, dk_acc[d], 0, 0, 0);
        }
    }
  }

  // write this wave's 16 keys of dK/dV (C row = key-within-16, col = d)
#pragma unroll
  for (int d = 0; d < D / 16; ++d)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = kt + krow0 + (lane >> 4) * 4 + r;
      if (key >= Tk) continue;
      dv[(((size_t)b * Hkv + hkv) * Tk + key) * D + d * 16 + c].u = f2bf(dv_acc[d][r]);
      dk[(((size_t)b * Hkv + hkv) * Tk + key) * D + d * 16 + c].u = f2bf(dk_acc[d][r]);
    }
}

template <int D, bool ALIBI, bool CAUSAL = true, bool RELB = false, bool KMASK = false,
          typename... S2S>
__global__ __launch_bounds__(BBLOCK, 2) void flash_bwd_dq_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
    const bf16_t* __restrict__ dout, const float* __restrict__ lse,
    const float* __restrict__ drow, const int* __restrict__ key_starts,
    const float* __restrict__ alibi_slopes /* [Hq]; read iff ALIBI */,
    bf16_t* __restrict__ dq, int B, int Hq, int Hkv,
    int Tq /* queries; also the keys when CAUSAL */, float scale,
    S2S... s2s_args /* rel_bias, bias_len, bias_zero, key_mask, Tk (common.h s2s_view) */) {
  static_assert(s2s_pack_ok(!CAUSAL || RELB || KMASK, sizeof...(S2S), 5),
                "seq2seq arguments: (rel_bias, bias_len, bias_zero, key_mask, Tk) iff a mode is on");
  const S2SView s2s = s2s_view(s2s_args...);
  const float* __restrict__ rel_bias = s2s.rel_bias;          // read iff RELB
  const unsigned char* __restrict__ key_mask = s2s.key_mask;  // read iff KMASK
  const int bias_len = s2s.bias_len, bias_zero = s2s.bias_zero;
  constexpr int ST = bwd_st(D);  // keys staged per step
  constexpr int KPAD = ST + 8;
  const int Tk = CAUSAL ? Tq : s2s.Tk;
  const int qt = blockIdx.x * BT;
  const int h = blockIdx.y;
  const int b = blockIdx.z;
  if (qt >= Tq) return;
  const int hkv = h / (Hq / Hkv);
  const int kstart = key_starts ? key_starts[b] : 0;
  const float slope = ALIBI ? alibi_slopes[h] : 0.f;

  const int lane = threadIdx.x % WAVE;
  const int wid = threadIdx.x / WAVE;
  const int c = lane & 15;
  const int g8 = (lane >> 4) * 8;
  const int qrow0 = wid * 16;  // this wave's 16 queries within the tile

  __shared__ unsigned short kT_lds[D * KPAD];
  __shared__ unsigned short vT_lds[D * KPAD];
  __shared__ unsigned short p_lds[BBLOCK / WAVE][16 * KPAD];

  // scaled-Q / dO A-fragments for this wave's 16 queries, plus their L / Drow
  bf16x8_fb q_frag[D / 32], do_frag[D / 32];
  load_afrag<D>(q + ((size_t)b * Hq + h) * (size_t)Tq * D, qt + qrow0, (long)Tq - 1, lane,
                q_frag, scale);
  load_afrag<D>(dout + ((size_t)b * Hq + h) * (size_t)Tq * D, qt + qrow0, (long)Tq - 1, lane,
                do_frag, 1.f);
  float L_r[4], D_r[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = min(qt + qrow0 + (lane >> 4) * 4 + r, Tq - 1);
    L_r[r] = lse[((size_t)b * Hq + h) * Tq + qrow];
    D_r[r] = drow[((size_t)b * Hq + h) * Tq + qrow];
  }

  f32x4_fb dq_acc[D / 16];
#pragma unroll
  for (int d = 0; d < D / 16; ++d) dq_acc[d] = {0.f, 0.f, 0.f, 0.f};

  const int kt_lo = (kstart / ST) * ST;
  // causal: no key tile past this block's last query
  const int kt_hi = CAUSAL ? min(Tk, qt + BT) : Tk;
  for (int kt = kt_lo; kt < kt_hi; kt += ST) {
    __syncthreads();
    stage_tileT<D, ST>(k + ((size_t)b * Hkv + hkv) * (size_t)Tk * D, kt, Tk - kt, kT_lds, 1.f);
    stage_tileT<D, ST>(v + ((size_t)b * Hkv + hkv) * (size_t)Tk * D, kt, Tk - kt, vT_lds, 1.f);
    __syncthreads();

    unsigned short* pw = p_lds[wid];
#pragma unroll
    for (int kk = 0; kk < ST / 16; ++kk) {
      f32x4_fb s = {0.f, 0.f, 0.f, 0.f};
      f32x4_fb dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int dch = 0; dch < D / 32; ++dch) {
        bf16x8_fb kf = load_bfragT<KPAD>(kT_lds, kk * 16 + c, dch, g8);
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(q_frag[dch], kf, s, 0, 0, 0);
        bf16x8_fb vf = load_bfragT<KPAD>(vT_lds, kk * 16 + c, dch, g8);
        dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(do_frag[dch], vf, dp, 0, 0, 0);
      }
      // element r: query = qt + qrow0 + (lane>>4)*4 + r, key = kt + kk*16 + c
      const int key = kt + kk * 16 + c;
      bool kvis = true;  // index clamped: keys >= Tk are masked by `key < Tk` anyway
      if constexpr (KMASK) kvis = key_mask[(size_t)b * Tk + min(key, Tk - 1)] != 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qrow = qt + qrow0 + (lane >> 4) * 4 + r;
        const bool valid = key < Tk && key >= kstart && (!CAUSAL || key <= qrow) &&
                           qrow < Tq && kvis;
        if constexpr (ALIBI) s[r] = alibi_score(s[r], slope, key, kstart);
        if constexpr (RELB)
          s[r] = rel_bias_score(s[r], rel_bias + (size_t)h * bias_len, bias_len, key, qrow,
                                bias_zero);
        const float p = (valid && L_r[r] < INFINITY) ? __expf(s[r] - L_r[r]) : 0.f;
        s[r] = p * (dp[r] - D_r[r]);  // dS
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
        pw[((lane >> 4) * 4 + r) * KPAD + kk * 16 + c] = f2bf(s[r]);
    }
    // dQ += dS K  (A = dS via relayout, B = kT natural rows = d)
#pragma unroll
    for (int d = 0; d < D / 16; ++d)
#pragma unroll
      for (int kch = 0; kch < ST; kch += 32) {
        bf16x8_fb sf = *reinterpret_cast<const bf16x8_fb*>(&pw[c * KPAD + kch + g8]);
        bf16x8_fb ktf =
            *reinterpret_cast<const bf16x8_fb*>(&kT_lds[(d * 16 + c) * KPAD + kch + g8]);
        dq_acc[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sf, ktf, dq_acc[d], 0, 0, 0);
      }
  }

#pragma unroll
  for (int d = 0; d < D / 16; ++d)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qrow = qt + qrow0 + (lane >> 4) * 4 + r;
      if (qrow >= Tq) continue;
      dq[(((size_t)b * Hq + h) * Tq + qrow) * D + d * 16 + c].u = f2bf(scale * dq_acc[d][r]);
    }
}

}  // namespace

// reference parity: CarperAI/trlx delegates attention backward to HF/torch
// autograd through the materialized scores; here the same gradients come from
// the recomputation kernels above (see tests/test_flash_backward.py).
std::vector<at::Tensor> flash_prefill_bwd(const at::Tensor& q, const at::Tensor& k,
                                          const at::Tensor& v, const at::Tensor& out,
                                          const at::Tensor& dout, const at::Tensor& lse,
                                          const c10::optional<at::Tensor>& key_starts,
                                          double scale,
                                          const c10::optional<at::Tensor>& alibi_slopes,
                                          const c10::optional<at::Tensor>& rel_bias,
                                          long bias_zero,
                                          const c10::optional<at::Tensor>& key_mask,
                                          bool causal) {
  TORCH_CHECK(q.is_cuda() && q.dtype() == at::kBFloat16 && q.dim() == 4 && q.is_contiguous(),
              "flash_prefill_bwd: q must be contiguous bf16 [B,Hq,T,D]");
  TORCH_CHECK(k.is_contiguous() && v.is_contiguous() && lse.is_contiguous());
  const int B = q.size(0), Hq = q.size(1), T = q.size(2), D = q.size(3);
  const int Hkv = k.size(1), Tk = k.size(2);
  // causal training: full self-attention from position 0 (the kernels have no
  // start_pos); only the non-causal modes take Tq != Tk (cross-attention)
  TORCH_CHECK(!causal || Tk == T, "flash_prefill_bwd: training path only (Tk == T)");
  TORCH_CHECK(Hq % Hkv == 0 && k.size(3) == D && v.sizes() == k.sizes());
  TORCH_CHECK(out.sizes() == q.sizes() && dout.sizes() == q.sizes() && lse.numel() == (long)B * Hq * T);
  const float* sl = alibi_slopes_ptr(alibi_slopes, q, Hq, "flash_prefill_bwd");
  const Seq2SeqArgs s2s =
      seq2seq_args(rel_bias, bias_zero, key_mask, causal, key_starts.has_value(), sl != nullptr,
                   q, B, Hq, T, Tk, 0, D, "flash_prefill_bwd");
  const auto ks_t = optional_int_ptr(key_starts, q, B, "flash_prefill_bwd", "key_starts");
  const int* ks = ks_t.second;
  auto dq = at::empty_like(q);
  auto dk = at::empty_like(k);
  auto dv = at::empty_like(v);
  auto dc = dout.contiguous();
  auto drow = (dc.to(at::kFloat) * out.to(at::kFloat)).sum(-1).contiguous();  // [B,Hq,T]
  auto stream = c10::hip::getCurrentHIPStream();
  auto qp = reinterpret_cast<const bf16_t*>(q.data_ptr());
  auto kp = reinterpret_cast<const bf16_t*>(k.data_ptr());
  auto vp = reinterpret_cast<const bf16_t*>(v.data_ptr());
  auto dop = reinterpret_cast<const bf16_t*>(dc.data_ptr());
  auto dqp = reinterpret_cast<bf16_t*>(dq.data_ptr());
  auto dkp = reinterpret_cast<bf16_t*>(dk.data_ptr());
  auto dvp = reinterpret_cast<bf16_t*>(dv.data_ptr());
  const float* lp = lse.data_ptr<float>();
  const float* drp = drow.data_ptr<float>();
  dim3 gk((Tk + BT - 1) / BT, Hkv, B);
  dim3 gq((T + BT - 1) / BT, Hq, B);
  dispatch_flash_mode(
      D, sl != nullptr, s2s.any, causal, s2s.rel_bias != nullptr, s2s.key_mask != nullptr,
      "flash_prefill_bwd", [&](auto d, auto al, auto ca, auto rb, auto km) {
        constexpr int DV = decltype(d)::value;
        constexpr bool AL = decltype(al)::value, CA = decltype(ca)::value,
                       RB = decltype(rb)::value, KM = decltype(km)::value;
        // both kernels end in the same optional seq2seq pack
        auto launch = [&](auto... s2s_pack) {
          flash_bwd_dkv_kernel<DV, AL, CA, RB, KM><<<gk, BBLOCK, 0, stream>>>(
              qp, kp, vp, dop, lp, drp, ks, sl, dkp, dvp, B, Hq, Hkv, T, (float)scale,
              s2s_pack...);
          flash_bwd_dq_kernel<DV, AL, CA, RB, KM><<<gq, BBLOCK, 0, stream>>>(
              qp, kp, vp, dop, lp, drp, ks, sl, dqp, B, Hq, Hkv, T, (float)scale, s2s_pack...);
        };
        if constexpr (CA && !RB && !KM) launch();
        else launch(s2s.rel_bias, s2s.bias_len, s2s.bias_zero, s2s.key_mask, Tk);
      });
  HIP_CHECK_LAST();
  return {dq, dk, dv};
}
