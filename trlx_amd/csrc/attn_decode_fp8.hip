// Decode attention over the fp8 KV cache (format: kv_fp8.hip): e4m3 codes
// [B, Hkv, S, D] with one fp32 scale per (batch row, KV head, key).  The cache is
// streamed at 1 + 4/D bytes per element instead of the bf16 kernels' 2.
//
//   q [B, Hq, 1, D] bf16 (unscaled), G = Hq / Hkv >= 1 (MHA, GQA and MQA alike),
//   visible keys of row b: [seq_starts[b], seq_lens[b]).
//
// Work split (that of attn_decode_gqa.hip).  A 256-thread block owns (batch row,
// KV head, chunk of up to 16 query heads of that KV head's group, key split s of
// NS).  The chunk's heads are the 16 M-rows of v_mfma_f32_16x16x32_bf16; rows past
// the group hold q = 0 and are never stored (at G = 1 one row is live: the MFMA
// is idle capacity of a kernel that waits on memory).  Split s covers the keys
// [s * per, (s + 1) * per) of the ALLOCATED length S, cut to the row's visible
// range.  The four waves take the 32-key sub-tiles of that range round-robin and
// meet only after the loop: no block barrier inside it.
//
// Data movement, per wave and 32-key sub-tile:
//   Q   resident bf16 A-fragments, unscaled.  The contraction index is PERMUTED
//       to suit the K load below: MFMA i (0 .. D/32) contracts, in its k-slot
//       quad*8 + j, the dim d = (i/2)*64 + quad*16 + (i%2)*8 + j.  Q is loaded
//       once with that permutation; any permutation of the contraction index
//       applied to both operands leaves the product unchanged.
//   K   the B operand straight from global memory: lane (c, quad) loads 16 B =
//       16 consecutive d of key c at d = L*64 + quad*16, which are exactly that
//       lane's B fragments of the two MFMAs 2L and 2L + 1.  D = 64: one load and
//       two MFMAs per 16 keys, D = 128: two loads and four MFMAs.  The bytes are
//       dequantized in registers (v_cvt_pk_f32_fp8, then the high halves of two
//       floats packed into one word: every e4m3 value is exact in bf16, so
//       this rounds nothing).  The next sub-tile's K and k_scale are requested as
//       soon as the MFMAs have read this one's.
//   S   score[h, key] = (scale * k_scale[key]) * acc (+ ALiBi) in fp32: the key's
//       scale multiplies the C fragment's column, which one lane holds (column c).
//       Online (m, l) per head row in fp32.
//   P   p * v_scale[key] in fp32, ONE rounding to bf16, relaid C-fragment ->
//       A-fragment through the wave's P tile.  l sums the unscaled p.  The V
//       codes therefore enter the P V MFMA exactly, as bf16.
//   V   loaded coalesced, 16 B per lane (lane -> key id / (D/16), bytes
//       16 * (id % (D/16))), rows of keys outside the visible range replaced by
//       zeros, dequantized and stored ROW-MAJOR as bf16 [32 keys][D/2 + 1 words];
//       the transposed B fragment is gathered with eight 16-bit reads
//       v[quad*8 + j][dg*16 + c].
// Every K and V byte of the block's key range leaves global memory once.  Every
// row index (key, query head) is clamped absolutely into its tensor before the
// load; clamped rows are masked.  A scale of 0 (an all-zero row) gives score
// 0 * acc = 0 and p * 0 = 0: the store kernel never writes a NaN code, so acc is
// finite.
//
// LDS layout and banks (32 banks of 4 B).  The tile is bf16 AFTER the dequantize,
// so its width is the grouped bf16 kernel's: per wave the V tile, 32 rows of
// RS = D/2 + 1 words, then the P tile, 16 rows of 20 words.
//   V reads:  lane (c, quad) reads the half-word at word
//             (quad*8 + j) * RS + dg*8 + c/2.  RS = 1 (mod 4) gives 8*RS = 8
//             (mod 32): the four quads start 8 banks apart and each covers 8
//             consecutive words (two lanes share a word, a broadcast), so the 64
//             lanes touch each of the 32 banks with ONE word: conflict-free.
//   V writes: a lane's 16 codes become 8 words at row * RS + 8 * chunk + w, written
//             as eight 32-bit stores (an odd row stride is only 4 B aligned).  One
//             store instruction covers 8 rows x 8 chunks at D = 128 and 16 rows x
//             4 chunks at D = 64; its bank is row + 8 * chunk + w (mod 32), and in
//             both shapes the 64 lanes fall exactly two to a bank, the minimum
//             for 64 words.
//   P tile:   written one bf16 at a time (row quad*4 + r, column kk*16 + c), read
//             as 16 B at word 20 * c + 4 * quad: conflict-free per 8-lane group.
//   Merge:    after the loop a wave's V tile holds its fp32 O [16][D + 2].
//
// Merge.  The four waves' (m, l, O) meet through LDS once.  NS == 1: the block
// divides by l and writes bf16.  NS > 1: it writes fp32 (m, l, O) to a workspace
// and attn_decode_fp8_merge combines the splits — two plain launches, no atomics,
// no counters, NS a pure function of the static sizes, so both capture into the
// decode hipGraph.  A row with no visible key returns zeros.
//
// Registers / LDS per instantiation and timings: profiles/kv_fp8_notes.md.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>

#include "attn_host.h"

// As attn_decode_gqa.hip: no packed fp32 VALU instructions in this file's device
// code, so every fp32 step after the MFMA is one scalar-per-lane instruction.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "common.h"

namespace {

constexpr int F8_BLOCK = 256;
constexpr int F8_WAVES = F8_BLOCK / WAVE;
constexpr int F8_ROWS = 16;  // query heads per block: the MFMA M dimension
constexpr int F8_KT = 32;    // keys per wave sub-tile: the MFMA K dimension of P V
constexpr int F8_PLD = F8_KT + 8;                // P tile row stride in shorts
constexpr int F8_PWORDS = F8_ROWS * F8_PLD / 2;  // P tile in words
constexpr int F8_MAX_SPLITS = 64;

constexpr int f8_rs(int D) { return D / 2 + 1; }             // V tile row stride in words
constexpr int f8_vwords(int D) { return F8_KT * f8_rs(D); }  // == F8_ROWS * (D + 2)

typedef __attribute__((ext_vector_type(8))) short bf16x8_f8;
typedef __attribute__((ext_vector_type(4))) float f32x4_f8;
typedef __attribute__((ext_vector_type(2))) float f32x2_f8;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_f8;

// orders a wave's own LDS writes and reads of its private tiles
DEV void f8_wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// all-reduce over the 16 lanes of a DPP row (one C-fragment row)
template <int CTRL>
DEV float f8_dpp(float v) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
DEV float f8_row_max(float v) {
  v = fmaxf(v, f8_dpp<0xB1>(v));      // quad_perm [1,0,3,2]
  v = fmaxf(v, f8_dpp<0x4E>(v));      // quad_perm [2,3,0,1]
  v = fmaxf(v, f8_dpp<0x141>(v));     // row_half_mirror
  return fmaxf(v, f8_dpp<0x140>(v));  // row_mirror
}
DEV float f8_row_sum(float v) {
  v += f8_dpp<0xB1>(v);
  v += f8_dpp<0x4E>(v);
  v += f8_dpp<0x141>(v);
  return v + f8_dpp<0x140>(v);
}

DEV void f8_block_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// two e4m3 codes (the low or the high half of w) -> two bf16 in one word: the
// converts give fp32 whose low 16 bits are zero, so the bf16 pair is the two
// high halves (the compiler makes one byte-permute of the shift, mask and or)
template <bool HI>
DEV unsigned int f8_dequant2(unsigned int w) {
  const f32x2_f8 f = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, HI);
  // scalars first: a bit cast applied to the vector element f[1] itself read f[0]
  const float f0 = f[0], f1 = f[1];
  return (__builtin_bit_cast(unsigned int, f0) >> 16) |
         (__builtin_bit_cast(unsigned int, f1) & 0xffff0000u);
}

// 8 codes (two words) -> one bf16 MFMA operand
DEV bf16x8_f8 f8_dequant8(unsigned int w0, unsigned int w1) {
  const u32x4_f8 r = {f8_dequant2<false>(w0), f8_dequant2<true>(w0), f8_dequant2<false>(w1),
                      f8_dequant2<true>(w1)};
  return __builtin_bit_cast(bf16x8_f8, r);
}

// the raw K bytes and the key scales of the sub-tile starting at key kb: one
// 16 B load per (16-key half, 64-dim chunk), key row clamped absolutely
template <int D>
DEV void f8_load_k(const unsigned char* __restrict__ kbase, const float* __restrict__ ksbase,
                   int kb, int S, int c, int quad, u32x4_f8 (&kraw)[2][D / 64], float (&ks)[2]) {
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const int row = min(max(kb + kk * 16 + c, 0), S - 1);
#pragma unroll
    for (int L = 0; L < D / 64; ++L)
      kraw[kk][L] =
          *reinterpret_cast<const u32x4_f8*>(kbase + (size_t)row * D + L * 64 + quad * 16);
    ks[kk] = ksbase[row];
  }
}

template <int D, bool ALIBI>
__global__ __launch_bounds__(F8_BLOCK) void attn_decode_fp8_kernel(
    const bf16_t* __restrict__ q, const unsigned char* __restrict__ kc,
    const float* __restrict__ kscale, const unsigned char* __restrict__ vc,
    const float* __restrict__ vscale, const int* __restrict__ seq_lens,
    const int* __restrict__ seq_starts,
    const float* __restrict__ alibi_slopes /* [Hq], read iff ALIBI */,
    bf16_t* __restrict__ out /* [B, Hq, D], written iff NS == 1 */,
    float* __restrict__ ws_o /* [B, Hq, NS, D], written iff NS > 1 */,
    float* __restrict__ ws_ml /* [B, Hq, NS, 2] */, int Hq, int Hkv, int S, int chunks, int NS,
    int per, float scale) {
  constexpr int RS = f8_rs(D);
  constexpr int VWORDS = f8_vwords(D);
  constexpr int VLD = 2 * RS;      // V tile row stride in shorts
  constexpr int OLD = D + 2;       // O tile row stride in floats (merge)
  constexpr int CPR = D / 16;      // 16 B chunks per V row of codes
  constexpr int RPI = WAVE / CPR;  // V rows a wave loads per instruction
  static_assert(VWORDS == F8_ROWS * OLD, "the O tile of the merge reuses the V tile");

  // block -> (b, hkv, chunk, split), split fastest
  const int split = blockIdx.x % NS;
  const int chunk = (blockIdx.x / NS) % chunks;
  const int bh = blockIdx.x / (NS * chunks);
  const int b = bh / Hkv;
  const int hkv = bh % Hkv;
  const int G = Hq / Hkv;
  const int head0 = hkv * G + chunk * F8_ROWS;          // query head of M-row 0
  const int nrows = min(G - chunk * F8_ROWS, F8_ROWS);  // M-rows that are query heads

  // visible keys of this block: split range cut to [kstart, len), all inside [0, S)
  const int len = min(seq_lens[b], S);
  const int kstart = max(seq_starts ? seq_starts[b] : 0, 0);
  const int lo = max(split * per, kstart);
  const int hi = min(min((split + 1) * per, S), len);
  const int ntiles = hi > lo ? (hi - lo + F8_KT - 1) / F8_KT : 0;

  const int lane = threadIdx.x % WAVE;
  const int wid = threadIdx.x / WAVE;
  const int c = lane & 15;
  const int quad = lane >> 4;

  // 16 B aligned: the P tile is read back as 128-bit A-fragments
  __shared__ __attribute__((aligned(16))) unsigned int tile_lds[F8_WAVES][VWORDS + F8_PWORDS];
  __shared__ float ml_lds[F8_WAVES][F8_ROWS][2];
  unsigned int* v_w = tile_lds[wid];
  const unsigned short* v_s = reinterpret_cast<const unsigned short*>(v_w);
  unsigned short* p_s = reinterpret_cast<unsigned short*>(v_w + VWORDS);

  const size_t bhkv = (size_t)b * Hkv + hkv;
  const unsigned char* kbase = kc + bhkv * (size_t)S * D;
  const unsigned char* vbase = vc + bhkv * (size_t)S * D;
  const float* ksbase = kscale + bhkv * (size_t)S;
  const float* vsbase = vscale + bhkv * (size_t)S;

  // Q A-fragments, contraction index permuted as the K load needs: fragment i
  // holds d = (i/2)*64 + quad*16 + (i%2)*8 + j; row c is query head head0 + c
  bf16x8_f8 q_frag[D / 32];
  {
    const int hq = min(head0 + c, Hq - 1);
    const bf16_t* qp = q + ((size_t)b * Hq + hq) * D + quad * 16;
    const bf16x8_f8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < D / 32; ++i) {
      const bf16x8_f8 v8 = *reinterpret_cast<const bf16x8_f8*>(qp + (i / 2) * 64 + (i % 2) * 8);
      q_frag[i] = c < nrows ? v8 : zero;
    }
  }
  // the slope of each C-fragment row's QUERY head
  float slope[4] = {0.f, 0.f, 0.f, 0.f};
  if constexpr (ALIBI) {
#pragma unroll
    for (int r = 0; r < 4; ++r) slope[r] = alibi_slopes[min(head0 + quad * 4 + r, Hq - 1)];
  }

  float m_row[4], l_row[4];  // fragment rows quad*4 + r, equal on the 16 lanes of a quad
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m_row[r] = -INFINITY;
    l_row[r] = 0.f;
  }
  f32x4_f8 oacc[D / 16];  // O fragments [16 heads x 16 d] per d-group
#pragma unroll
  for (int dg = 0; dg < D / 16; ++dg) oacc[dg] = {0.f, 0.f, 0.f, 0.f};

  u32x4_f8 kraw[2][D / 64];
  float ks[2] = {0.f, 0.f};
  if (wid < ntiles) f8_load_k<D>(kbase, ksbase, lo + wid * F8_KT, S, c, quad, kraw, ks);

  for (int t = wid; t < ntiles; t += F8_WAVES) {
    const int kb = lo + t * F8_KT;  // first key of the sub-tile

    // ---- V codes and scales: coalesced 16 B loads, issued before the score MFMAs
    u32x4_f8 vraw[F8_KT / RPI];
#pragma unroll
    for (int it = 0; it < F8_KT / RPI; ++it) {
      const int row = min(max(kb + it * RPI + lane / CPR, 0), S - 1);
      vraw[it] =
          *reinterpret_cast<const u32x4_f8*>(vbase + (size_t)row * D + (lane % CPR) * 16);
    }
    float vs[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) vs[kk] = vsbase[min(max(kb + kk * 16 + c, 0), S - 1)];

    // ---- S = Q K^T: two [16 heads x 16 keys] fragments ----------------------
    f32x4_f8 sfrag[2];
    float kscl[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      f32x4_f8 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < D / 32; ++i) {
        const bf16x8_f8 kf =
            f8_dequant8(kraw[kk][i / 2][(i % 2) * 2], kraw[kk][i / 2][(i % 2) * 2 + 1]);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(q_frag[i], kf, acc, 0, 0, 0);
      }
      sfrag[kk] = acc;
      kscl[kk] = scale * ks[kk];
    }
    // this wave's next sub-tile, into the registers the MFMAs have just read
    if (t + F8_WAVES < ntiles)
      f8_load_k<D>(kbase, ksbase, kb + F8_WAVES * F8_KT, S, c, quad, kraw, ks);

    // ---- scale, bias, mask, online softmax ----------------------------------
    // fragment element (kk, r): head row quad*4 + r, key kb + kk*16 + c
    float mnew[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) mnew[r] = -INFINITY;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int key = kb + kk * 16 + c;
      const bool valid = key < hi;  // key >= lo holds for every key of a sub-tile
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float sc = sfrag[kk][r] * kscl[kk];
        if constexpr (ALIBI) sc = alibi_score(sc, slope[r], key, kstart);
        sc = valid ? sc : -INFINITY;
        sfrag[kk][r] = sc;
        mnew[r] = fmaxf(mnew[r], sc);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      mnew[r] = fmaxf(f8_row_max(mnew[r]), m_row[r]);  // finite: key kb of the sub-tile is visible
    }
    float psum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = sfrag[kk][r] == -INFINITY ? 0.f : __expf(sfrag[kk][r] - mnew[r]);
        psum[r] += p;
        // the key's V scale rides on P: one rounding, the codes stay exact
        p_s[(quad * 4 + r) * F8_PLD + kk * 16 + c] = f2bf(p * vs[kk]);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      psum[r] = f8_row_sum(psum[r]);
      const float corr = m_row[r] == -INFINITY ? 0.f : __expf(m_row[r] - mnew[r]);
      l_row[r] = l_row[r] * corr + psum[r];
      m_row[r] = mnew[r];
#pragma unroll
      for (int dg = 0; dg < D / 16; ++dg) oacc[dg][r] *= corr;
    }

    // ---- V tile -> LDS as bf16, row-major, invisible keys as zeros -----------
#pragma unroll
    for (int it = 0; it < F8_KT / RPI; ++it) {
      const int row = it * RPI + lane / CPR;
      const bool valid = kb + row < hi;
      unsigned int* dst = v_w + row * RS + (lane % CPR) * 8;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const unsigned int raw = valid ? vraw[it][w] : 0u;  // code 0 is +0.0
        dst[2 * w + 0] = f8_dequant2<false>(raw);
        dst[2 * w + 1] = f8_dequant2<true>(raw);
      }
    }
    f8_wave_lds_fence();

    // ---- O += P V -------------------------------------------------------------
    const bf16x8_f8 pf = *reinterpret_cast<const bf16x8_f8*>(p_s + c * F8_PLD + quad * 8);
#pragma unroll
    for (int dg = 0; dg < D / 16; ++dg) {
      bf16x8_f8 vf;
#pragma unroll
      for (int j = 0; j < 8; ++j) vf[j] = (short)v_s[(quad * 8 + j) * VLD + dg * 16 + c];
      oacc[dg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, vf, oacc[dg], 0, 0, 0);
    }
    f8_wave_lds_fence();  // the next sub-tile overwrites both tiles
  }

  // ---- merge the four waves' (m, l, O) through LDS, once ----------------------
  float* o_f = reinterpret_cast<float*>(v_w);  // this wave's V tile, now [16][OLD] fp32
#pragma unroll
  for (int dg = 0; dg < D / 16; ++dg) {
#pragma unroll
    for (int r = 0; r < 4; ++r) o_f[(quad * 4 + r) * OLD + dg * 16 + c] = oacc[dg][r];
  }
  if (c == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ml_lds[wid][quad * 4 + r][0] = m_row[r];
      ml_lds[wid][quad * 4 + r][1] = l_row[r];
    }
  }
  f8_block_barrier();

  // thread -> (head row, 16 of its output dims)
  const int row = threadIdx.x / 16;
  const int dcol = threadIdx.x % 16;
  if (row >= nrows) return;
  float mstar = -INFINITY;
#pragma unroll
  for (int w = 0; w < F8_WAVES; ++w) mstar = fmaxf(mstar, ml_lds[w][row][0]);
  float wgt[F8_WAVES];
  float lstar = 0.f;
#pragma unroll
  for (int w = 0; w < F8_WAVES; ++w) {
    const float mw = ml_lds[w][row][0];
    wgt[w] = mw == -INFINITY ? 0.f : __expf(mw - mstar);
    lstar += ml_lds[w][row][1] * wgt[w];
  }
  const size_t bhq = (size_t)b * Hq + head0 + row;
  if (NS > 1 && dcol == 0) {
    ws_ml[(bhq * NS + split) * 2 + 0] = mstar;
    ws_ml[(bhq * NS + split) * 2 + 1] = lstar;
  }
#pragma unroll
  for (int dg = 0; dg < D / 16; ++dg) {
    const int d = dg * 16 + dcol;
    float acc = 0.f;
#pragma unroll
    for (int w = 0; w < F8_WAVES; ++w)
      acc += reinterpret_cast<const float*>(tile_lds[w])[row * OLD + d] * wgt[w];
    if (NS > 1) ws_o[(bhq * NS + split) * D + d] = acc;
    else out[bhq * D + d].u = f2bf(lstar > 0.f ? acc / lstar : 0.f);  // no visible key: zeros
  }
}

// Second launch of the split path: out[b, hq, d] from the NS partial (m, l, O).
// One thread per output element; a split with no visible key has m = -inf and
// weight 0, a row with none at all returns zeros.
template <int D>
__global__ __launch_bounds__(F8_BLOCK) void attn_decode_fp8_merge(
    const float* __restrict__ ws_o, const float* __restrict__ ws_ml, bf16_t* __restrict__ out,
    long total /* B * Hq * D */, int NS) {
  const long idx = (long)blockIdx.x * F8_BLOCK + threadIdx.x;
  if (idx >= total) return;
  const long bhq = idx / D;
  const int d = (int)(idx % D);
  const float* ml = ws_ml + bhq * NS * 2;
  float mstar = -INFINITY;
  for (int s = 0; s < NS; ++s) mstar = fmaxf(mstar, ml[2 * s]);
  float lstar = 0.f, acc = 0.f;
  for (int s = 0; s < NS; ++s) {
    const float ms = ml[2 * s];
    if (ms == -INFINITY) continue;
    const float w = __expf(ms - mstar);
    lstar += ml[2 * s + 1] * w;
    acc += ws_o[(bhq * NS + s) * D + d] * w;
  }
  out[idx].u = f2bf(lstar > 0.f ? acc / lstar : 0.f);
}

// Key splits: a pure function of the static sizes, never of seq_lens, so a
// captured graph keeps its launch shapes.  The grouped bf16 kernel's rule (split
// while the grid has fewer than 128 blocks, never below 512 keys per split, at
// most 16), kept because the two kernels share their work split.
int fp8_num_splits(long B, long Hkv, long chunks, long S) {
  const long blocks = B * Hkv * chunks;
  const long want = (128 + blocks - 1) / blocks;
  const long room = std::max(1L, S / 512);
  return (int)std::min<long>({want, room, 16L});
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

at::Tensor attention_decode_fp8(const at::Tensor& q, const at::Tensor& k8,
                                const at::Tensor& k_scale, const at::Tensor& v8,
                                const at::Tensor& v_scale, const at::Tensor& seq_lens,
                                double scale, const c10::optional<at::Tensor>& seq_starts,
                                const c10::optional<at::Tensor>& alibi_slopes, long num_splits) {
  const char* op = "attention_decode_fp8";
  TORCH_CHECK(q.is_cuda() && q.dtype() == at::kBFloat16 && q.is_contiguous() && q.dim() == 4 &&
                  q.size(2) == 1,
              op, ": q must be contiguous bf16 [B,Hq,1,D] on the GPU");
  TORCH_CHECK(k8.is_cuda() && v8.is_cuda() && k8.dtype() == at::kByte &&
                  v8.dtype() == at::kByte && k8.dim() == 4 && k8.is_contiguous() &&
                  v8.is_contiguous() && v8.sizes() == k8.sizes() && k8.device() == q.device() &&
                  v8.device() == q.device(),
              op, ": caches must be contiguous uint8 (e4m3 codes) [B,Hkv,S,D] on q's device");
  const int B = q.size(0), Hq = q.size(1), D = q.size(3);
  const int Hkv = k8.size(1), S = k8.size(2);
  TORCH_CHECK(k8.size(0) == B && k8.size(3) == D && Hkv > 0 && Hq % Hkv == 0 && S > 0, op,
              ": cache shape does not match q");
  for (const at::Tensor* s : {&k_scale, &v_scale})
    TORCH_CHECK(s->is_cuda() && s->device() == q.device() && s->dtype() == at::kFloat &&
                    s->is_contiguous() && s->dim() == 3 && s->size(0) == B && s->size(1) == Hkv &&
                    s->size(2) == S,
                op, ": k_scale and v_scale must be contiguous fp32 [B,Hkv,S] on q's device");
  for (const at::Tensor* t : {&q, &k8, &v8})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, op,
                ": q and the caches must be 16 B aligned");
  TORCH_CHECK(seq_lens.is_cuda() && seq_lens.device() == q.device() &&
                  seq_lens.dtype() == at::kInt && seq_lens.numel() == B &&
                  seq_lens.is_contiguous(),
              op, ": seq_lens must be contiguous int32 [B] on q's device");
  TORCH_CHECK(num_splits >= 0 && num_splits <= F8_MAX_SPLITS, op, ": num_splits must be 0..",
              F8_MAX_SPLITS, ", got ", num_splits);
  const float* asl = alibi_slopes_ptr(alibi_slopes, q, Hq, op);
  const auto ss_t = optional_int_ptr(seq_starts, q, B, op, "seq_starts");
  const int* ss = ss_t.second;
  auto out = at::empty_like(q);
  if (B == 0) return out;

  const int G = Hq / Hkv;
  const int chunks = (G + F8_ROWS - 1) / F8_ROWS;
  const int NS = num_splits > 0 ? (int)num_splits : fp8_num_splits(B, Hkv, chunks, S);
  const int per = ((S + NS - 1) / NS + F8_KT - 1) / F8_KT * F8_KT;
  const long nblocks = (long)B * Hkv * chunks * NS;
  TORCH_CHECK(nblocks < (1L << 31), op, ": grid too large");
  at::Tensor ws_o, ws_ml;
  float* wo = nullptr;
  float* wml = nullptr;
  if (NS > 1) {
    ws_o = at::empty({B, Hq, NS, D}, q.options().dtype(at::kFloat));
    ws_ml = at::empty({B, Hq, NS, 2}, q.options().dtype(at::kFloat));
    wo = ws_o.data_ptr<float>();
    wml = ws_ml.data_ptr<float>();
  }
  auto stream = c10::hip::getCurrentHIPStream();
  auto qp = reinterpret_cast<const bf16_t*>(q.data_ptr());
  auto outp = reinterpret_cast<bf16_t*>(out.data_ptr());
  dispatch_head_dim(kKvFp8HeadDims, D, op, [&](auto d) {
    constexpr int kD = decltype(d)::value;
    dispatch_bool(asl != nullptr, [&](auto al) {
      attn_decode_fp8_kernel<kD, decltype(al)::value><<<(unsigned)nblocks, F8_BLOCK, 0, stream>>>(
          qp, k8.data_ptr<uint8_t>(), k_scale.data_ptr<float>(), v8.data_ptr<uint8_t>(),
          v_scale.data_ptr<float>(), seq_lens.data_ptr<int>(), ss, asl, outp, wo, wml, Hq, Hkv, S,
          chunks, NS, per, (float)scale);
    });
    if (NS > 1) {
      const long total = (long)B * Hq * kD;
      attn_decode_fp8_merge<kD><<<(unsigned)((total + F8_BLOCK - 1) / F8_BLOCK), F8_BLOCK, 0,
                                  stream>>>(wo, wml, outp, total, NS);
    }
  });
  HIP_CHECK_LAST();
  return out;
}
