// Grouped-query decode attention: the query heads that share one KV head are
// served by ONE block, so a block's K/V rows leave global memory once instead
// of once per query head (attn_decode.hip launches a block per QUERY head), and
// the group's scores are a matrix product.
//
//   q [B, Hq, 1, D] vs cache [B, Hkv, S, D] (bf16, contiguous), G = Hq / Hkv >= 2,
//   visible keys of row b: [seq_starts[b], seq_lens[b]).
//
// Work split.  A 256-thread block owns (batch row b, KV head hkv, chunk of up to
// 16 query heads of that group, key split s of NS).  The chunk's heads are the 16
// M-rows of v_mfma_f32_16x16x32_bf16; rows past the group (G < 16, or the tail
// chunk of G > 16) hold q = 0 and are never stored.  Split s covers the keys
// [s * per, (s + 1) * per) of the ALLOCATED length S (per = ceil(S / NS) rounded
// up to 32), cut to the row's visible range; an empty cut contributes (m, l, O)
// = (-inf, 0, 0).  The four waves take the 32-key sub-tiles of that range
// round-robin and meet only after the loop: no block barrier inside it.
//
// Data movement, per wave and 32-key sub-tile:
//   Q   resident bf16 A-fragments, UNSCALED (row = head, k-slice = (lane>>4)*8);
//       `scale` multiplies the fp32 score fragment, q is never rounded twice.
//   K   the B operand straight from row-major global memory: lane (c, quad)
//       loads 16 B of key c at d = dch*32 + quad*8 (flash_bwd_dbias.hip's
//       load), D/32 loads for each of the two 16-key halves.  The next
//       sub-tile's K is requested as soon as the MFMAs have read this one's.
//   P   fp32 probabilities rounded to bf16 and relaid C-fragment -> A-fragment
//       through the wave's P tile [16][32 + 8] shorts (flash_prefill.hip).
//   V   P V needs 8 consecutive KEYS of one d per lane — V transposed.  The
//       tile is loaded coalesced, 16 B per lane (lane -> key id / (D/8), dims
//       8 * (id % (D/8))), rows of keys outside the visible range replaced by
//       zeros (so 0 * stale cache never makes a NaN), and stored ROW-MAJOR
//       [32 keys][D/2 + 1 words]; the B fragment is then gathered with eight
//       16-bit reads v[quad*8 + j][dg*16 + c].
// Every K and V element of the block's key range is loaded from global memory
// exactly once.  Every row index (key, query head) is clamped absolutely into
// its tensor before the load; clamped rows are masked.
//
// LDS layout and banks (32 banks of 4 B).  Per wave: the V tile, 32 rows of
// RS = D/2 + 1 words, then the P tile, 16 rows of 20 words.
//   V reads:  lane (c, quad) reads the half-word at word
//             (quad*8 + j) * RS + dg*8 + c/2.  RS = 1 (mod 4) gives 8*RS = 8
//             (mod 32): the four quads start 8 banks apart and each covers 8
//             consecutive words (two lanes share a word, a broadcast), so the
//             64 lanes touch each of the 32 banks with ONE word: conflict-free.
//   V writes: an odd row stride is only 4-byte aligned, so a lane's 16 B go out
//             as four 32-bit writes to word row * RS + 4 * chunk + w.  At D=128
//             a wave writes 4 rows x 16 chunks, at D=64 8 rows x 8 chunks; in
//             both the 64 lanes fall two to a bank, the minimum for 64 words.
//   P tile:   written one bf16 at a time (row quad*4 + r, column kk*16 + c),
//             read as 16 B at word 20 * c + 4 * quad: 20c mod 32 takes eight
//             distinct multiples of 4 over any 8 consecutive lanes, which is
//             the unit a 128-bit read is served in: conflict-free.
//   Merge:    after the loop a wave's V tile holds its fp32 O [16][D + 2] (the
//             same 16 * (D + 2) words); (m, l) go to a small array of their own.
//
// Merge.  The four waves' (m, l, O) meet through LDS once.  NS == 1: the block
// divides by l and writes bf16 output.  NS > 1: it writes the fp32 (m, l, O) of
// its split to a workspace [B, Hq, NS, ...] and attn_decode_gqa_merge combines
// them — two plain launches, no atomics, no counters, nothing that depends on
// seq_lens, so both capture into the decode hipGraph.
//
// Registers / LDS per instantiation: profiles/gqa_decode_notes.md.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>

#include "attn_host.h"

// Device code of this file is compiled without the packed fp32 VALU instructions
// (as flash_bwd_dbias.hip): every fp32 step after the MFMA is one scalar-per-lane
// instruction.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "common.h"

namespace {

constexpr int GQ_BLOCK = 256;
constexpr int GQ_WAVES = GQ_BLOCK / WAVE;
constexpr int GQ_ROWS = 16;   // query heads per block: the MFMA M dimension
constexpr int GQ_KT = 32;     // keys per wave sub-tile: the MFMA K dimension of P V
constexpr int GQ_PLD = GQ_KT + 8;               // P tile row stride in shorts
constexpr int GQ_PWORDS = GQ_ROWS * GQ_PLD / 2;  // P tile in words
constexpr int GQ_MAX_SPLITS = 64;

constexpr int gq_rs(int D) { return D / 2 + 1; }             // V tile row stride in words
constexpr int gq_vwords(int D) { return GQ_KT * gq_rs(D); }  // == GQ_ROWS * (D + 2)

typedef __attribute__((ext_vector_type(8))) short bf16x8_gq;
typedef __attribute__((ext_vector_type(4))) float f32x4_gq;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_gq;

// orders a wave's own LDS writes and reads of its private tiles (the LDS
// executes one wave's accesses in order; this keeps the compiler from moving
// them across)
DEV void gq_wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// The functions of this file carry a target attribute of their own (above), so
// the HIP header's __shfl_xor and __syncthreads would stay out-of-line calls;
// the builtins below are what those expand to.
//
// all-reduce over the 16 lanes of a DPP row (the lanes that share `quad`, i.e.
// one C-fragment row): xor 1, xor 2, mirror within 8, mirror within 16
template <int CTRL>
DEV float gq_dpp(float v) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
DEV float gq_row_max(float v) {
  v = fmaxf(v, gq_dpp<0xB1>(v));   // quad_perm [1,0,3,2]
  v = fmaxf(v, gq_dpp<0x4E>(v));   // quad_perm [2,3,0,1]
  v = fmaxf(v, gq_dpp<0x141>(v));  // row_half_mirror
  return fmaxf(v, gq_dpp<0x140>(v));  // row_mirror
}
DEV float gq_row_sum(float v) {
  v += gq_dpp<0xB1>(v);
  v += gq_dpp<0x4E>(v);
  v += gq_dpp<0x141>(v);
  return v + gq_dpp<0x140>(v);
}

DEV void gq_block_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// the two 16-key B fragments of the sub-tile starting at key kb: one 16 B load
// per (half, 32-dim chunk), key row clamped absolutely into [0, S)
template <int D>
DEV void gq_load_k(const bf16_t* __restrict__ kbase, int kb, int S, int c, int quad,
                   bf16x8_gq (&kf)[2][D / 32]) {
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const int row = min(max(kb + kk * 16 + c, 0), S - 1);
#pragma unroll
    for (int dch = 0; dch < D / 32; ++dch)
      kf[kk][dch] =
          *reinterpret_cast<const bf16x8_gq*>(kbase + (size_t)row * D + dch * 32 + quad * 8);
  }
}

template <int D, bool ALIBI>
__global__ __launch_bounds__(GQ_BLOCK) void attn_decode_gqa_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ kc, const bf16_t* __restrict__ vc,
    const int* __restrict__ seq_lens, const int* __restrict__ seq_starts,
    const float* __restrict__ alibi_slopes /* [Hq], read iff ALIBI */,
    bf16_t* __restrict__ out /* [B, Hq, D], written iff NS == 1 */,
    float* __restrict__ ws_o /* [B, Hq, NS, D], written iff NS > 1 */,
    float* __restrict__ ws_ml /* [B, Hq, NS, 2] */, int Hq, int Hkv, int S, int chunks, int NS,
    int per, float scale) {
  constexpr int RS = gq_rs(D);
  constexpr int VWORDS = gq_vwords(D);
  constexpr int VLD = 2 * RS;     // V tile row stride in shorts
  constexpr int OLD = D + 2;      // O tile row stride in floats (merge)
  constexpr int CPR = D / 8;      // 16 B chunks per V row
  constexpr int RPI = WAVE / CPR;  // V rows a wave loads per instruction
  static_assert(VWORDS == GQ_ROWS * OLD, "the O tile of the merge reuses the V tile");

  // block -> (b, hkv, chunk, split), split fastest
  const int split = blockIdx.x % NS;
  const int chunk = (blockIdx.x / NS) % chunks;
  const int bh = blockIdx.x / (NS * chunks);
  const int b = bh / Hkv;
  const int hkv = bh % Hkv;
  const int G = Hq / Hkv;
  const int head0 = hkv * G + chunk * GQ_ROWS;      // query head of M-row 0
  const int nrows = min(G - chunk * GQ_ROWS, GQ_ROWS);  // M-rows that are query heads

  // visible keys of this block: split range cut to [kstart, len), all inside [0, S)
  const int len = min(seq_lens[b], S);
  const int kstart = max(seq_starts ? seq_starts[b] : 0, 0);
  const int lo = max(split * per, kstart);
  const int hi = min(min((split + 1) * per, S), len);
  const int ntiles = hi > lo ? (hi - lo + GQ_KT - 1) / GQ_KT : 0;

  const int lane = threadIdx.x % WAVE;
  const int wid = threadIdx.x / WAVE;
  const int c = lane & 15;
  const int quad = lane >> 4;

  // 16 B aligned: the P tile is read back as 128-bit A-fragments
  __shared__ __attribute__((aligned(16))) unsigned int tile_lds[GQ_WAVES][VWORDS + GQ_PWORDS];
  __shared__ float ml_lds[GQ_WAVES][GQ_ROWS][2];
  unsigned int* v_w = tile_lds[wid];
  const unsigned short* v_s = reinterpret_cast<const unsigned short*>(v_w);
  unsigned short* p_s = reinterpret_cast<unsigned short*>(v_w + VWORDS);

  const bf16_t* kbase = kc + ((size_t)b * Hkv + hkv) * (size_t)S * D;
  const bf16_t* vbase = vc + ((size_t)b * Hkv + hkv) * (size_t)S * D;

  // Q A-fragments: row c is query head head0 + c, zero past the group
  bf16x8_gq q_frag[D / 32];
  {
    const int hq = min(head0 + c, Hq - 1);
    const bf16_t* qp = q + ((size_t)b * Hq + hq) * D + quad * 8;
    const bf16x8_gq zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int dch = 0; dch < D / 32; ++dch) {
      const bf16x8_gq v8 = *reinterpret_cast<const bf16x8_gq*>(qp + dch * 32);
      q_frag[dch] = c < nrows ? v8 : zero;
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
  f32x4_gq oacc[D / 16];  // O fragments [16 heads x 16 d] per d-group
#pragma unroll
  for (int dg = 0; dg < D / 16; ++dg) oacc[dg] = {0.f, 0.f, 0.f, 0.f};

  bf16x8_gq kf[2][D / 32];
  if (wid < ntiles) gq_load_k<D>(kbase, lo + wid * GQ_KT, S, c, quad, kf);

  for (int t = wid; t < ntiles; t += GQ_WAVES) {
    const int kb = lo + t * GQ_KT;  // first key of the sub-tile

    // ---- V tile: coalesced 16 B loads, issued before the score MFMAs -------
    u32x4_gq vraw[GQ_KT / RPI];
#pragma unroll
    for (int it = 0; it < GQ_KT / RPI; ++it) {
      const int key = kb + it * RPI + lane / CPR;
      const int row = min(max(key, 0), S - 1);
      vraw[it] =
          *reinterpret_cast<const u32x4_gq*>(vbase + (size_t)row * D + (lane % CPR) * 8);
    }

    // ---- S = Q K^T: two [16 heads x 16 keys] fragments ----------------------
    f32x4_gq sfrag[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      f32x4_gq acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int dch = 0; dch < D / 32; ++dch)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(q_frag[dch], kf[kk][dch], acc, 0, 0, 0);
      sfrag[kk] = acc;
    }
    // this wave's next sub-tile, into the registers the MFMAs have just read
    if (t + GQ_WAVES < ntiles) gq_load_k<D>(kbase, kb + GQ_WAVES * GQ_KT, S, c, quad, kf);

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
        float sc = sfrag[kk][r] * scale;
        if constexpr (ALIBI) sc = alibi_score(sc, slope[r], key, kstart);
        sc = valid ? sc : -INFINITY;
        sfrag[kk][r] = sc;
        mnew[r] = fmaxf(mnew[r], sc);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      mnew[r] = fmaxf(gq_row_max(mnew[r]), m_row[r]);  // finite: key kb of the sub-tile is visible
    }
    float psum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = sfrag[kk][r] == -INFINITY ? 0.f : __expf(sfrag[kk][r] - mnew[r]);
        psum[r] += p;
        p_s[(quad * 4 + r) * GQ_PLD + kk * 16 + c] = f2bf(p);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      psum[r] = gq_row_sum(psum[r]);
      const float corr = m_row[r] == -INFINITY ? 0.f : __expf(m_row[r] - mnew[r]);
      l_row[r] = l_row[r] * corr + psum[r];
      m_row[r] = mnew[r];
#pragma unroll
      for (int dg = 0; dg < D / 16; ++dg) oacc[dg][r] *= corr;
    }

    // ---- V tile -> LDS, row-major, invisible keys as zeros -------------------
#pragma unroll
    for (int it = 0; it < GQ_KT / RPI; ++it) {
      const int row = it * RPI + lane / CPR;
      const bool valid = kb + row < hi;
      unsigned int* dst = v_w + row * RS + (lane % CPR) * 4;
#pragma unroll
      for (int w = 0; w < 4; ++w) dst[w] = valid ? vraw[it][w] : 0u;
    }
    gq_wave_lds_fence();

    // ---- O += P V -------------------------------------------------------------
    const bf16x8_gq pf = *reinterpret_cast<const bf16x8_gq*>(p_s + c * GQ_PLD + quad * 8);
#pragma unroll
    for (int dg = 0; dg < D / 16; ++dg) {
      bf16x8_gq vf;
#pragma unroll
      for (int j = 0; j < 8; ++j) vf[j] = (short)v_s[(quad * 8 + j) * VLD + dg * 16 + c];
      oacc[dg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, vf, oacc[dg], 0, 0, 0);
    }
    gq_wave_lds_fence();  // the next sub-tile overwrites both tiles
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
  gq_block_barrier();

  // thread -> (head row, 16 of its output dims)
  const int row = threadIdx.x / 16;
  const int dcol = threadIdx.x % 16;
  if (row >= nrows) return;
  float mstar = -INFINITY;
#pragma unroll
  for (int w = 0; w < GQ_WAVES; ++w) mstar = fmaxf(mstar, ml_lds[w][row][0]);
  float wgt[GQ_WAVES];
  float lstar = 0.f;
#pragma unroll
  for (int w = 0; w < GQ_WAVES; ++w) {
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
    for (int w = 0; w < GQ_WAVES; ++w)
      acc += reinterpret_cast<const float*>(tile_lds[w])[row * OLD + d] * wgt[w];
    if (NS > 1) ws_o[(bhq * NS + split) * D + d] = acc;
    else out[bhq * D + d].u = f2bf(lstar > 0.f ? acc / lstar : 0.f);  // no visible key: zeros
  }
}

// Second launch of the split path: out[b, hq, d] from the NS partial (m, l, O).
// One thread per output element; a split with no visible key has m = -inf and
// weight 0, a row with none at all returns zeros.
template <int D>
__global__ __launch_bounds__(GQ_BLOCK) void attn_decode_gqa_merge(
    const float* __restrict__ ws_o, const float* __restrict__ ws_ml, bf16_t* __restrict__ out,
    long total /* B * Hq * D */, int NS) {
  const long idx = (long)blockIdx.x * GQ_BLOCK + threadIdx.x;
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
// captured graph keeps its launch shapes.  Split only while the grid has fewer
// than 128 blocks (one per two CUs of the 256: from there on one more split
// measured no faster, and slower past 256 blocks), and never below 512 keys per
// split (four sub-tiles for each of the four waves: 256-key splits measured
// slower than 512-key ones at the same shape).  The timings this was chosen
// from are in profiles/gqa_decode_notes.md.
int gqa_num_splits(long B, long Hkv, long chunks, long S) {
  const long blocks = B * Hkv * chunks;
  const long want = (128 + blocks - 1) / blocks;
  const long room = std::max(1L, S / 512);
  return (int)std::min<long>({want, room, 16L});
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

at::Tensor attention_decode_gqa(const at::Tensor& q, const at::Tensor& kc, const at::Tensor& vc,
                                const at::Tensor& seq_lens, double scale,
                                const c10::optional<at::Tensor>& seq_starts,
                                const c10::optional<at::Tensor>& alibi_slopes, long num_splits) {
  const char* op = "attention_decode_gqa";
  TORCH_CHECK(q.is_cuda() && q.dtype() == at::kBFloat16 && q.is_contiguous() && q.dim() == 4 &&
                  q.size(2) == 1,
              op, ": q must be contiguous bf16 [B,Hq,1,D] on the GPU");
  TORCH_CHECK(kc.is_cuda() && vc.is_cuda() && kc.dtype() == at::kBFloat16 &&
                  vc.dtype() == at::kBFloat16 && kc.dim() == 4 && kc.is_contiguous() &&
                  vc.is_contiguous() && vc.sizes() == kc.sizes() && kc.device() == q.device() &&
                  vc.device() == q.device(),
              op, ": caches must be contiguous bf16 [B,Hkv,S,D] on q's device");
  const int B = q.size(0), Hq = q.size(1), D = q.size(3);
  const int Hkv = kc.size(1), S = kc.size(2);
  TORCH_CHECK(kc.size(0) == B && kc.size(3) == D && Hkv > 0 && Hq % Hkv == 0 && S > 0, op,
              ": cache shape does not match q");
  const int G = Hq / Hkv;
  TORCH_CHECK(G >= 2, op, ": needs at least 2 query heads per KV head, got ", G);
  TORCH_CHECK(seq_lens.is_cuda() && seq_lens.device() == q.device() &&
                  seq_lens.dtype() == at::kInt && seq_lens.numel() == B &&
                  seq_lens.is_contiguous(),
              op, ": seq_lens must be contiguous int32 [B] on q's device");
  TORCH_CHECK(num_splits >= 0 && num_splits <= GQ_MAX_SPLITS, op, ": num_splits must be 0..",
              GQ_MAX_SPLITS, ", got ", num_splits);
  const float* asl = alibi_slopes_ptr(alibi_slopes, q, Hq, op);
  const auto ss_t = optional_int_ptr(seq_starts, q, B, op, "seq_starts");
  const int* ss = ss_t.second;
  auto out = at::empty_like(q);
  if (B == 0) return out;

  const int chunks = (G + GQ_ROWS - 1) / GQ_ROWS;
  const int NS = num_splits > 0 ? (int)num_splits : gqa_num_splits(B, Hkv, chunks, S);
  const int per = ((S + NS - 1) / NS + GQ_KT - 1) / GQ_KT * GQ_KT;
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
  auto kp = reinterpret_cast<const bf16_t*>(kc.data_ptr());
  auto vp = reinterpret_cast<const bf16_t*>(vc.data_ptr());
  auto outp = reinterpret_cast<bf16_t*>(out.data_ptr());
  auto sl = seq_lens.data_ptr<int>();
  dispatch_head_dim(kGqaDecodeHeadDims, D, op, [&](auto d) {
    constexpr int kD = decltype(d)::value;
    dispatch_bool(asl != nullptr, [&](auto al) {
      attn_decode_gqa_kernel<kD, decltype(al)::value><<<(unsigned)nblocks, GQ_BLOCK, 0, stream>>>(
          qp, kp, vp, sl, ss, asl, outp, wo, wml, Hq, Hkv, S, chunks, NS, per, (float)scale);
    });
    if (NS > 1) {
      const long total = (long)B * Hq * kD;
      attn_decode_gqa_merge<kD><<<(unsigned)((total + GQ_BLOCK - 1) / GQ_BLOCK), GQ_BLOCK, 0,
                                  stream>>>(wo, wml, outp, total, NS);
    }
  });
  HIP_CHECK_LAST();
  return out;
}
