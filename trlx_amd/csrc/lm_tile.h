// The 256x256x64 MFMA mainloop of the lm-head kernels, once: tile constants,
// the LDS swizzle and its staging, the XCD-aware workgroup remap and (in
// lm_tile_mainloop.inc) the K-loop, plus the host prelude every kernel on this
// path shares.  lm_logprobs_v2.hip (forward) and ce_backward.hip (backward)
// include both and keep only their per-row staging and their epilogues; a new
// kernel on this path does the same and does not copy the loop.
//
// Structure (CDNA4 guide "minimum 2-phase" T3 recipe + T1/T2/T5):
//   - 256x256 output tile, BK=64, 8 waves (2M x 4N), per-wave C = 128x64
//     held in 128 accumulator VGPRs (the [N, V] logits never exist).
//   - Double-buffered A/B LDS (128 KiB dynamic) staged with 16-byte
//     global_load_lds.  Per K-tile: {issue next tile's 8 loads; ds_read
//     k2-half fragments; lgkmcnt(0); setprio(1); 32 MFMA; setprio(0)} x2,
//     then ONE vmcnt(0)+barrier.  Intra-tile, waves only READ the shared
//     buffer — no hazard — so they skew freely and one wave's ds_reads
//     overlap the others' MFMAs.  (A fully barriered 8-phase variant
//     measured 465 TF with SQ_WAIT_ANY ~= MFMA cycles: CU-wide lockstep
//     serialized the LDS and MFMA pipes.)
//   - 3-bit XOR LDS swizzle (16B-chunk ^= row&7): applied as a PRE-SWIZZLED
//     GLOBAL source column on the store side — global_load_lds ignores
//     per-lane LDS addresses (lowered readfirstlane->M0, hardware writes
//     M0 + laneId*16) — and as swizzled ds_read addresses.  The linear
//     [row][64] layout is 16-way bank conflicted (row stride 128 B);
//     measured 44M -> 6M SQ_LDS_BANK_CONFLICT.
//   - XCD-aware bijective workgroup remap (8 XCDs, each a private L2),
//     mt-major so co-resident workgroups share a B (weight) tile.
//
// Shapes: hidden [N, H] bf16 (H % 64 == 0), weight [V, H] bf16 row-major
// (NT GEMM).
#pragma once

#include <ATen/ATen.h>

#include "common.h"

namespace lm_tile {

constexpr int BM = 256;     // rows (tokens) per workgroup
constexpr int BN = 256;     // vocab columns per workgroup
constexpr int BK = 64;      // K-step
constexpr int BLOCK = 512;  // 8 waves: 2 (M) x 4 (N)

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// byte layout of one A or B buffer: [256 rows][64 cols] bf16 = 32 KiB
constexpr int TILE_BYTES = BM * BK * 2;  // 32768
constexpr int ROW_BYTES = BK * 2;        // 128
// dynamic LDS starts with [ A buf0 | A buf1 | B buf0 | B buf1 ]; what a kernel
// keeps live across the K-loop (labels, per-row data) sits above AB_BYTES
constexpr int AB_BYTES = 4 * TILE_BYTES;  // 131072

DEV int swz(int byte_off) {
  // 3-bit XOR swizzle: 16B-chunk index (byte bits 4-6) ^= row low bits
  // (byte bits 7-9).  Fragment ds_reads walk 16 consecutive rows at a fixed
  // column chunk (16-way bank conflicted in a linear [row][64] layout — row
  // stride 128 B = all 32 banks apart); the XOR spreads them across all 8
  // chunk positions -> 2 lanes/bank, which CDNA4 serves conflict-free
  // (guide: 2-way is 1.02x).  Stronger than st_16x32's single-bit XOR
  // (8-way): measured 44M SQ_LDS_BANK_CONFLICT with 1-bit vs the MFMA
  // cycles it gated.
  return byte_off ^ (((byte_off >> 7) & 7) << 4);
}

// cooperative issue of one half-tile (128 rows x 64 cols bf16) = 2
// global_load_lds instructions; gr0 = first global row, rows clamped to the
// last valid row (duplicates are masked in the epilogue).
//
// The hardware derives each lane's LDS byte as M0 + laneId*16 (the compiler
// lowers the LDS operand via readfirstlane -> M0; per-lane destination bits
// are DISCARDED), so the st_16x32 swizzle cannot be applied on the store
// side.  Instead the GLOBAL source column is pre-swizzled: the lane whose
// (implicit, linear) LDS slot l should hold the element that a swizzled
// ds_read at swz(b)=l expects loads that element directly —
// src_col = tcol ^ ((dst_row & 7) * 8)  (element-granular form of swz).
DEV void issue_half(const bf16_t* __restrict__ src, int src_stride, int gr0, int max_row, int k0,
                    char* lds_base, int dst_row0, int tid) {
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int off = c * 4096 + tid * 8;  // element offset within [128][64]
    const int trow = off >> 6;
    const int tcol = off & 63;
    const int dst_row = dst_row0 + trow;
    const int src_col = tcol ^ ((dst_row & 7) << 3);  // pre-swizzle
    const int grow = min(gr0 + trow, max_row);
    const int dst_byte = dst_row * ROW_BYTES + tcol * 2;  // linear (hw layout)
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)(src + (size_t)grow * src_stride +
                                                                k0 + src_col),
        (__attribute__((address_space(3))) unsigned int*)(lds_base + dst_byte), 16, 0, 0);
  }
}

struct TileCoord {
  int vt, mt;      // vocab (column) tile, token (row) tile
  int row0, col0;  // their first row and column
};

// This workgroup's tile on a (nV, nM) grid.
DEV TileCoord tile_coord(int nV, int nM) {
  // XCD-aware bijective remap of the flattened workgroup id (8 XCDs)
  const int nwg = nV * nM;
  int wg = blockIdx.y * gridDim.x + blockIdx.x;
  {
    const int xcd = wg % 8;
    const int q8 = nwg / 8, r8 = nwg % 8;
    wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + wg / 8;
  }
  // mt-major: consecutive workgroup ids (contiguous per XCD after the remap)
  // share one B (weight) tile and walk the M tiles, so each XCD's L2 holds
  // its hot B tile + the full A K-slice; vt-major left every resident WG
  // streaming a distinct 384 KB B tile (measured: vmem-wait dominated).
  const int vt = wg / nM;
  const int mt = wg % nM;
  return {vt, mt, mt * BM, vt * BN};
}

// The mainloop itself is lm_tile_mainloop.inc, text that a kernel includes
// inside its body, and not a function here.  As a __forceinline__ function it
// computed the same bits, but the compiler optimises an inlined function on its
// own before it inlines it and forms the fragment addresses and the loop guard
// differently from the same lines written in the kernel: the backward kernels
// came out 0.3-1.6 % slower on an MI355X (profiles/lm_tile_refactor_notes.md §1).
// Included as text, the kernels compile to the instructions they had with the
// loop written out in each of them.

// ---- host ---------------------------------------------------------------------

struct Shape {
  int N, H, V;
  int nV, nM;  // the launch grid: column tiles x row tiles
};

// The operand checks of every op on this path, all on the device: hidden
// [N, H] and weight [V, H] bf16 and contiguous, H % 64 == 0, labels [N] int64
// and contiguous.
inline Shape check_operands(const char* op, const at::Tensor& hidden, const at::Tensor& weight,
                            const at::Tensor& labels) {
  TORCH_CHECK(hidden.is_cuda() && hidden.dtype() == at::kBFloat16 && hidden.dim() == 2 &&
              hidden.is_contiguous());
  TORCH_CHECK(weight.is_cuda() && weight.dtype() == at::kBFloat16 && weight.is_contiguous());
  TORCH_CHECK(labels.is_cuda() && labels.dtype() == at::kLong && labels.is_contiguous());
  const int N = hidden.size(0);
  const int H = hidden.size(1);
  const int V = weight.size(0);
  TORCH_CHECK(weight.size(1) == H && labels.numel() == N);
  TORCH_CHECK(H % BK == 0, op, ": hidden size must be a multiple of 64");
  return {N, H, V, (V + BN - 1) / BN, (N + BM - 1) / BM};
}

// Lets Kernel be launched with Bytes (> 64 KiB) of dynamic LDS; the attribute
// is set on the kernel's first use and never again.
template <auto Kernel, int Bytes>
inline void allow_dynamic_lds() {
  static const hipError_t once =
      hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize, Bytes);
  TORCH_CHECK(once == hipSuccess, "cannot raise the dynamic LDS limit to ", Bytes,
              " bytes: ", hipGetErrorString(once));
}

}  // namespace lm_tile
