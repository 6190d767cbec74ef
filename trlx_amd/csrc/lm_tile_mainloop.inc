// The 256x256x64 mainloop of the lm-head kernels, from accumulator zeroing
// through the last barrier of the K-loop.  Program text, not a header: a kernel
// includes it once, inside its body, between its per-row staging and its
// epilogue (see lm_tile.h for why it is not a function), after
//     f32x4 acc[8][4];
// and with these names in scope:
//     hidden, weight   const bf16_t* __restrict__, [N, H] and [V, H] row-major
//     N, H, V          int, H % 64 == 0
//     row0, col0       int, the tile's first row and column (tile_coord)
//     a_base, b_base   char*, the two double-buffered operand tiles in LDS
//                      (2 * TILE_BYTES each)
//     tid, lane, wave_m, wave_n   int: threadIdx.x, tid % 64, wid >> 2, wid & 3
// It leaves acc = hidden[row0 : row0 + 256] @ weight[col0 : col0 + 256]^T over
// all of H: wave (wave_m, wave_n) holds rows wave_m * 128 + i * 16 and columns
// wave_n * 64 + j * 16 in acc[i][j] (MFMA 16x16 C layout).  Rows past N - 1 /
// V - 1 repeat the last valid one.  Its own names stay inside its block.  The
// last barrier has passed at its end, so the kernel may overwrite a_base/b_base.
{
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  const int nK = H / BK;
  const int max_arow = N - 1;
  const int max_brow = V - 1;

  // ---- prologue: stage K-tile 0, drain, sync
  issue_half(weight, H, col0, max_brow, 0, b_base, 0, tid);
  issue_half(weight, H, col0 + 128, max_brow, 0, b_base, 128, tid);
  issue_half(hidden, H, row0, max_arow, 0, a_base, 0, tid);
  issue_half(hidden, H, row0 + 128, max_arow, 0, a_base, 128, tid);
  asm volatile("s_waitcnt vmcnt(0)");
  __builtin_amdgcn_s_barrier();

  // fragment addressing (byte offsets, swizzled at use)
  const int frow = lane & 15;       // row/col within a 16-wide fragment
  const int fk8 = (lane >> 4) * 8;  // k-slice start within a 32-wide K block

  bf16x8 bfrag[4];  // [j] — one half-K (32) at a time
  bf16x8 afrag[8];  // [i]

  // K-loop, minimum-2-phase shape (guide T3 recipe): per K-tile
  //   {issue next tile's 8 loads; ds_read k2=0 frags; lgkm; MFMA*32;
  //    ds_read k2=1 frags; lgkm; MFMA*32; vmcnt(0); barrier; flip}
  // ONE barrier per K-tile: intra-tile, waves only READ the same buffer
  // (no hazard), so they skew freely and each wave's ds_reads overlap the
  // other waves' MFMAs on the SIMD.  The earlier 8-barriers-per-K-tile
  // lockstep serialized the LDS and MFMA pipes CU-wide (measured 465 TF,
  // SQ_WAIT_ANY ~= MFMA cycles); this shape measured +40% (guide m230/m248).
  // The vmcnt(0) before the barrier is what makes the next tile's buffer
  // complete for every wave; without it the loop is a data race.
  for (int m = 0; m < nK; ++m) {
    const int p = m & 1;
    char* a_buf = a_base + p * TILE_BYTES;
    char* b_buf = b_base + p * TILE_BYTES;
    if (m + 1 < nK) {
      char* a_nxt = a_base + (p ^ 1) * TILE_BYTES;
      char* b_nxt = b_base + (p ^ 1) * TILE_BYTES;
      const int k0 = (m + 1) * BK;
      issue_half(weight, H, col0, max_brow, k0, b_nxt, 0, tid);
      issue_half(weight, H, col0 + 128, max_brow, k0, b_nxt, 128, tid);
      issue_half(hidden, H, row0, max_arow, k0, a_nxt, 0, tid);
      issue_half(hidden, H, row0 + 128, max_arow, k0, a_nxt, 128, tid);
    }
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int brow = wave_n * 64 + j * 16 + frow;
        bfrag[j] = *reinterpret_cast<const bf16x8*>(
            b_buf + swz(brow * ROW_BYTES + (k2 * 32 + fk8) * 2));
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int arow = wave_m * 128 + i * 16 + frow;
        afrag[i] = *reinterpret_cast<const bf16x8*>(
            a_buf + swz(arow * ROW_BYTES + (k2 * 32 + fk8) * 2));
      }
      asm volatile("s_waitcnt lgkmcnt(0)");
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] =
              __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag[i], bfrag[j], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    asm volatile("s_waitcnt vmcnt(0)");
    __builtin_amdgcn_s_barrier();
  }
}
