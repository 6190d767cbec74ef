// Fused LoRA adapter path: the two rank-r GEMMs around a frozen linear, bf16.
//
//   lora_shrink:  T[N, r] = alpha * X[N, C] @ Wt[r, C]^T          (tall x skinny)
//   lora_expand:  Y[N, C] = Base[N, C] + alpha * T[N, r] @ Wt[C, r]^T
//
// The "weight" is always [cols, inner] row-major, so its MFMA fragment is one
// 16 B load per lane.  Forward: T = shrink(x, A), y = expand(base(x), T, B,
// scaling) in place.  Backward: dT = shrink(dY, B^T, scaling), dX = expand(dY @
// W, dT, A^T) in place; the transposes are r x C tensors made on the host.
// 1 <= r <= 64, C % 8 == 0 (every row is read in 16 B pieces).
//
// lora_shrink_kernel<NT, SPLIT> - bound by the one read of X.
//  - A 256-thread block owns one 16-row group of X (and one of `nsplit` column
//    ranges of it).  Its four waves take the 128-column chunks of the range
//    round-robin; a wave holds all NT = ceil(r / 16) accumulators of
//    v_mfma_f32_16x16x32_bf16, so it loads each X element once whatever r is.
//    The X A-fragment comes straight from global memory with the lane layout of
//    skinny_gemm.hip (lane l: row l & 15, k-slice (l >> 4) * 8): a chunk is 256
//    contiguous bytes per row, two whole cache lines.
//  - Wt fragments are read through L1 / L2, not staged in LDS: the waves of a
//    block split C, so no two of them ever want the same Wt element and a
//    block-level stage would only copy it once more.  Reuse is across blocks
//    (every row group reads all of Wt, <= 2.8 MB, which stays in L2).
//  - Two chunks are in flight per wave: the 4 + 4 NT loads of the next chunk
//    are issued before the MFMAs of the present one (two register stages, the
//    loop is unrolled by two so no stage is copied).  Every load is
//    unconditional: a lane past the end of the range reads column 0 of its row
//    and its X fragment is zeroed before the MFMA.  C % 8 == 0 makes a lane's
//    16 B vector whole or absent.  Rows past N and rank rows past r are clamped
//    on load and never stored.
//  - The waves' partial tiles meet in LDS once (red[4][NT][64] float4, 4 KB per
//    NT; every access is one 16 B word per lane at consecutive addresses, a
//    contiguous 1 KB per instruction, conflict-free on any bank count) and wave
//    j adds tile j in wave order 0..3.  With nsplit > 1 (small N) the blocks
//    write fp32 slabs [nsplit, N, r] and lora_shrink_finish adds them in split
//    order; no atomics, and nsplit is a pure function of (N, C), so results are
//    bit-identical from run to run and the launches capture into graphs.
//  - T is written with 2 B stores from the C-fragment (16 lanes cover 32
//    contiguous bytes).  T is r / C of the bytes of X; not worth a relay.
//
// lora_expand_kernel<KS, RVEC> - bound by one read and one write of Y.
//  - Operands swapped: Wt rows are the M side, token rows the N side, so the
//    C-fragment gives a lane four consecutive COLUMNS of one row.  The M index a
//    of MFMA m (m = 0..3) is bound to column (a >> 2) * 16 + m * 4 + (a & 3) of
//    a 64-column tile; lane (row = l & 15, q = l >> 4) then holds the 16
//    consecutive columns q * 16 .. q * 16 + 15 of its row over the four MFMAs.
//    Base is loaded and Y stored as two 16 B pieces per lane, 128 contiguous
//    bytes per row per wave - one cache line - and every element is read and
//    written by the same lane, so Y may alias Base.  No LDS, no barrier.
//  - A wave keeps its 16 rows of T resident as KS = 1 or 2 B-fragments (rank
//    zero-padded to 32 or 64 in registers) and walks a strip of column tiles.
//    The four waves of a block are four consecutive row groups on the same
//    strip, so a Wt tile is fetched from L2 once per block and hit in L1 after.
//  - The loads of the next tile (2 of Base, 4 KS of Wt) are issued before the
//    MFMAs and the epilogue of the present one; two register stages, unrolled
//    by two.  A piece past C re-reads the row's last piece and is dropped, a
//    tile past the strip re-reads the strip's last tile.
//  - r % 8 != 0 (RVEC off) reads the rank fragments element by element; rows of
//    T and Wt are then not 16 B-aligned.  No model uses such a rank.
//  - Grid: (ceil(N / 64), strips); the strip count is a pure function of (N, C)
//    aiming at EXPAND_TARGET_BLOCKS blocks, so N = 8192 and N = 128 both spread
//    over the machine.
//
// fp32 accumulation, one rounding per output.  alpha is the adapter's constant
// scaling, a launch argument; nothing data-dependent comes from the host.
// Registers, LDS and scratch per instantiation: profiles/lora_notes.md.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <limits>

#include "common.h"
#include "dispatch.h"

namespace {

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

constexpr int BLOCK = 256;
constexpr int MAX_RANK = 64;  // ops.LORA_MAX_RANK
// shrink: columns of one wave's chunk (four k-steps of 32)
constexpr int CHUNK = 128;
// shrink: a block's column range is at least this long before X is split across
// blocks (ops.LORA_SPLIT_COLS), and splitting stops at this many blocks
constexpr int SPLIT_COLS = 1024;
constexpr int SHRINK_TARGET_BLOCKS = 512;
constexpr int MAX_SPLIT = 8;
// expand: columns of one tile (four MFMAs of 16) and the block count aimed at
constexpr int TILE = 64;
constexpr int EXPAND_TARGET_BLOCKS = 2048;

DEV bf16x8_t zero8() { return bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0}; }

DEV bf16x8_t load16(const bf16_t* p) { return *reinterpret_cast<const bf16x8_t*>(p); }

// ---- shrink ---------------------------------------------------------------------

template <int NT>
struct ShrinkStage {
  bf16x8_t x[4];
  bf16x8_t w[4][NT];
};

// Chunk c of the row: four k-steps.  A lane whose vector lies past col_end reads
// column 0 instead (shrink_mma zeroes its X fragment).
template <int NT>
DEV void shrink_load(ShrinkStage<NT>& st, const bf16_t* xp, const bf16_t* (&wp)[NT], int c,
                     int k8, int col_end) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int col = c * CHUNK + s * 32 + k8;
    const int lc = col < col_end ? col : 0;
    st.x[s] = load16(xp + lc);
#pragma unroll
    for (int j = 0; j < NT; ++j) st.w[s][j] = load16(wp[j] + lc);
  }
}

template <int NT>
DEV void shrink_mma(const ShrinkStage<NT>& st, f32x4_t (&acc)[NT], int c, int k8, int col_end) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int col = c * CHUNK + s * 32 + k8;
    const bf16x8_t x = col < col_end ? st.x[s] : zero8();
#pragma unroll
    for (int j = 0; j < NT; ++j)
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x, st.w[s][j], acc[j], 0, 0, 0);
  }
}

// SPLIT: out is fp32 slabs [gridDim.y, N, r], unscaled; else bf16 T [N, r].
template <int NT, bool SPLIT>
__global__ __launch_bounds__(BLOCK) void lora_shrink_kernel(
    const bf16_t* __restrict__ X, const bf16_t* __restrict__ Wt, void* __restrict__ out, int N,
    int C, int r, float alpha, int chunks_per_split) {
  __shared__ f32x4_t red[4][NT][WAVE];
  const int lane = threadIdx.x % WAVE;
  const int wid = threadIdx.x / WAVE;
  const int row0 = blockIdx.x * 16;
  const int chunks = (C + CHUNK - 1) / CHUNK;
  const int c0 = blockIdx.y * chunks_per_split;
  const int c1 = min(c0 + chunks_per_split, chunks);
  const int col_end = min(C, c1 * CHUNK);
  const int k8 = (lane >> 4) * 8;

  const bf16_t* xp = X + (size_t)min(row0 + (lane & 15), N - 1) * C;
  const bf16_t* wp[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) wp[j] = Wt + (size_t)min(j * 16 + (lane & 15), r - 1) * C;

  f32x4_t acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // the wave's chunks are c0 + wid, c0 + wid + 4, ...; two stages in flight
  ShrinkStage<NT> a, b;
  int c = c0 + wid;
  shrink_load<NT>(a, xp, wp, c, k8, col_end);
  for (; c < c1; c += 8) {
    shrink_load<NT>(b, xp, wp, c + 4, k8, col_end);
    shrink_mma<NT>(a, acc, c, k8, col_end);
    shrink_load<NT>(a, xp, wp, c + 8, k8, col_end);
    shrink_mma<NT>(b, acc, c + 4, k8, col_end);
  }

#pragma unroll
  for (int j = 0; j < NT; ++j) red[wid][j][lane] = acc[j];
  __syncthreads();
  // wave j finishes rank tile j, adding the four waves' partials in wave order
  if (wid >= NT) return;
  f32x4_t sum = red[0][wid][lane];
#pragma unroll
  for (int w = 1; w < 4; ++w) sum += red[w][wid][lane];

  // C-fragment: row = (lane >> 4) * 4 + i, column = lane & 15
  const int col = wid * 16 + (lane & 15);
  if (col >= r) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = row0 + (lane >> 4) * 4 + i;
    if (row >= N) continue;
    if (SPLIT) {
      static_cast<float*>(out)[((size_t)blockIdx.y * N + row) * r + col] = sum[i];
    } else {
      ScalarIO<bf16_t>::store(static_cast<bf16_t*>(out) + (size_t)row * r + col, alpha * sum[i]);
    }
  }
}

// T = alpha * (slab 0 + slab 1 + ...), in split order
__global__ __launch_bounds__(BLOCK) void lora_shrink_finish(const float* __restrict__ slabs,
                                                            bf16_t* __restrict__ T, long n,
                                                            int nsplit, float alpha) {
  const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  float v = slabs[i];
  for (int s = 1; s < nsplit; ++s) v += slabs[(size_t)s * n + i];
  ScalarIO<bf16_t>::store(T + i, alpha * v);
}

// ---- expand ---------------------------------------------------------------------

// Elements k .. k + 7 of a rank-r row, zeros from r on.  RVEC (r % 8 == 0): one
// 16 B load, whole or absent (an absent one re-reads elements 0..7).
template <bool RVEC>
DEV bf16x8_t load_rank8(const bf16_t* rowp, int k, int r) {
  if constexpr (RVEC) {
    const bf16x8_t v = load16(rowp + (k < r ? k : 0));
    return k < r ? v : zero8();
  } else {
    bf16x8_t v;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int idx = k + e;
      const short u = (short)rowp[idx < r ? idx : 0].u;
      v[e] = idx < r ? u : (short)0;
    }
    return v;
  }
}

template <int KS>
struct ExpandStage {
  bf16x8_t base[2];
  bf16x8_t w[4][KS];
};

// Tile t of the strip [.., t1): the lane's two Base pieces and its four Wt
// A-fragments per k-step.  A tile past the strip re-reads tile t1 - 1, a piece
// past C the row's last piece; neither is used.
template <int KS, bool RVEC>
DEV void expand_load(ExpandStage<KS>& st, const bf16_t* bp, const bf16_t* Wt, int t, int t1,
                     int lane, int C, int r) {
  const int col0 = min(t, t1 - 1) * TILE;
  const int q = lane >> 4;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int col = col0 + q * 16 + p * 8;
    st.base[p] = load16(bp + (col < C ? col : C - 8));
  }
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int a = lane & 15;
    const int wrow = min(col0 + (a >> 2) * 16 + m * 4 + (a & 3), C - 1);
#pragma unroll
    for (int s = 0; s < KS; ++s)
      st.w[m][s] = load_rank8<RVEC>(Wt + (size_t)wrow * r, s * 32 + q * 8, r);
  }
}

template <int KS>
DEV void expand_tile(const ExpandStage<KS>& st, const bf16x8_t (&tb)[KS], bf16_t* yp, int t,
                     int lane, int C, bool row_ok, float alpha) {
  f32x4_t acc[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    acc[m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s)
      acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(st.w[m][s], tb[s], acc[m], 0, 0, 0);
  }
  // acc[m][i] is column q * 16 + m * 4 + i of the tile, for row lane & 15
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int col = t * TILE + (lane >> 4) * 16 + p * 8;
    if (!row_ok || col >= C) continue;
    bf16x8_t y;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float b = bf2f((unsigned short)st.base[p][e]);
      y[e] = (short)f2bf(__builtin_fmaf(alpha, acc[p * 2 + (e >> 2)][e & 3], b));
    }
    *reinterpret_cast<bf16x8_t*>(yp + col) = y;
  }
}

// Y may be Base: no __restrict__ on the two.
template <int KS, bool RVEC>
__global__ __launch_bounds__(BLOCK) void lora_expand_kernel(
    const bf16_t* Base, const bf16_t* __restrict__ T, const bf16_t* __restrict__ Wt, bf16_t* Y,
    int N, int C, int r, float alpha, int tiles_per_strip) {
  const int lane = threadIdx.x % WAVE;
  const int row0 = (blockIdx.x * 4 + threadIdx.x / WAVE) * 16;
  if (row0 >= N) return;  // no barrier below
  const int tiles = (C + TILE - 1) / TILE;
  const int t0 = blockIdx.y * tiles_per_strip;
  const int t1 = min(t0 + tiles_per_strip, tiles);
  const int row = row0 + (lane & 15);
  const bool row_ok = row < N;
  const size_t lrow = (size_t)min(row, N - 1);
  const bf16_t* bp = Base + lrow * C;
  bf16_t* yp = Y + lrow * C;

  bf16x8_t tb[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) tb[s] = load_rank8<RVEC>(T + lrow * r, s * 32 + (lane >> 4) * 8, r);

  ExpandStage<KS> a, b;
  expand_load<KS, RVEC>(a, bp, Wt, t0, t1, lane, C, r);
  for (int t = t0; t < t1; t += 2) {
    expand_load<KS, RVEC>(b, bp, Wt, t + 1, t1, lane, C, r);
    expand_tile<KS>(a, tb, yp, t, lane, C, row_ok, alpha);
    expand_load<KS, RVEC>(a, bp, Wt, t + 2, t1, lane, C, r);
    if (t + 1 < t1) expand_tile<KS>(b, tb, yp, t + 1, lane, C, row_ok, alpha);
  }
}

// ---- host -----------------------------------------------------------------------

bool aligned16(const at::Tensor& t) { return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0; }

void check_bf16_matrix(const at::Tensor& t, const at::Tensor& like, const char* op,
                       const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device() && t.scalar_type() == at::kBFloat16 &&
                  t.dim() == 2 && t.is_contiguous(),
              op, ": ", name, " must be a contiguous 2-D bfloat16 tensor on the GPU");
}

const bf16_t* cptr(const at::Tensor& t) { return static_cast<const bf16_t*>(t.data_ptr()); }

// f(std::integral_constant<int, n>{}) for n in 1..4
template <typename F>
void dispatch_1_to_4(int n, F&& f) {
  if (n == 1) f(std::integral_constant<int, 1>{});
  else if (n == 2) f(std::integral_constant<int, 2>{});
  else if (n == 3) f(std::integral_constant<int, 3>{});
  else f(std::integral_constant<int, 4>{});
}

}  // namespace

// T [N, r] = alpha * x [N, C] @ wt [r, C]^T
at::Tensor lora_shrink(const at::Tensor& x, const at::Tensor& wt, double alpha) {
  const char* op = "lora_shrink";
  check_bf16_matrix(x, x, op, "x");
  check_bf16_matrix(wt, x, op, "wt");
  const long N = x.size(0), C = x.size(1), r = wt.size(0);
  TORCH_CHECK(wt.size(1) == C, op, ": wt must be [r, ", C, "], got ", wt.sizes());
  TORCH_CHECK(r >= 1 && r <= MAX_RANK, op, ": rank must be in 1..", MAX_RANK, ", got ", r);
  TORCH_CHECK(C >= 8 && C % 8 == 0, op, ": the inner dim must be a positive multiple of 8, got ", C);
  TORCH_CHECK(aligned16(x) && aligned16(wt), op, ": x and wt must be 16 B-aligned");
  TORCH_CHECK(N <= std::numeric_limits<int>::max() - 16 &&
                  C <= std::numeric_limits<int>::max() - 16 * CHUNK,
              op, ": shape too large");
  auto T = at::empty({N, r}, x.options());
  if (N == 0) return T;

  const int groups = (int)((N + 15) / 16);
  const int chunks = (int)((C + CHUNK - 1) / CHUNK);
  const int nsplit = (int)std::clamp<long>(
      std::min<long>(SHRINK_TARGET_BLOCKS / groups, C / SPLIT_COLS), 1, MAX_SPLIT);
  const int per_split = (chunks + nsplit - 1) / nsplit;
  const dim3 grid(groups, nsplit);
  auto stream = c10::hip::getCurrentHIPStream();
  dispatch_1_to_4((int)(r + 15) / 16, [&](auto nt) {
    constexpr int NT = decltype(nt)::value;
    if (nsplit == 1) {
      lora_shrink_kernel<NT, false><<<grid, BLOCK, 0, stream>>>(
          cptr(x), cptr(wt), T.data_ptr(), (int)N, (int)C, (int)r, (float)alpha, per_split);
    } else {
      auto slabs = at::empty({nsplit, N, r}, x.options().dtype(at::kFloat));
      lora_shrink_kernel<NT, true><<<grid, BLOCK, 0, stream>>>(
          cptr(x), cptr(wt), slabs.data_ptr(), (int)N, (int)C, (int)r, (float)alpha, per_split);
      const long n = N * r;
      lora_shrink_finish<<<(unsigned)((n + BLOCK - 1) / BLOCK), BLOCK, 0, stream>>>(
          slabs.data_ptr<float>(), static_cast<bf16_t*>(T.data_ptr()), n, nsplit, (float)alpha);
    }
  });
  HIP_CHECK_LAST();
  return T;
}

// out [N, C] = base [N, C] + alpha * t [N, r] @ wt [C, r]^T; out may be base
at::Tensor lora_expand(const at::Tensor& base, const at::Tensor& t, const at::Tensor& wt,
                       double alpha, at::Tensor out) {
  const char* op = "lora_expand";
  check_bf16_matrix(base, base, op, "base");
  check_bf16_matrix(t, base, op, "t");
  check_bf16_matrix(wt, base, op, "wt");
  check_bf16_matrix(out, base, op, "out");
  const long N = base.size(0), C = base.size(1), r = t.size(1);
  TORCH_CHECK(out.sizes() == base.sizes(), op, ": out must have base's shape");
  TORCH_CHECK(t.size(0) == N && wt.size(0) == C && wt.size(1) == r, op, ": t must be [", N,
              ", r] and wt [", C, ", r], got ", t.sizes(), " and ", wt.sizes());
  TORCH_CHECK(r >= 1 && r <= MAX_RANK, op, ": rank must be in 1..", MAX_RANK, ", got ", r);
  TORCH_CHECK(C >= 8 && C % 8 == 0, op, ": the outer dim must be a positive multiple of 8, got ", C);
  const bool rvec = r % 8 == 0;
  TORCH_CHECK(aligned16(base) && aligned16(out) && (!rvec || (aligned16(t) && aligned16(wt))), op,
              ": base, out, t and wt must be 16 B-aligned");
  TORCH_CHECK(N <= std::numeric_limits<int>::max() - 64 &&
                  C <= std::numeric_limits<int>::max() - 4 * TILE,
              op, ": shape too large");
  if (N == 0) return out;

  const int row_blocks = (int)((N + 63) / 64);
  const int tiles = (int)((C + TILE - 1) / TILE);
  const int want = std::clamp(EXPAND_TARGET_BLOCKS / row_blocks, 1, std::min(tiles, 65535));
  const int per_strip = (tiles + want - 1) / want;
  const dim3 grid(row_blocks, (tiles + per_strip - 1) / per_strip);
  auto stream = c10::hip::getCurrentHIPStream();
  dispatch_bool(r > 32, [&](auto two) {
    dispatch_bool(rvec, [&](auto vec) {
      lora_expand_kernel<decltype(two)::value ? 2 : 1, decltype(vec)::value>
          <<<grid, BLOCK, 0, stream>>>(cptr(base), cptr(t), cptr(wt),
                                       static_cast<bf16_t*>(out.data_ptr()), (int)N, (int)C,
                                       (int)r, (float)alpha, per_strip);
    });
  });
  HIP_CHECK_LAST();
  return out;
}
