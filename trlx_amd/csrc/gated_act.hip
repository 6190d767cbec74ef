// Gated MLP activation h = act(g) * u (SwiGLU / GeGLU), forward and backward.
//
// Plan (the op is bandwidth-bound: 3 elements moved per output forward, 5 per
// element backward, a few dozen VALU operations each):
//  - Layout by pointers.  g and u come as two base pointers with two row
//    strides, so one body serves the fused Llama tensor gu [N, 2I] (u = g + I,
//    both strides 2I) and two separate [N, I] tensors (T5).  The backward
//    writes dg and du the same way: for the fused layout they are the halves of
//    one fresh d_gate_up [N, 2I], written exactly once, never zero-filled.
//  - Work split.  A 256-thread block owns one (row, chunk of CHUNK columns)
//    tile; row and chunk come from blockIdx.x with one division per block.
//    Thread t owns the vectors t, t + 256, ... of the chunk, UNROLL = CHUNK /
//    (256 * VEC) of them, so every step of the unroll is one coalesced 4 KiB
//    row segment per input.
//  - Bytes in flight.  All UNROLL loads of every input are issued before the
//    first use: 2 * UNROLL (forward) or 3 * UNROLL (backward) independent 16 B
//    loads per lane, i.e. 16 / 24 KiB per block with VEC = 8.
//  - VEC elements are 16 B per lane (8 bf16 / 4 fp32).  That instantiation needs
//    I % VEC == 0 and 16 B-aligned bases and row strides (an odd I in the fused
//    layout puts u off alignment); the host decides, in vec_ok, and otherwise
//    launches VEC = 1.  Columns past I are predicated per vector: their loads
//    go to column 0 of the row (load_col), their stores are skipped.
//  - Math in fp32, one rounding to T per output.  act and act' share one
//    exponential (silu, gelu_new) or one erf and one exponential (gelu):
//    0.5 (1 + tanh z) is written as sigmoid(2z), which keeps its relative
//    accuracy in the negative tail where 1 + tanh cancels, and every derivative
//    is built from the sigmoid and its complement (sigmoid_pair) or the density,
//    so nothing is inf * 0 for finite g (checked to |g| = 1e4).
//  - No LDS, no atomics, no host-side values: both launches capture into graphs.
//    Offsets are 64-bit.  Resource usage: profiles/gated_act_notes.md.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include <limits>

#include "common.h"
#include "dispatch.h"

namespace {

constexpr int BLOCK = 256;
// columns per block; ops.GATED_ACT_CHUNK is the same number
constexpr int CHUNK = 4096;

// the codes of ops.ACT_CODES
constexpr int ACT_GELU = 1, ACT_GELU_NEW = 2, ACT_SILU = 4;

// VEC elements of T as one naturally aligned unit: a 16 B pack moves as one
// global_load/store_dwordx4
template <typename T, int VEC>
struct alignas(sizeof(T) * VEC) Pack {
  T v[VEC];
};

// s = sigmoid(x) and c = 1 - s from one exponential.  e = exp(-|x|) <= 1 never
// overflows, and neither s nor c comes from a subtraction, so both keep their
// relative accuracy in their tails (1 - s computed as such loses it from x ~ 4
// on, which showed in dg) and are finite for every finite x.
DEV void sigmoid_pair(float x, float& s, float& c) {
  const float e = expf(-fabsf(x));
  const float r = 1.f / (1.f + e);
  const float er = e * r;
  s = x >= 0.f ? r : er;
  c = x >= 0.f ? er : r;
}

// a = act(g), da = act'(g).  A caller that drops da pays nothing for it.
template <int ACT>
DEV void act_eval(float g, float& a, float& da) {
  static_assert(ACT == ACT_GELU || ACT == ACT_GELU_NEW || ACT == ACT_SILU, "unknown activation");
  if constexpr (ACT == ACT_SILU) {
    float s, c;
    sigmoid_pair(g, s, c);
    a = g * s;
    da = s * (1.f + g * c);
  } else if constexpr (ACT == ACT_GELU_NEW) {
    // z = k0 (g + k g^3); 0.5 (1 + tanh z) = sigmoid(2z) = s, 0.5 (1 - tanh^2 z) = 2 s (1 - s)
    constexpr float C2 = 2.f * 0.7978845608028654f, K = 0.044715f;
    const float g2 = g * g;
    float s, c;
    sigmoid_pair(C2 * g * (1.f + K * g2), s, c);
    a = g * s;
    da = s + (s * c) * (g * (C2 * (1.f + 3.f * K * g2)));
  } else {
    const float cdf = 0.5f * (1.f + erff(g * 0.7071067811865476f));
    a = g * cdf;
    da = cdf + g * (0.3989422804014327f * expf(-0.5f * g * g));
  }
}

// The tile of this block: the row's pointers are advanced by the caller, col0 is
// this thread's first column.  One division per block.
struct Tile {
  long row;
  int col0;
};
template <int VEC>
DEV Tile tile_of_block(int chunks) {
  const unsigned row = blockIdx.x / (unsigned)chunks;
  const unsigned chunk = blockIdx.x - row * (unsigned)chunks;
  return {(long)row, (int)chunk * CHUNK + (int)threadIdx.x * VEC};
}

// The column that step k of the unroll LOADS: its own, or column 0 of the row
// where that lies past I.  Every load is then in bounds and unconditional, so
// all of them issue back to back ahead of the math (under a branch per step the
// compiler waited for each step's data before issuing the next step's loads);
// the lanes past I re-read one cached vector and store nothing.
template <int VEC>
DEV int load_col(int col0, int k, int I) {
  const int col = col0 + k * BLOCK * VEC;
  return col < I ? col : 0;
}

template <typename T, int ACT, int VEC>
__global__ __launch_bounds__(BLOCK) void gated_act_fwd_kernel(
    const T* __restrict__ g, const T* __restrict__ u, T* __restrict__ h, long g_stride,
    long u_stride, int I, int chunks) {
  constexpr int UNROLL = CHUNK / (BLOCK * VEC);
  using P = Pack<T, VEC>;
  const Tile t = tile_of_block<VEC>(chunks);
  g += t.row * g_stride;
  u += t.row * u_stride;
  h += t.row * (long)I;
  P gv[UNROLL], uv[UNROLL];
#pragma unroll
  for (int k = 0; k < UNROLL; ++k) {
    const int col = load_col<VEC>(t.col0, k, I);
    gv[k] = *reinterpret_cast<const P*>(g + col);
    uv[k] = *reinterpret_cast<const P*>(u + col);
  }
#pragma unroll
  for (int k = 0; k < UNROLL; ++k) {
    const int col = t.col0 + k * BLOCK * VEC;
    if (col < I) {
      P hv;
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        float a, da;
        act_eval<ACT>(ScalarIO<T>::load(&gv[k].v[i]), a, da);
        ScalarIO<T>::store(&hv.v[i], a * ScalarIO<T>::load(&uv[k].v[i]));
      }
      *reinterpret_cast<P*>(h + col) = hv;
    }
  }
}

// dg = dh u act'(g), du = dh act(g)
template <typename T, int ACT, int VEC>
__global__ __launch_bounds__(BLOCK) void gated_act_bwd_kernel(
    const T* __restrict__ g, const T* __restrict__ u, const T* __restrict__ dh,
    T* __restrict__ dg, T* __restrict__ du, long g_stride, long u_stride, long dg_stride,
    long du_stride, int I, int chunks) {
  constexpr int UNROLL = CHUNK / (BLOCK * VEC);
  using P = Pack<T, VEC>;
  const Tile t = tile_of_block<VEC>(chunks);
  g += t.row * g_stride;
  u += t.row * u_stride;
  dh += t.row * (long)I;
  dg += t.row * dg_stride;
  du += t.row * du_stride;
  P gv[UNROLL], uv[UNROLL], hv[UNROLL];
#pragma unroll
  for (int k = 0; k < UNROLL; ++k) {
    const int col = load_col<VEC>(t.col0, k, I);
    gv[k] = *reinterpret_cast<const P*>(g + col);
    uv[k] = *reinterpret_cast<const P*>(u + col);
    hv[k] = *reinterpret_cast<const P*>(dh + col);
  }
#pragma unroll
  for (int k = 0; k < UNROLL; ++k) {
    const int col = t.col0 + k * BLOCK * VEC;
    if (col < I) {
      P dgv, duv;
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        float a, da;
        act_eval<ACT>(ScalarIO<T>::load(&gv[k].v[i]), a, da);
        const float d = ScalarIO<T>::load(&hv[k].v[i]);
        ScalarIO<T>::store(&dgv.v[i], d * ScalarIO<T>::load(&uv[k].v[i]) * da);
        ScalarIO<T>::store(&duv.v[i], d * a);
      }
      *reinterpret_cast<P*>(dg + col) = dgv;
      *reinterpret_cast<P*>(du + col) = duv;
    }
  }
}

// ---- host ----------------------------------------------------------------------

template <typename F>
void dispatch_dtype(const at::Tensor& x, const char* op, F&& f) {
  if (x.scalar_type() == at::kBFloat16) f(bf16_t{});
  else if (x.scalar_type() == at::kFloat) f(float{});
  else TORCH_CHECK(false, op, ": dtype must be bfloat16 or float32, got ", x.dtype());
}

// f(std::integral_constant<int, ACT>{}) for the three gated activations
template <typename F>
void dispatch_act(long act, const char* op, F&& f) {
  if (act == ACT_SILU) f(std::integral_constant<int, ACT_SILU>{});
  else if (act == ACT_GELU_NEW) f(std::integral_constant<int, ACT_GELU_NEW>{});
  else if (act == ACT_GELU) f(std::integral_constant<int, ACT_GELU>{});
  else TORCH_CHECK(false, op, ": activation code must be gelu (1), gelu_new (2) or silu (4), got ",
                   act);
}

// g and u as the kernels read them: element pointers (void: the dtype is
// dispatched later) and row strides in elements
struct GatedView {
  const at::Tensor *g, *u;  // u == g for the fused layout
  long N, I, u_offset;      // u's first element, in elements from its tensor's data
  bool fused;
};

GatedView check_g_u(const at::Tensor& g, const c10::optional<at::Tensor>& u, const char* op) {
  auto rows_ok = [](const at::Tensor& t) { return t.dim() == 2 && t.stride(1) == 1; };
  TORCH_CHECK(g.is_cuda() && rows_ok(g), op,
              ": gate must be a 2-D tensor on the GPU with a last-dim stride of 1");
  if (!u.has_value()) {
    TORCH_CHECK(g.size(1) % 2 == 0, op, ": a fused [N, 2I] gate_up needs an even last dim, got ",
                g.size(1));
    return {&g, &g, g.size(0), g.size(1) / 2, g.size(1) / 2, true};
  }
  TORCH_CHECK(rows_ok(*u) && u->sizes() == g.sizes() && u->dtype() == g.dtype() &&
                  u->device() == g.device(),
              op, ": up must have gate's shape, dtype and device and a last-dim stride of 1");
  return {&g, &*u, g.size(0), g.size(1), 0, false};
}

// The 16 B-per-lane instantiation is legal when the rows split into whole
// vectors and every base pointer and row stride keeps them 16 B-aligned.
bool vec_ok(long I, size_t vec, size_t elt, std::initializer_list<const void*> bases,
            std::initializer_list<long> row_strides) {
  bool ok = I % (long)vec == 0;
  for (const void* p : bases) ok = ok && reinterpret_cast<uintptr_t>(p) % 16 == 0;
  for (long s : row_strides) ok = ok && (s * (long)elt) % 16 == 0;
  return ok;
}

// blocks of one launch: N rows x chunks of CHUNK columns
int grid_of(long N, int chunks, const char* op) {
  const long blocks = N * chunks;
  TORCH_CHECK(blocks <= std::numeric_limits<int>::max(), op, ": ", N, " rows x ", chunks,
              " column chunks exceed the grid limit");
  return (int)blocks;
}

}  // namespace

// h [N, I] = act(g) * u.  Without u, g is the fused [N, 2I] (gate | up).
at::Tensor gated_act_fwd(const at::Tensor& g, const c10::optional<at::Tensor>& u, long act) {
  const char* op = "gated_act_fwd";
  const GatedView v = check_g_u(g, u, op);
  auto h = at::empty({v.N, v.I}, g.options());
  if (v.N == 0 || v.I == 0) return h;
  TORCH_CHECK(v.I <= std::numeric_limits<int>::max() - CHUNK, op, ": I too large");
  const int chunks = (int)((v.I + CHUNK - 1) / CHUNK);
  const int grid = grid_of(v.N, chunks, op);
  const long gs = v.g->stride(0), us = v.u->stride(0);
  auto stream = c10::hip::getCurrentHIPStream();
  dispatch_dtype(g, op, [&](auto t) {
    using T = decltype(t);
    constexpr int VEC = 16 / sizeof(T);
    const T* gp = static_cast<const T*>(v.g->data_ptr());
    const T* up = static_cast<const T*>(v.u->data_ptr()) + v.u_offset;
    T* hp = static_cast<T*>(h.data_ptr());
    dispatch_act(act, op, [&](auto a) {
      dispatch_bool(vec_ok(v.I, VEC, sizeof(T), {gp, up, hp}, {gs, us}), [&](auto vec) {
        gated_act_fwd_kernel<T, decltype(a)::value, decltype(vec)::value ? VEC : 1>
            <<<grid, BLOCK, 0, stream>>>(gp, up, hp, gs, us, (int)v.I, chunks);
      });
    });
  });
  HIP_CHECK_LAST();
  return h;
}

// {d_gate_up [N, 2I]} for the fused layout, {dg, du} for separate tensors
std::vector<at::Tensor> gated_act_bwd(const at::Tensor& g, const c10::optional<at::Tensor>& u,
                                      const at::Tensor& dh, long act) {
  const char* op = "gated_act_bwd";
  const GatedView v = check_g_u(g, u, op);
  TORCH_CHECK(dh.dim() == 2 && dh.size(0) == v.N && dh.size(1) == v.I && dh.is_contiguous() &&
                  dh.dtype() == g.dtype() && dh.device() == g.device(),
              op, ": dh must be a contiguous [N, I] tensor of gate's dtype and device");
  std::vector<at::Tensor> out;
  if (v.fused) out = {at::empty({v.N, 2 * v.I}, g.options())};
  else out = {at::empty({v.N, v.I}, g.options()), at::empty({v.N, v.I}, g.options())};
  if (v.N == 0 || v.I == 0) return out;
  TORCH_CHECK(v.I <= std::numeric_limits<int>::max() - CHUNK, op, ": I too large");
  const int chunks = (int)((v.I + CHUNK - 1) / CHUNK);
  const int grid = grid_of(v.N, chunks, op);
  const long gs = v.g->stride(0), us = v.u->stride(0);
  const long ds = v.fused ? 2 * v.I : v.I;  // row stride of dg and of du
  auto stream = c10::hip::getCurrentHIPStream();
  dispatch_dtype(g, op, [&](auto t) {
    using T = decltype(t);
    constexpr int VEC = 16 / sizeof(T);
    const T* gp = static_cast<const T*>(v.g->data_ptr());
    const T* up = static_cast<const T*>(v.u->data_ptr()) + v.u_offset;
    const T* dhp = static_cast<const T*>(dh.data_ptr());
    T* dgp = static_cast<T*>(out[0].data_ptr());
    T* dup = v.fused ? dgp + v.I : static_cast<T*>(out[1].data_ptr());
    dispatch_act(act, op, [&](auto a) {
      dispatch_bool(vec_ok(v.I, VEC, sizeof(T), {gp, up, dhp, dgp, dup}, {gs, us, ds}),
                    [&](auto vec) {
        gated_act_bwd_kernel<T, decltype(a)::value, decltype(vec)::value ? VEC : 1>
            <<<grid, BLOCK, 0, stream>>>(gp, up, dhp, dgp, dup, gs, us, ds, ds, (int)v.I,
                                         chunks);
      });
    });
  });
  HIP_CHECK_LAST();
  return out;
}
