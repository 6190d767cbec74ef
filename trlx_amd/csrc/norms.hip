// Fused RMSNorm / LayerNorm fwd+bwd, with and without the fused residual add
// (SURVEY.md K3).
//
// One forward template and one backward template; RMS or LayerNorm (LN), the
// bias, the residual add and who owns a row are compile-time switches, and an
// off switch leaves no instruction behind.  Rows are grid-strided, loads are
// 16 B/lane (guide Guideline 13) with a scalar tail for H % 8, accumulation is
// fp32 and the row statistics are saved for the backward.
// Weight/bias gradients: each block accumulates its rows into an LDS partial
// (every column owned by exactly one thread, race-free), writes it as one
// [H] slab with plain stores, and the host reduces the [grid, H] slabs with
// sum(0).  No atomics anywhere, so the gradients are bit-reproducible.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include "common.h"
#include "dispatch.h"

namespace {

constexpr int BLOCK = 256;
constexpr int NWAVES = BLOCK / WAVE;

// ---- who owns a row ------------------------------------------------------------

// A 256-thread block per row: LDS reduction, a barrier per row.  Any H.
struct BlockRows {
  static constexpr int LANES = BLOCK;  // threads striding one row
  static constexpr int ROWS = 1;       // rows per block
  DEV static int lane() { return threadIdx.x; }
  DEV static int slot() { return 0; }
  DEV static float sum(float v) {
    __shared__ float rbuf[NWAVES];
    return block_sum<NWAVES>(v, rbuf);
  }
  DEV static void end_row() { __syncthreads(); }
};

// A wave per row, for small/medium H (decode shapes: H=768, N=128 rows).  The
// block policy gives each 768-wide row a 256-thread block: only 96 lanes load
// anything and the row pays two LDS+barrier reduction rounds.  Here each WAVE
// owns a row — shfl-only reductions, zero LDS, zero barriers — and a block
// carries NWAVES independent rows.
// Measured (bench cycle profile pf3): layernorm_fwd was 8.1 us/call avg and
// the top non-GEMM kernel at 185 ms of a 3.1 s GPU cycle.
struct WaveRows {
  static constexpr int LANES = WAVE;
  static constexpr int ROWS = NWAVES;
  DEV static int lane() { return threadIdx.x % WAVE; }
  DEV static int slot() { return threadIdx.x / WAVE; }
  DEV static float sum(float v) { return wave_sum(v); }
  DEV static void end_row() {}
};

// ---- forward -------------------------------------------------------------------

// y = norm(x) * w (+ b); rstd gets the row's 1/rms (RMS) or 1/std (LN), mean
// the row mean (LN only; RMS passes null, as it does for b).
// HAS_RES: s = x + res is written to sout and normalized (residual-add
// fused into the norm — saves the separate elementwise-add kernel and one
// full stream read per residual connection; profile r01: adds were 5.6% of
// cycle kernels).
template <typename T, typename Rows, bool LN, bool HAS_BIAS, bool HAS_RES>
__global__ void norm_fwd_kernel(const T* __restrict__ x, const T* __restrict__ res,
                                const T* __restrict__ w, const T* __restrict__ b,
                                T* __restrict__ y, T* __restrict__ sout,
                                float* __restrict__ mean, float* __restrict__ rstd, int H,
                                float eps, long N) {
  static_assert(LN || !HAS_BIAS, "RMSNorm has no bias");
  const int slot = Rows::slot();
  const int lane = Rows::lane();
  const int H8 = H & ~7;
  for (long row = (long)blockIdx.x * Rows::ROWS + slot; row < N;
       row += (long)gridDim.x * Rows::ROWS) {
    const T* xr = x + (size_t)row * H;
    const T* rr = HAS_RES ? res + (size_t)row * H : nullptr;
    T* sr = HAS_RES ? sout + (size_t)row * H : nullptr;
    T* yr = y + (size_t)row * H;
    float s = 0.f, ss = 0.f;
    for (int base = lane * 8; base < H8; base += Rows::LANES * 8) {
      float v[8];
      load8<T>(xr + base, v);
      if (HAS_RES) {
        float rv[8];
        load8<T>(rr + base, rv);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] += rv[i];
        store8<T>(sr + base, v);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (LN) s += v[i];
        ss += v[i] * v[i];
      }
    }
    for (int i = H8 + lane; i < H; i += Rows::LANES) {
      float xi = ScalarIO<T>::load(xr + i);
      if (HAS_RES) {
        xi += ScalarIO<T>::load(rr + i);
        ScalarIO<T>::store(sr + i, xi);
      }
      if (LN) s += xi;
      ss += xi * xi;
    }
    if (LN) s = Rows::sum(s);
    ss = Rows::sum(ss);
    float mu = 0.f, istd;
    if (LN) {
      mu = s / H;
      const float var = fmaxf(ss / H - mu * mu, 0.f);
      istd = rsqrtf(var + eps);
    } else {
      istd = rsqrtf(ss / H + eps);
    }
    if (lane == 0) {
      if (LN) mean[row] = mu;
      rstd[row] = istd;
    }
    const T* src = HAS_RES ? sr : xr;
    for (int base = lane * 8; base < H8; base += Rows::LANES * 8) {
      float v[8], wv[8], bv[8];
      load8<T>(src + base, v);
      load8<T>(w + base, wv);
      if (HAS_BIAS) load8<T>(b + base, bv);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float o = LN ? (v[i] - mu) * istd * wv[i] : v[i] * istd * wv[i];
        if (HAS_BIAS) o += bv[i];
        v[i] = o;
      }
      store8<T>(yr + base, v);
    }
    for (int i = H8 + lane; i < H; i += Rows::LANES) {
      float o = ScalarIO<T>::load(src + i);
      o = (LN ? (o - mu) * istd : o * istd) * ScalarIO<T>::load(w + i);
      if (HAS_BIAS) o += ScalarIO<T>::load(b + i);
      ScalarIO<T>::store(yr + i, o);
    }
    Rows::end_row();
  }
}

// ---- backward ------------------------------------------------------------------

// Block per row.  dw (and db for LN) are [gridDim.x, H] slabs.
// HAS_DRES: dres (the residual-stream gradient from downstream) is added
// into dx — the backward half of the fused residual+norm.
template <typename T, bool LN, bool HAS_DRES>
__global__ void norm_bwd_kernel(const T* __restrict__ x, const T* __restrict__ w,
                                const float* __restrict__ mean, const float* __restrict__ rstd,
                                const T* __restrict__ dy, const T* __restrict__ dres,
                                T* __restrict__ dx, float* __restrict__ dw,
                                float* __restrict__ db, int H, long N) {
  extern __shared__ float acc[];  // H floats of dw, then (LN) H floats of db
  __shared__ float rbuf[NWAVES];
  float* dwacc = acc;
  float* dbacc = acc + H;
  for (int i = threadIdx.x; i < H; i += BLOCK) {
    dwacc[i] = 0.f;
    if (LN) dbacc[i] = 0.f;
  }
  __syncthreads();
  const int H8 = H & ~7;
  for (long row = blockIdx.x; row < N; row += gridDim.x) {
    const T* xr = x + (size_t)row * H;
    const T* dyr = dy + (size_t)row * H;
    const T* drr = HAS_DRES ? dres + (size_t)row * H : nullptr;
    T* dxr = dx + (size_t)row * H;
    const float mu = LN ? mean[row] : 0.f;
    const float r = rstd[row];
    float s1 = 0.f, s2 = 0.f;  // sum(dy*w), sum(dy*w*xhat) (RMS: sum(dy*w*x))
    for (int base = threadIdx.x * 8; base < H8; base += BLOCK * 8) {
      float xv[8], dv[8], wv[8];
      load8<T>(xr + base, xv);
      load8<T>(dyr + base, dv);
      load8<T>(w + base, wv);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float dyw = dv[i] * wv[i];
        if (LN) s1 += dyw;
        s2 += LN ? dyw * (xv[i] - mu) * r : dyw * xv[i];
      }
    }
    for (int i = H8 + threadIdx.x; i < H; i += BLOCK) {
      float dyw = ScalarIO<T>::load(dyr + i) * ScalarIO<T>::load(w + i);
      if (LN) s1 += dyw;
      s2 += LN ? dyw * (ScalarIO<T>::load(xr + i) - mu) * r : dyw * ScalarIO<T>::load(xr + i);
    }
    if (LN) s1 = block_sum<NWAVES>(s1, rbuf) / H;
    s2 = block_sum<NWAVES>(s2, rbuf);
    s2 = LN ? s2 / H : s2 * r * r * r / H;
    for (int base = threadIdx.x * 8; base < H8; base += BLOCK * 8) {
      float xv[8], dv[8], wv[8], o[8];
      load8<T>(xr + base, xv);
      load8<T>(dyr + base, dv);
      load8<T>(w + base, wv);
      float ev[8];
      if (HAS_DRES) load8<T>(drr + base, ev);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float xhat = (xv[i] - mu) * r;  // LN only
        o[i] = LN ? r * (dv[i] * wv[i] - s1 - xhat * s2) : r * wv[i] * dv[i] - s2 * xv[i];
        if (HAS_DRES) o[i] += ev[i];
        dwacc[base + i] += LN ? dv[i] * xhat : dv[i] * xv[i] * r;
        if (LN) dbacc[base + i] += dv[i];
      }
      store8<T>(dxr + base, o);
    }
    for (int i = H8 + threadIdx.x; i < H; i += BLOCK) {
      const float dv = ScalarIO<T>::load(dyr + i);
      const float xv = ScalarIO<T>::load(xr + i);
      const float wv = ScalarIO<T>::load(w + i);
      const float xhat = (xv - mu) * r;  // LN only
      float o = LN ? r * (dv * wv - s1 - xhat * s2) : r * wv * dv - s2 * xv;
      if (HAS_DRES) o += ScalarIO<T>::load(drr + i);
      ScalarIO<T>::store(dxr + i, o);
      dwacc[i] += LN ? dv * xhat : dv * xv * r;
      if (LN) dbacc[i] += dv;
    }
    __syncthreads();
  }
  // per-block partial slabs (plain stores; v1's atomicAdd tail serialized
  // ~2048 adds per address = ~60 us/launch — profile r02)
  for (int i = threadIdx.x; i < H; i += BLOCK) {
    dw[(size_t)blockIdx.x * H + i] = dwacc[i];
    if (LN) db[(size_t)blockIdx.x * H + i] = dbacc[i];
  }
}

// ---- host ----------------------------------------------------------------------

constexpr long GRID_MAX = 2048;
// wave-per-row dispatch bound: a wave covers H<=4096 in <=8 vec8 strides
constexpr int WAVE_H_MAX = 4096;

// f(T{}) with T the kernels' element type for x's dtype, as dispatch_bool
// hands over a constant; ptr<T>(t) is t's data as T* (null for no tensor).
template <typename F>
void dispatch_dtype(const at::Tensor& x, const char* op, F&& f) {
  if (x.scalar_type() == at::kBFloat16) f(bf16_t{});
  else if (x.scalar_type() == at::kFloat) f(float{});
  else TORCH_CHECK(false, op, ": dtype must be bfloat16 or float32, got ", x.dtype());
}
template <typename T>
T* ptr(const at::Tensor& t) {
  return t.defined() ? static_cast<T*>(t.data_ptr()) : nullptr;
}

// an optional [N, H] companion of x (res, dres): contiguous, x's dtype and shape
at::Tensor like_x(const c10::optional<at::Tensor>& t, const at::Tensor& x, const char* op,
                  const char* what) {
  if (!t.has_value()) return at::Tensor();
  TORCH_CHECK(t->sizes() == x.sizes() && t->dtype() == x.dtype() && t->device() == x.device(),
              op, ": ", what, " must have x's shape, dtype and device");
  return t->contiguous();
}

void check_x_w(const at::Tensor& x, const at::Tensor& w, const char* op) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous(), op,
              ": x must be a contiguous [N, H] tensor on the GPU");
  TORCH_CHECK(w.dtype() == x.dtype() && w.numel() == x.size(1) && w.device() == x.device(), op,
              ": weight must have x's dtype and H elements");
}

// {y, [mean,] rstd, [s]}: mean for LN, s = x + res when res is given
template <bool LN>
std::vector<at::Tensor> norm_fwd(const char* op, const at::Tensor& x, const at::Tensor& w,
                                 const c10::optional<at::Tensor>& b, double eps,
                                 const c10::optional<at::Tensor>& res) {
  check_x_w(x, w, op);
  const long N = x.size(0);
  const int H = x.size(1);
  auto y = at::empty_like(x);
  auto rstd = at::empty({N}, x.options().dtype(at::kFloat));
  auto mean = LN ? at::empty_like(rstd) : at::Tensor();
  auto rc = like_x(res, x, op, "res");
  auto sout = rc.defined() ? at::empty_like(x) : at::Tensor();
  at::Tensor wc = w.contiguous(), bc;
  if (b.has_value()) {
    TORCH_CHECK(b->dtype() == x.dtype() && b->numel() == H && b->device() == x.device(), op,
                ": bias must have x's dtype and H elements");
    bc = b->contiguous();
  }
  if (N > 0) {
    auto stream = c10::hip::getCurrentHIPStream();
    dispatch_dtype(x, op, [&](auto t) {
      using T = decltype(t);
      dispatch_bool(H <= WAVE_H_MAX, [&](auto wave) {
        using Rows = std::conditional_t<decltype(wave)::value, WaveRows, BlockRows>;
        const int grid = (int)std::min<long>((N + Rows::ROWS - 1) / Rows::ROWS, GRID_MAX);
        dispatch_bool(bc.defined(), [&](auto hb) {
          dispatch_bool(rc.defined(), [&](auto hr) {
            norm_fwd_kernel<T, Rows, LN, LN && decltype(hb)::value, decltype(hr)::value>
                <<<grid, BLOCK, 0, stream>>>(ptr<const T>(x), ptr<const T>(rc), ptr<const T>(wc),
                                             ptr<const T>(bc), ptr<T>(y), ptr<T>(sout),
                                             ptr<float>(mean), ptr<float>(rstd), H, (float)eps,
                                             N);
          });
        });
      });
    });
    HIP_CHECK_LAST();
  }
  std::vector<at::Tensor> out{y};
  if (LN) out.push_back(mean);
  out.push_back(rstd);
  if (rc.defined()) out.push_back(sout);
  return out;
}

// {dx, dw, [db]}: db for LN; mean is undefined for RMS
template <bool LN>
std::vector<at::Tensor> norm_bwd(const char* op, const at::Tensor& x, const at::Tensor& w,
                                 const at::Tensor& mean, const at::Tensor& rstd,
                                 const at::Tensor& dy, const c10::optional<at::Tensor>& dres) {
  check_x_w(x, w, op);
  const long N = x.size(0);
  const int H = x.size(1);
  TORCH_CHECK(H <= 16384, op, ": H too large for LDS accumulation");
  auto is_stat = [&](const at::Tensor& s) {
    return s.defined() && s.device() == x.device() && s.dtype() == at::kFloat &&
           s.numel() == N && s.is_contiguous();
  };
  TORCH_CHECK(is_stat(rstd) && (!LN || is_stat(mean)), op,
              ": the saved statistics must be contiguous fp32 with one element per row (", N, ")");
  auto dyc = like_x(dy, x, op, "dy");
  auto drc = like_x(dres, x, op, "dres");
  auto dx = at::empty_like(x);
  auto wc = w.contiguous();
  const int grid = (int)std::min<long>(N, GRID_MAX);
  // one [H] slab per block; without rows nothing is launched and the sum is zero
  auto slabs = [&] {
    const auto fp32 = x.options().dtype(at::kFloat);
    return N == 0 ? at::zeros({1, H}, fp32) : at::empty({grid, H}, fp32);
  };
  auto dwp = slabs();
  auto dbp = LN ? slabs() : at::Tensor();
  if (N > 0) {
    auto stream = c10::hip::getCurrentHIPStream();
    const size_t lds = (LN ? 2 : 1) * (size_t)H * sizeof(float);
    dispatch_dtype(x, op, [&](auto t) {
      using T = decltype(t);
      dispatch_bool(drc.defined(), [&](auto hd) {
        norm_bwd_kernel<T, LN, decltype(hd)::value><<<grid, BLOCK, lds, stream>>>(
            ptr<const T>(x), ptr<const T>(wc), ptr<const float>(mean), ptr<const float>(rstd),
            ptr<const T>(dyc), ptr<const T>(drc), ptr<T>(dx), ptr<float>(dwp), ptr<float>(dbp), H,
            N);
      });
    });
    HIP_CHECK_LAST();
  }
  std::vector<at::Tensor> out{dx, dwp.sum(0).to(w.dtype())};
  if (LN) out.push_back(dbp.sum(0).to(w.dtype()));
  return out;
}

}  // namespace

std::vector<at::Tensor> rmsnorm_fwd(const at::Tensor& x, const at::Tensor& w, double eps,
                                    const c10::optional<at::Tensor>& res) {
  return norm_fwd<false>("rmsnorm_fwd", x, w, c10::nullopt, eps, res);
}

std::vector<at::Tensor> rmsnorm_bwd(const at::Tensor& x, const at::Tensor& w,
                                    const at::Tensor& invr, const at::Tensor& dy,
                                    const c10::optional<at::Tensor>& dres) {
  return norm_bwd<false>("rmsnorm_bwd", x, w, at::Tensor(), invr, dy, dres);
}

std::vector<at::Tensor> layernorm_fwd(const at::Tensor& x, const at::Tensor& w,
                                      const c10::optional<at::Tensor>& b, double eps,
                                      const c10::optional<at::Tensor>& res) {
  return norm_fwd<true>("layernorm_fwd", x, w, b, eps, res);
}

std::vector<at::Tensor> layernorm_bwd(const at::Tensor& x, const at::Tensor& w,
                                      const at::Tensor& mean, const at::Tensor& invstd,
                                      const at::Tensor& dy,
                                      const c10::optional<at::Tensor>& dres) {
  return norm_bwd<true>("layernorm_bwd", x, w, mean, invstd, dy, dres);
}
