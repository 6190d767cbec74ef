// Host-side helpers shared by the attention kernel files (flash_prefill.hip,
// flash_backward.hip, attn_decode.hip): input validation and the compile-time
// dispatch from runtime (head dim, mode flags) to a kernel instantiation.
// Host only — device helpers live in common.h.
#pragma once

#include <ATen/ATen.h>

#include <string>
#include <type_traits>
#include <utility>

#include "dispatch.h"  // dispatch_bool

// ---- head dims ---------------------------------------------------------------

// The head dims each kernel family is instantiated for: the one place on the
// C++ side.  ops/__init__.py mirrors them as FLASH_HEAD_DIMS,
// SEQ2SEQ_FLASH_HEAD_DIMS, DECODE_HEAD_DIMS and SEQ2SEQ_DECODE_HEAD_DIMS.
template <int... Ds>
struct HeadDims {};
constexpr HeadDims<64, 96, 128, 256> kFlashHeadDims{};       // flash fwd + bwd
constexpr HeadDims<64, 128> kSeq2SeqFlashHeadDims{};         // their seq2seq modes
constexpr HeadDims<32, 64, 96, 128, 256> kDecodeHeadDims{};  // attention_decode, fused
constexpr HeadDims<64, 128> kSeq2SeqDecodeHeadDims{};        // s2s_decode.hip (T5 per-token step)

// ---- runtime value -> compile-time constant ------------------------------------

// f(std::integral_constant<int, D>{}) for the listed dim equal to D; any other
// D raises "<op>: head dim must be 64, 96, 128 or 256, got <D>" (the list is Ds).
// A LEFT fold: clang then instantiates f, and emits the kernels it launches, in
// list order; a right fold reverses the kernels in the code object.
template <int... Ds, typename F>
void dispatch_head_dim(HeadDims<Ds...>, int D, const char* op, F&& f) {
  const bool found = (... || (D == Ds ? (f(std::integral_constant<int, Ds>{}), true) : false));
  if (found) return;
  const int dims[] = {Ds...};
  const int n = sizeof...(Ds);
  std::string list;
  for (int i = 0; i < n; ++i)
    list += (i == 0 ? "" : i + 1 == n ? " or " : ", ") + std::to_string(dims[i]);
  TORCH_CHECK(false, op, ": head dim must be ", list, ", got ", D);
}

// The table of flash-kernel instantiations, forward and backward alike:
//   a seq2seq mode:  kSeq2SeqFlashHeadDims x the seven (causal, bias, mask)
//                    combinations other than (true, false, false), never with
//                    ALiBi (seq2seq_args checks);
//   no seq2seq mode: kFlashHeadDims x ALiBi on/off, (CAUSAL, RELB, KMASK) =
//                    (true, false, false) — the kernels' empty argument pack.
// (The rows stand in the order the kernels have in the code object.)
// f(D, ALIBI, CAUSAL, RELB, KMASK) gets integral constants.  (true, false,
// false) is passed by the second row only, so a launch lambda that chooses its
// argument list by `if constexpr (CA && !RB && !KM)` never instantiates that
// combination with the seq2seq pack.
template <typename F>
void dispatch_flash_mode(int D, bool alibi, bool s2s_any, bool causal, bool rel_bias,
                         bool key_mask, const char* op, F&& f) {
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  if (s2s_any) {
    dispatch_head_dim(kSeq2SeqFlashHeadDims, D, op, [&](auto d) {
      dispatch_bool(causal, [&](auto ca) {
        dispatch_bool(rel_bias, [&](auto rb) {
          dispatch_bool(key_mask, [&](auto km) {
            constexpr bool plain =
                decltype(ca)::value && !decltype(rb)::value && !decltype(km)::value;
            if constexpr (!plain) f(d, no, ca, rb, km);
            else TORCH_INTERNAL_ASSERT(false, op, ": seq2seq dispatch without a seq2seq mode");
          });
        });
      });
    });
    return;
  }
  dispatch_head_dim(kFlashHeadDims, D, op, [&](auto d) {
    dispatch_bool(alibi, [&](auto al) { f(d, al, yes, no, no); });
  });
}

// ---- optional inputs ------------------------------------------------------------

// validate an optional per-batch-row int32 vector (key_starts / seq_starts:
// same device as `like`, kInt, B elements) and return it contiguous — the
// caller keeps the tensor alive for the launch — with its pointer, or
// {undefined, null} when none was given.
inline std::pair<at::Tensor, const int*> optional_int_ptr(const c10::optional<at::Tensor>& opt,
                                                          const at::Tensor& like, long B,
                                                          const char* op, const char* what) {
  if (!opt.has_value()) return {at::Tensor(), nullptr};
  TORCH_CHECK(opt->device() == like.device(), op, ": ", what,
              " must live on the same device as the inputs");
  TORCH_CHECK(opt->dtype() == at::kInt && opt->numel() == B, op, ": ", what,
              " must be int32 with one element per batch row (", B, "), got ", opt->dtype(),
              " x ", opt->numel());
  at::Tensor t = opt->contiguous();
  return {t, t.data_ptr<int>()};
}

// host side: validate an optional ALiBi slope vector (fp32, contiguous, same
// device as `like`, one slope per QUERY head) and return its pointer, or null
// when no bias was given.
inline const float* alibi_slopes_ptr(const c10::optional<at::Tensor>& slopes,
                                     const at::Tensor& like, long num_q_heads,
                                     const char* op) {
  if (!slopes.has_value()) return nullptr;
  TORCH_CHECK(slopes->dtype() == at::kFloat && slopes->is_contiguous(), op,
              ": alibi_slopes must be contiguous fp32");
  TORCH_CHECK(slopes->device() == like.device(), op,
              ": alibi_slopes must live on the same device as the inputs");
  TORCH_CHECK(slopes->numel() == num_q_heads, op, ": alibi_slopes needs one slope per query head (",
              num_q_heads, "), got ", slopes->numel());
  return slopes->data_ptr<float>();
}

// host side: the seq2seq (T5) modes of the flash kernels — non-causal,
// Toeplitz relative bias, arbitrary key mask.  Validates the optional inputs
// and returns raw pointers (null = mode off).  `any` says whether a seq2seq
// instantiation is needed at all; those exist at head dims 64 and 128 only.
struct Seq2SeqArgs {
  const float* rel_bias = nullptr;  // [Hq, L] fp32
  int bias_len = 0;                 // L
  int bias_zero = 0;                // index of relative position 0
  const unsigned char* key_mask = nullptr;  // [B, Tk], nonzero = visible
  bool any = false;
};

inline Seq2SeqArgs seq2seq_args(const c10::optional<at::Tensor>& rel_bias, long bias_zero,
                                const c10::optional<at::Tensor>& key_mask, bool causal,
                                bool has_key_starts, bool has_alibi, const at::Tensor& like,
                                long B, long num_q_heads, long Tq, long Tk, long start_pos,
                                long D, const char* op) {
  Seq2SeqArgs a;
  if (rel_bias.has_value()) {
    TORCH_CHECK(!has_alibi, op, ": rel_bias and alibi_slopes are mutually exclusive");
    TORCH_CHECK(rel_bias->dtype() == at::kFloat && rel_bias->is_contiguous() &&
                    rel_bias->dim() == 2 && rel_bias->size(0) == num_q_heads,
                op, ": rel_bias must be contiguous fp32 [Hq, L]");
    TORCH_CHECK(rel_bias->device() == like.device(), op,
                ": rel_bias must live on the same device as the inputs");
    const long L = rel_bias->size(1);
    TORCH_CHECK(bias_zero - (start_pos + Tq - 1) >= 0 && bias_zero + Tk - 1 < L, op,
                ": rel_bias [Hq, ", L, "] with bias_zero ", bias_zero,
                " does not cover queries ", start_pos, "..", start_pos + Tq - 1, " x keys 0..",
                Tk - 1);
    a.rel_bias = rel_bias->data_ptr<float>();
    a.bias_len = (int)L;
    a.bias_zero = (int)bias_zero;
  }
  if (key_mask.has_value()) {
    TORCH_CHECK(!has_key_starts, op, ": key_mask and key_starts are mutually exclusive");
    TORCH_CHECK(key_mask->dtype() == at::kByte && key_mask->is_contiguous() &&
                    key_mask->dim() == 2 && key_mask->size(0) == B && key_mask->size(1) == Tk,
                op, ": key_mask must be contiguous uint8 [B, Tk]");
    TORCH_CHECK(key_mask->device() == like.device(), op,
                ": key_mask must live on the same device as the inputs");
    TORCH_CHECK(Tk > 0, op, ": key_mask needs at least one key");
    a.key_mask = key_mask->data_ptr<unsigned char>();
  }
  a.any = a.rel_bias != nullptr || a.key_mask != nullptr || !causal;
  if (a.any) {
    TORCH_CHECK(!has_alibi, op, ": key_mask / non-causal attention do not combine with alibi_slopes");
    TORCH_CHECK(D == 64 || D == 128, op,
                ": rel_bias / key_mask / non-causal attention need head dim 64 or 128, got ", D);
  }
  return a;
}
