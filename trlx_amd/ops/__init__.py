"""Custom-op dispatch: HIP/CDNA4 kernels on GPU, torch reference on CPU.

Policy (enforced): on a GPU (ROCm) device the hand-written gfx950 kernels are
the ONLY path — if the compiled extension is missing the op raises instead of
silently falling back to eager PyTorch.  On CPU the pure-torch reference
implementations run so the full framework is testable without hardware.

Set ``TRLX_AMD_ALLOW_EAGER=1`` to permit the eager fallback on GPU (debugging
only; never in benchmarks).
"""

import os
from typing import Optional, Tuple

import torch

from . import reference

# Head dims the attention kernels are instantiated for — the one source of
# truth for every dispatch gate (models/nn/transformer.py, generation.py); the
# head-dim lists at the top of csrc/attn_host.h are the same sets.
FLASH_HEAD_DIMS = (64, 96, 128, 256)  # flash_prefill / flash_attention (fwd + bwd)
DECODE_HEAD_DIMS = (32, 64, 96, 128, 256)  # attention_decode / fused_decode_attention

# Which of FLASH_HEAD_DIMS the model takes BY DEFAULT, per direction.  The
# project's rule: a fusion is the default only where a same-box A/B against
# the materializing rocBLAS + causal_softmax path shows it not slower
# (profiles/headdim_notes.md).  D=96 wins the no_grad forward and loses the
# training forward+backward; D=256 loses both.  The losing (D, direction)
# pairs stay reachable — they are the O(T) memory path — by setting the
# existing switch to 0: TRLX_AMD_NO_FLASH_PREFILL=0 / TRLX_AMD_NO_FLASH_TRAIN=0.
FLASH_PREFILL_DEFAULT_DIMS = (64, 96, 128)
FLASH_TRAIN_DEFAULT_DIMS = (64, 128)

# The seq2seq (T5) modes of the same kernels — non-causal, Toeplitz relative
# bias, arbitrary key mask, Tq != Tk — exist at these head dims only (t5-small
# through 11b and flan-t5).  Their defaults follow the same rule, measured by
# tools/bench_t5_attention.py against the eager matmul -> softmax -> matmul
# sequence and recorded in profiles/t5_attention_notes.md: every (head dim,
# direction) pair measured faster than eager (D=128 forward+backward by 3%,
# everything else by 2x or more), so all four are defaults.
SEQ2SEQ_FLASH_HEAD_DIMS = (64, 128)
SEQ2SEQ_FLASH_PREFILL_DEFAULT_DIMS = (64, 128)
SEQ2SEQ_FLASH_TRAIN_DEFAULT_DIMS = (64, 128)

# The T5 per-token generation step (csrc/s2s_decode.hip; kSeq2SeqDecodeHeadDims
# in attn_host.h): seq2seq_decode_attention / seq2seq_cross_decode_attention.
SEQ2SEQ_DECODE_HEAD_DIMS = (64, 128)


def _flash_gate(head_dim: int, train: bool, built, prefill_default, train_default) -> bool:
    """The gate behind ``flash_enabled`` / ``seq2seq_flash_enabled``: ``built``
    are the instantiated head dims, the other two the measured defaults."""
    if head_dim not in built:
        return False
    prefill = os.environ.get("TRLX_AMD_NO_FLASH_PREFILL")
    if prefill == "1":
        return False
    if not train:
        return prefill == "0" or head_dim in prefill_default
    switch = os.environ.get("TRLX_AMD_NO_FLASH_TRAIN")
    if switch == "1":
        return False
    return switch == "0" or head_dim in train_default


def flash_enabled(head_dim: int, train: bool) -> bool:
    """Does a model with this head dim take the flash kernels for the no_grad
    forward (``train=False``) or the training forward+backward (``train=True``)?

    ``TRLX_AMD_NO_FLASH_PREFILL=1`` turns both directions off and
    ``TRLX_AMD_NO_FLASH_TRAIN=1`` the training direction; ``=0`` turns the
    direction on for every instantiated head dim; unset follows the measured
    defaults above."""
    return _flash_gate(head_dim, train, FLASH_HEAD_DIMS, FLASH_PREFILL_DEFAULT_DIMS,
                       FLASH_TRAIN_DEFAULT_DIMS)


def seq2seq_flash_enabled(head_dim: int, train: bool) -> bool:
    """``flash_enabled`` for the T5 attention path (``ops.seq2seq_attention``):
    the same two switches with the same meaning (``1`` off, ``0`` on, unset
    follows the measured defaults), over the seq2seq default sets."""
    return _flash_gate(head_dim, train, SEQ2SEQ_FLASH_HEAD_DIMS,
                       SEQ2SEQ_FLASH_PREFILL_DEFAULT_DIMS, SEQ2SEQ_FLASH_TRAIN_DEFAULT_DIMS)


_EXT = None
_EXT_TRIED = False
_EXT_ERR: Optional[str] = None


def _load_ext():
    """Import the in-tree compiled extension (trlx_amd._C)."""
    global _EXT, _EXT_TRIED, _EXT_ERR
    if _EXT_TRIED:
        return _EXT
    _EXT_TRIED = True
    try:
        from trlx_amd import _C  # built by setup.py build_ext --inplace

        _EXT = _C
    except ImportError as e:  # pragma: no cover - exercised on GPU boxes
        _EXT = None
        _EXT_ERR = str(e)
    return _EXT


def extension_available() -> bool:
    return _load_ext() is not None


def _require_ext(op_name: str):
    ext = _load_ext()
    if ext is None:
        if os.environ.get("TRLX_AMD_ALLOW_EAGER") == "1":
            return None
        raise RuntimeError(
            f"trlx_amd op '{op_name}' needs the HIP extension (trlx_amd._C) on GPU "
            f"but it is not built (import error: {_EXT_ERR}). "
            f"Run `python setup.py build_ext --inplace` (or __graft_entry__.build()). "
            f"Set TRLX_AMD_ALLOW_EAGER=1 to debug with the eager fallback."
        )
    return ext


# --------------------------------------------------------------------------
# logprobs_of_labels
# --------------------------------------------------------------------------


class _LogprobsOfLabels(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, ext):
        logprobs, lse = ext.logprobs_fwd(logits, labels)
        ctx.save_for_backward(logits, labels, lse)
        return logprobs

    @staticmethod
    def backward(ctx, grad_out):
        logits, labels, lse = ctx.saved_tensors
        ext = _require_ext("logprobs_of_labels")
        grad_logits = ext.logprobs_bwd(logits, labels, lse, grad_out.contiguous())
        return grad_logits, None, None


def logprobs_of_labels(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """log softmax(logits)[..., labels] without materializing [., V] logprobs.

    Replaces reference trlx/utils/modeling.py:213-219 — the fused HIP kernel
    does the row max/logsumexp reduction and the single-label gather in one
    pass."""
    if logits.is_cuda:
        ext = _require_ext("logprobs_of_labels")
        if ext is not None:
            flat_logits = logits.reshape(-1, logits.shape[-1]).contiguous()
            flat_labels = labels.reshape(-1).contiguous()
            out = _LogprobsOfLabels.apply(flat_logits, flat_labels, ext)
            return out.view(labels.shape)
    return reference.logprobs_of_labels(logits, labels)


# --------------------------------------------------------------------------
# fused LM-head + logprob gather (no [B,T,V] logits materialization)
# --------------------------------------------------------------------------


def lm_logprobs(hidden: torch.Tensor, weight: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """log p(labels) from final hidden states + lm_head weight, computed
    tile-by-tile over the vocab so the [N, V] logits never hit HBM.

    Inference-only (no grad).  hidden [N,H] (bf16), weight [V,H], labels [N].
    """
    if hidden.is_cuda:
        ext = _require_ext("lm_logprobs")
        if ext is not None and hasattr(ext, "lm_logprobs"):
            h = hidden.contiguous()
            if h.shape[1] % 64 == 0 and hasattr(ext, "lm_logprobs_v2") and \
                    os.environ.get("TRLX_AMD_LM_LOGPROBS_V1") != "1":
                # minimum-2-phase pipelined 256x256 MFMA kernel
                return ext.lm_logprobs_v2(h, weight.contiguous(), labels.contiguous())
            return ext.lm_logprobs(h, weight.contiguous(), labels.contiguous())
    logits = hidden.float() @ weight.float().t()
    return reference.logprobs_of_labels(logits, labels)


class _LMLogprobsTrain(torch.autograd.Function):
    """Training-path fused lm_head+logprobs: forward via the pipelined MFMA
    kernel (logits never materialize, saves only the fp32 logsumexp);
    backward recomputes the logits tile-by-tile and emits dlogits directly
    (csrc/ce_backward.hip), then contracts with W / hidden on hipBLASLt for
    dh and dW."""

    @staticmethod
    def forward(ctx, hidden, weight, labels, ext):
        out, lse = ext.lm_logprobs_v2_with_lse(hidden, weight, labels, True)
        ctx.save_for_backward(hidden, weight, labels, lse)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        hidden, weight, labels, lse = ctx.saved_tensors
        ext = _require_ext("lm_logprobs_train")
        dlogits = ext.ce_dlogits(hidden, weight, labels, lse,
                                 grad_out.contiguous().float())
        dh = dlogits @ weight
        dw = dlogits.t() @ hidden if ctx.needs_input_grad[1] else None
        return dh, dw, None, None


def lm_logprobs_train(hidden: torch.Tensor, weight: torch.Tensor,
                      labels: torch.Tensor) -> torch.Tensor:
    """Differentiable log p(labels) from final hidden states + lm_head weight.

    GPU bf16 (H % 64 == 0): fused kernels, the [N, V] logits exist only as
    the bf16 dlogits of the backward.  Otherwise: plain logits path with
    the same math."""
    if (hidden.is_cuda and hidden.dtype == torch.bfloat16
            and weight.dtype == torch.bfloat16 and hidden.shape[-1] % 64 == 0
            and os.environ.get("TRLX_AMD_FUSED_LM_LOGPROBS") != "0"):
        ext = _require_ext("lm_logprobs_train")
        if ext is not None and hasattr(ext, "ce_dlogits"):
            return _LMLogprobsTrain.apply(hidden.contiguous(), weight.contiguous(),
                                          labels.contiguous(), ext)
    logits = torch.nn.functional.linear(hidden, weight)
    return logprobs_of_labels(logits, labels)


class _LinearGatherLSE(torch.autograd.Function):
    """z = x @ w^T + bias reduced to (z at idx, logsumexp z) per row without
    an [N, V] forward tensor (csrc/lm_logprobs_v2.hip, BIAS instantiation);
    the backward recomputes z tile-by-tile into the bf16 dz
    (csrc/ce_backward.hip, GATHER_LSE instantiation) and contracts it on
    hipBLASLt, as _LMLogprobsTrain does."""

    @staticmethod
    def forward(ctx, x, weight, bias, idx, ext):
        xb = x.to(torch.bfloat16).contiguous()
        wb = weight.to(torch.bfloat16).contiguous()
        b = bias.float().contiguous()
        val, lse = ext.linear_gather_lse_fwd(xb, wb, b, idx)
        ctx.save_for_backward(xb, wb, b, idx, lse)
        ctx.in_dtypes = (x.dtype, weight.dtype, bias.dtype)
        return val, lse

    @staticmethod
    def backward(ctx, g_val, g_lse):
        xb, wb, b, idx, lse = ctx.saved_tensors
        ext = _require_ext("linear_gather_lse")
        dz = ext.linear_gather_lse_bwd(xb, wb, b, idx, lse, g_val.float().contiguous(),
                                       g_lse.float().contiguous())
        need = ctx.needs_input_grad
        dx = (dz @ wb).to(ctx.in_dtypes[0]) if need[0] else None
        dw = (dz.t() @ xb).to(ctx.in_dtypes[1]) if need[1] else None
        # fp32 accumulation of the bf16 dz without an [N, V] fp32 copy
        db = dz.sum(0, dtype=torch.float32).to(ctx.in_dtypes[2]) if need[2] else None
        return dx, dw, db, None, None


def linear_gather_lse(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
                      idx: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``z = x @ weight^T + bias`` reduced per row to ``(z[n, idx[n]],
    logsumexp_v z[n, v])``, both differentiable.  x [N,K], weight [V,K],
    bias [V], idx [N] int64 -> two [N] tensors.

    GPU with K % 64 == 0: the fused kernels on bf16-rounded x and weight (fp32
    bias, fp32 accumulation and outputs); the only [N, V] tensor is the bf16
    dz of the backward.  Otherwise: F.linear + gather + logsumexp in the input
    dtype."""
    if x.is_cuda and x.shape[-1] % 64 == 0:
        ext = _require_ext("linear_gather_lse")
        if ext is not None and hasattr(ext, "linear_gather_lse_fwd"):
            return _LinearGatherLSE.apply(x, weight, bias, idx.contiguous(), ext)
    z = torch.nn.functional.linear(x, weight, bias)
    return z.gather(-1, idx.unsqueeze(-1)).squeeze(-1), torch.logsumexp(z, dim=-1)


def gathered_linear(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
                    idx: torch.Tensor) -> torch.Tensor:
    """``F.linear(x, weight, bias)[n, idx[n]]`` from the N gathered weight
    rows: N dot products instead of a vocab-wide GEMM.  Plain torch, fp32
    accumulation as in the GEMM it stands for, result in x's dtype."""
    out = (x.float() * weight[idx].float()).sum(-1) + bias[idx].float()
    return out.to(x.dtype)


ACT_CODES = {"none": 0, "gelu": 1, "gelu_new": 2, "relu": 3, "silu": 4}
_ACT_FNS = {
    0: lambda y: y,
    1: torch.nn.functional.gelu,
    2: lambda y: torch.nn.functional.gelu(y, approximate="tanh"),
    3: torch.nn.functional.relu,
    4: torch.nn.functional.silu,
}


def skinny_linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
                  act: int = 0) -> torch.Tensor:
    """Inference linear for skinny-M shapes (KV-cached decode): one 16x16
    MFMA tile per wave streaming the weight at line rate, bias + activation
    fused (csrc/skinny_gemm.hip).  Falls back to F.linear (+ activation)
    when autograd is on, on CPU, or for large M.

    OPT-IN (TRLX_AMD_SKINNY=1): wins its standalone microbench 1.2-2.4x,
    but inside the captured decode graph hipBLASLt's algos already run
    these shapes faster (same-box A/B: 749 vs 722 samples/s with the skinny
    path on) — the standalone hipBLASLt baseline was cold-start slow."""
    K = x.shape[-1]
    M = x.numel() // K
    if (x.is_cuda and not torch.is_grad_enabled() and x.dtype == torch.bfloat16
            and weight.dtype == torch.bfloat16 and M <= 256 and K % 32 == 0):
        if os.environ.get("TRLX_AMD_FP8_DECODE") == "1":
            # fp8 (e4m3) WEIGHT-ONLY decode GEMM: halves the weight stream
            # that the decode L2-access wall is proportional to.  Weight-only
            # quantization; activations and accumulation stay bf16/fp32;
            # per-output-row scales applied exactly on the accumulator.
            # OPT-IN: ~0.4% relative logit noise shifts sampled trajectories.
            ext = _require_ext("skinny_gemm_fp8")
            if ext is not None and hasattr(ext, "skinny_gemm_fp8"):
                q = getattr(weight, "_fp8_cache", None)
                if q is None or q[0].shape != weight.shape:
                    weight._fp8_cache = quantize_fp8_rows(weight)
                    q = weight._fp8_cache
                bb = bias.bfloat16() if bias is not None and bias.dtype != torch.bfloat16 \
                    else bias
                y = ext.skinny_gemm_fp8(x.reshape(M, K).contiguous(), q[0], q[1], bb, act)
                return y.view(*x.shape[:-1], weight.shape[0])
        if os.environ.get("TRLX_AMD_SKINNY") == "1":
            ext = _require_ext("skinny_gemm")
            if ext is not None and hasattr(ext, "skinny_gemm"):
                y = ext.skinny_gemm(x.reshape(M, K).contiguous(), weight.contiguous(), bias,
                                    act)
                return y.view(*x.shape[:-1], weight.shape[0])
    if (act in (1, 2, 3) and bias is not None and x.is_cuda
            and not torch.is_grad_enabled() and x.dtype == torch.bfloat16
            and _addmm_act_ok()):
        # single hipBLASLt GEMM with bias+GELU/ReLU epilogue: the eager
        # elementwise GELU was 127 ms of a 3.1 s bench cycle (profile pf3);
        # measured 24.3 -> 19.6 us on the decode MLP shape, 45.6 -> 33.7 us
        # on the experience shape (tools/probe_ln_gelu.py)
        try:
            y = torch._addmm_activation(bias, x.reshape(M, K), weight.t(),
                                        use_gelu=(act != 3))
            return y.view(*x.shape[:-1], weight.shape[0])
        except RuntimeError:
            global _ADDMM_ACT
            _ADDMM_ACT = False
    y = torch.nn.functional.linear(x, weight, bias)
    return _ACT_FNS[act](y)


def quantize_fp8_rows(w: torch.Tensor):
    """Per-output-row e4m3 weight quantization for the fp8 decode GEMM:
    returns (bytes [N, K] uint8, scales [N] fp32) with scale = amax/448."""
    wf = w.detach().float()
    s = (wf.abs().amax(dim=1) / 448.0).clamp(min=1e-12)
    q = (wf / s[:, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return q.view(torch.uint8).contiguous(), s.contiguous()


def dequantize_fp8_rows(q8: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """Reference inverse of quantize_fp8_rows (fp32)."""
    return q8.view(torch.float8_e4m3fn).float() * s[:, None]


def refresh_fp8_caches(module: "torch.nn.Module") -> int:
    """Requantize every cached fp8 decode weight IN PLACE (same buffers, so
    captured decode graphs see the fresh values).  Needed between training
    steps and generation: FusedAdamW writes the parameter arenas from a
    kernel, which torch's version counter never sees, so the caches cannot
    self-invalidate.  Returns the number of refreshed weights."""
    n = 0
    for m in module.modules():
        w = getattr(m, "weight", None)
        q = getattr(w, "_fp8_cache", None) if w is not None else None
        if q is not None:
            q8, s = quantize_fp8_rows(w)
            q[0].copy_(q8)
            q[1].copy_(s)
            n += 1
    return n


_ADDMM_ACT: Optional[bool] = None


def _addmm_act_ok() -> bool:
    global _ADDMM_ACT
    if _ADDMM_ACT is None:
        _ADDMM_ACT = (hasattr(torch, "_addmm_activation")
                      and os.environ.get("TRLX_AMD_NO_FUSED_ACT") != "1")
    return _ADDMM_ACT


# --------------------------------------------------------------------------
# norms
# --------------------------------------------------------------------------


class _Norm(torch.autograd.Function):
    """RMSNorm (``kind`` "rmsnorm", no bias) or LayerNorm ("layernorm") of the
    last dim, alone or with the residual add fused in.

    With ``res``: (y, s) = (norm(x + res), x + res).  The backward adds the
    residual-stream gradient ``ds`` into dx inside the norm-backward kernel, so
    the whole residual connection costs zero extra elementwise kernels.  dx
    and dres are the SAME tensor (aliasing is safe: autograd accumulates grads
    out-of-place).  Saved for the backward: the normalized input (x, or s with
    ``res``), the weight and the row statistics the kernel wrote."""

    @staticmethod
    def forward(ctx, kind, x, res, weight, bias, eps, ext):
        x2d = x.reshape(-1, x.shape[-1]).contiguous()
        r2d = res.reshape(x2d.shape).contiguous() if res is not None else None
        if kind == "rmsnorm":
            out, *stats = ext.rmsnorm_fwd(x2d, weight, eps, r2d)
        else:
            out, *stats = ext.layernorm_fwd(x2d, weight, bias, eps, r2d)
        s = stats.pop() if res is not None else x2d
        ctx.save_for_backward(s, weight, *stats)
        ctx.kind = kind
        ctx.x_shape = x.shape
        ctx.has_res = res is not None
        ctx.has_bias = bias is not None
        out = out.view(x.shape)
        return (out, s.view(x.shape)) if res is not None else out

    @staticmethod
    def backward(ctx, grad_out, grad_s=None):
        s2d, weight, *stats = ctx.saved_tensors
        ext = _require_ext(ctx.kind)
        bwd = ext.rmsnorm_bwd if ctx.kind == "rmsnorm" else ext.layernorm_bwd
        gs = grad_s.reshape(s2d.shape).contiguous() if grad_s is not None else None
        dx, dw, *db = bwd(s2d, weight, *stats, grad_out.reshape(s2d.shape).contiguous(), gs)
        dx = dx.view(ctx.x_shape)
        return (None, dx, dx if ctx.has_res else None, dw, db[0] if ctx.has_bias else None,
                None, None)


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    if x.is_cuda:
        ext = _require_ext("rmsnorm")
        if ext is not None:
            return _Norm.apply("rmsnorm", x, None, weight, None, eps, ext)
    return reference.rmsnorm(x, weight, eps)


def rmsnorm_add(x: torch.Tensor, res: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6):
    """Returns (rmsnorm(x + res), x + res)."""
    if x.is_cuda:
        ext = _require_ext("rmsnorm")
        if ext is not None:
            return _Norm.apply("rmsnorm", x, res, weight, None, eps, ext)
    s = x + res
    return reference.rmsnorm(s, weight, eps), s


def layernorm(
    x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], eps: float = 1e-5
) -> torch.Tensor:
    if x.is_cuda:
        ext = _require_ext("layernorm")
        if ext is not None:
            return _Norm.apply("layernorm", x, None, weight, bias, eps, ext)
    return reference.layernorm(x, weight, bias, eps)


def layernorm_add(x: torch.Tensor, res: torch.Tensor, weight: torch.Tensor,
                  bias: Optional[torch.Tensor], eps: float = 1e-5):
    """Returns (layernorm(x + res), x + res)."""
    if x.is_cuda:
        ext = _require_ext("layernorm")
        if ext is not None:
            return _Norm.apply("layernorm", x, res, weight, bias, eps, ext)
    s = x + res
    return reference.layernorm(s, weight, bias, eps), s


# --------------------------------------------------------------------------
# RoPE
# --------------------------------------------------------------------------


class _Rope(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cos, sin, positions, interleaved, rot, ext):
        out = ext.rope_fwd(x.contiguous(), cos, sin, positions, interleaved, False, rot)
        ctx.save_for_backward(cos, sin, positions)
        ctx.interleaved = interleaved
        ctx.rot = rot
        return out

    @staticmethod
    def backward(ctx, grad_out):
        cos, sin, positions = ctx.saved_tensors
        ext = _require_ext("rope")
        dx = ext.rope_fwd(grad_out.contiguous(), cos, sin, positions, ctx.interleaved, True, ctx.rot)
        return dx, None, None, None, None, None, None


def apply_rope(
    q: torch.Tensor,
    k: torch.Tensor,
    cos: torch.Tensor,
    sin: torch.Tensor,
    positions: Optional[torch.Tensor] = None,
    interleaved: bool = False,
    rot: int = 0,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Rotary embedding on q, k [B, H, T, D].  ``cos/sin``: [P, rot/2] tables
    (host-precomputed — guide Appendix B); ``positions``: [B, T] int32 row
    indices into the tables (required when prompts are left-padded);
    ``rot`` <= D rotates only the first ``rot`` dims (GPT-J/NeoX partial
    rotary), 0 means full D."""
    D = q.shape[-1]
    if rot <= 0:
        rot = D
    if positions is None:
        T = q.shape[2]
        positions = torch.arange(T, device=q.device, dtype=torch.int32).expand(q.shape[0], T).contiguous()
    if q.is_cuda:
        ext = _require_ext("rope")
        if ext is not None:
            positions = positions.to(torch.int32).contiguous()
            qo = _Rope.apply(q, cos, sin, positions, interleaved, rot, ext)
            ko = _Rope.apply(k, cos, sin, positions, interleaved, rot, ext)
            return qo, ko
    # CPU reference: gather per-position tables [B, T, rot/2]
    c = cos[positions.long()]
    s = sin[positions.long()]
    return _rope_ref_positional(q, k, c, s, interleaved, rot)


def _rope_ref_positional(q, k, c, s, interleaved, rot):
    """CPU reference with per-(b,t) tables c,s of [B, T, rot/2]."""

    def rotate(x):
        xf = x.float()
        xr = xf[..., :rot]
        if interleaved:
            x1, x2 = xr[..., 0::2], xr[..., 1::2]
        else:
            half = rot // 2
            x1, x2 = xr[..., :half], xr[..., half:]
        cc = c.float().unsqueeze(1)  # [B, 1, T, rot/2]
        ss = s.float().unsqueeze(1)
        o1 = x1 * cc - x2 * ss
        o2 = x2 * cc + x1 * ss
        if interleaved:
            out = torch.stack((o1, o2), dim=-1).flatten(-2)
        else:
            out = torch.cat((o1, o2), dim=-1)
        if rot < x.shape[-1]:
            out = torch.cat((out, xf[..., rot:]), dim=-1)
        return out.to(x.dtype)

    return rotate(q), rotate(k)


# --------------------------------------------------------------------------
# GAE / whitening
# --------------------------------------------------------------------------


def gae_advantages_and_returns(
    values: torch.Tensor,
    rewards: torch.Tensor,
    gamma: float,
    lam: float,
    use_whitening: bool = True,
    distributed: bool = False,
    group=None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """GAE reverse scan (+ optional distributed whitening) — SURVEY.md K6."""
    if values.is_cuda:
        ext = _require_ext("gae")
        if ext is not None:
            adv, ret = ext.gae(values.contiguous().float(), rewards.contiguous().float(), gamma, lam)
            if use_whitening:
                adv = whiten(adv, distributed=distributed, group=group)
            return adv.detach(), ret
    with torch.no_grad():
        adv, ret = reference.gae_advantages_and_returns(values, rewards, gamma, lam, use_whitening=False)
        if use_whitening:
            adv = whiten(adv, distributed=distributed, group=group)
        return adv.detach(), ret


def whiten(xs: torch.Tensor, shift_mean: bool = True, distributed: bool = False, group=None) -> torch.Tensor:
    """Zero-mean/unit-var normalization, optionally with global (cross-rank)
    statistics over ``group`` (reference trlx/utils/modeling.py:200-210)."""
    if xs.is_cuda:
        ext = _require_ext("whiten")
        if ext is not None:
            stats = ext.sum_count(xs.contiguous().float())  # [sum, sumsq, count]
            if distributed:
                import torch.distributed as dist

                dist.all_reduce(stats, group=group)
            mean = stats[0] / stats[2]
            var = stats[1] / stats[2] - mean * mean
            return ext.normalize(xs.contiguous().float(), mean, var, shift_mean)
    return reference.whiten(xs, shift_mean, distributed, group)


# --------------------------------------------------------------------------
# fused PPO loss
# --------------------------------------------------------------------------

# What PPOConfig.loss returns, in its order: the layout of the kernel's
# statistics vector (csrc/ppo_loss.hip, the O_* enum).
PPO_LOSS_STAT_KEYS = (
    "losses/total_loss", "losses/policy_loss", "losses/value_loss",
    "values/mean", "values/min", "values/max", "values/std", "values/values_error", "values/clipfrac",
    "old_values/mean", "old_values/min", "old_values/max", "old_values/std",
    "returns/mean", "returns/min", "returns/max", "returns/std",
    "policy/approx_kl", "policy/clipfrac", "ratio", "padding_percentage",
)


class _PPOLoss(torch.autograd.Function):
    """The kernel already wrote d loss / d logprobs and d loss / d values for
    an upstream gradient of 1 (stacked as one [2, B, R] tensor); backward is
    ONE device-side multiply by the incoming gradient."""

    @staticmethod
    def forward(ctx, logprobs, values, old_logprobs, old_values, advantages, returns, mask,
                cliprange, cliprange_value, vf_coef, ext):
        loss, stats, grads = ext.ppo_loss(logprobs, values, old_logprobs, old_values, advantages,
                                          returns, mask, cliprange, cliprange_value, vf_coef)
        ctx.save_for_backward(grads)
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    def backward(ctx, grad_loss, _grad_stats):
        (grads,) = ctx.saved_tensors
        g = grads * grad_loss
        return (g[0] if ctx.needs_input_grad[0] else None,
                g[1] if ctx.needs_input_grad[1] else None) + (None,) * 9


def ppo_loss_fusable(logprobs, values, old_logprobs, old_values, advantages, returns, mask) -> bool:
    """Does this call of ``PPOConfig.loss`` take the fused kernel?  GPU fp32
    [B, R] inputs of one shape (any strides), an int64 mask, gradients wanted
    for ``logprobs``/``values`` only, and ``TRLX_AMD_NO_FUSED_PPO_LOSS`` not 1."""
    if os.environ.get("TRLX_AMD_NO_FUSED_PPO_LOSS") == "1":
        return False
    floats = (logprobs, values, old_logprobs, old_values, advantages, returns)
    if not (logprobs.is_cuda and logprobs.dim() == 2 and logprobs.numel() > 0):
        return False
    if not all(t.is_cuda and t.dtype == torch.float32 and t.shape == logprobs.shape
               and t.device == logprobs.device for t in floats):
        return False
    if not (mask.is_cuda and mask.dtype == torch.int64 and mask.shape == logprobs.shape
            and mask.device == logprobs.device):
        return False
    if torch.is_grad_enabled() and any(t.requires_grad for t in floats[2:]):
        return False
    return _require_ext("ppo_loss") is not None


def ppo_loss(logprobs, values, old_logprobs, old_values, advantages, returns, mask,
             cliprange: float, cliprange_value: float, vf_coef: float):
    """Clipped-surrogate PPO loss and its statistics from one kernel launch
    (csrc/ppo_loss.hip).  Returns ``(loss, stats)`` as ``PPOConfig.loss``
    does: ``loss`` a 0-dim tensor with the autograd node, ``stats`` a dict of
    0-dim device tensors (views into one vector; no host synchronisation, so
    the call can be captured into a graph)."""
    ext = _require_ext("ppo_loss")
    loss, stats = _PPOLoss.apply(logprobs, values, old_logprobs, old_values, advantages, returns,
                                 mask, float(cliprange), float(cliprange_value), float(vf_coef), ext)
    return loss, dict(zip(PPO_LOSS_STAT_KEYS, stats.unbind(0)))


# --------------------------------------------------------------------------
# sampling
# --------------------------------------------------------------------------


def decode_prep(
    qkv: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    cache_idx: torch.Tensor,
    num_heads: int,
    cos: Optional[torch.Tensor] = None,
    sin: Optional[torch.Tensor] = None,
    key_starts: Optional[torch.Tensor] = None,
    rot: int = 0,
    interleaved: bool = False,
) -> torch.Tensor:
    """Fused decode-step QKV prep: split fused qkv [B,1,QKV], RoPE q/k at
    position (*cache_idx - key_starts[b]), append k/v to the cache at
    *cache_idx, return q [B,Hq,1,D].  GPU-only (the eager path covers CPU)."""
    ext = _require_ext("decode_prep")
    return ext.decode_prep(qkv.contiguous(), k_cache, v_cache, cos, sin, key_starts, cache_idx,
                           num_heads, rot, interleaved)


def fused_decode_attention(
    qkv: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    seq_lens: torch.Tensor,
    key_starts: Optional[torch.Tensor],
    cos: Optional[torch.Tensor],
    sin: Optional[torch.Tensor],
    cache_idx: torch.Tensor,
    rot: int,
    interleaved: bool,
    scale: float,
    alibi_slopes: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """MHA decode step in ONE kernel: split fused qkv, RoPE q/k, append k/v
    to the cache at *cache_idx, flash-decode attention — out [B,H,1,D].
    GPU-only (the eager path covers CPU); requires Hq == Hkv.
    ``alibi_slopes`` [H] fp32 adds ``slope[h] * (key - key_starts[b])`` to the
    scaled scores (Bloom; not combinable with RoPE tables)."""
    ext = _require_ext("fused_decode_attention")
    ks = key_starts.to(torch.int32).contiguous() if key_starts is not None else None
    if cos is not None and cos.dtype != torch.float32:
        cos, sin = cos.float(), sin.float()  # kernels require fp32 trig tables
    return ext.fused_decode_attention(qkv.contiguous(), k_cache, v_cache,
                                      seq_lens.to(torch.int32).contiguous(), ks, cos, sin,
                                      cache_idx, rot, interleaved, scale, alibi_slopes)


class _QKVPrep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, num_heads, num_kv_heads, head_dim, cos, sin, pos, qscale, rot,
                interleaved, ext):
        q, k, v = ext.qkv_prep_fwd(qkv, num_heads, num_kv_heads, head_dim, cos, sin, pos,
                                   qscale, rot, interleaved)
        ctx.save_for_backward(*( [cos, sin, pos] if cos is not None else [] ))
        ctx.has_rope = cos is not None
        ctx.qscale = qscale
        ctx.rot = rot
        ctx.interleaved = interleaved
        return q, k, v

    @staticmethod
    def backward(ctx, dq, dk, dv):
        ext = _require_ext("qkv_prep")
        cos = sin = pos = None
        if ctx.has_rope:
            cos, sin, pos = ctx.saved_tensors
        dqkv = ext.qkv_prep_bwd(dq.contiguous(), dk.contiguous(), dv.contiguous(), cos, sin,
                                pos, ctx.qscale, ctx.rot, ctx.interleaved)
        return dqkv, None, None, None, None, None, None, None, None, None, None


def qkv_prep(
    qkv: torch.Tensor,
    num_heads: int,
    num_kv_heads: int,
    head_dim: int,
    cos: Optional[torch.Tensor] = None,
    sin: Optional[torch.Tensor] = None,
    positions: Optional[torch.Tensor] = None,
    qscale: float = 1.0,
    rot: int = 0,
    interleaved: bool = False,
):
    """Fused split + RoPE + q-scale for the T>1 path (GPU-only; autograd-
    aware — backward applies the inverse rotation and re-packs grads)."""
    ext = _require_ext("qkv_prep")
    if positions is not None:
        positions = positions.to(torch.int32).contiguous()
    if cos is not None and cos.dtype != torch.float32:
        cos, sin = cos.float(), sin.float()  # kernels require fp32 trig tables
    return _QKVPrep.apply(qkv.contiguous(), num_heads, num_kv_heads, head_dim, cos, sin,
                          positions, qscale, rot, interleaved, ext)


def sample_token(
    logits: torch.Tensor,
    temperature: float = 1.0,
    top_k: int = 0,
    top_p: float = 1.0,
    generator: Optional[torch.Generator] = None,
    seed: Optional[int] = None,
    offset: int = 0,
) -> torch.Tensor:
    """One fused sampling step [B, V] -> [B].

    On GPU: Gumbel-max categorical sampling in a single pass (no softmax
    materialization), counter-based RNG keyed by (seed, offset, row) for
    per-DP-rank reproducibility.  top_k/top_p pre-filter runs tile-wise in
    the same kernel via threshold select.
    """
    if logits.is_cuda:
        ext = _require_ext("sample_token")
        if ext is not None:
            if temperature == 0.0:
                return torch.argmax(logits, dim=-1)
            if seed is None:
                seed = int(torch.randint(0, 2**31 - 1, (1,), generator=generator).item())
            dev_offset = isinstance(offset, torch.Tensor)
            if top_p is not None and 0.0 < top_p < 1.0:
                # top-p needs a sorted scan: do the filter with library sort,
                # then fused gumbel sampling on the filtered logits.  Every op
                # here is hipGraph-capturable (device-offset RNG included), so
                # top-p decode stays on the captured-graph path.
                # HF order: top-k first, then top-p (matches reference.sample_token)
                def _gumbel(t):
                    if dev_offset:
                        return ext.gumbel_sample_dev(t, 1.0, None, seed, offset)
                    return ext.gumbel_sample(t, 1.0, None, seed, offset)

                lg = logits.float() / max(temperature, 1e-6)
                if top_k and 0 < top_k < logits.shape[-1]:
                    # both filters confined to the [B, top_k] subset: softmax
                    # over the top-k masked vocab equals softmax over the
                    # subset, so the p-filter never touches [B, V]
                    vals, idx = torch.topk(lg, top_k, dim=-1)  # sorted desc
                    probs = torch.softmax(vals, dim=-1)
                    cum = probs.cumsum(dim=-1)
                    vals = vals.masked_fill(cum - probs > top_p, float("-inf"))
                    pos = _gumbel(vals.contiguous())
                    return idx.gather(-1, pos.view(-1, 1)).view(pos.shape)
                # V-wide: per-row threshold from the sorted scan, elementwise
                # mask — no [B, V] scatter (was a 520 us kernel at [128, 50257])
                sorted_logits, _ = torch.sort(lg, descending=True, dim=-1)
                probs = torch.softmax(sorted_logits, dim=-1)
                cum = probs.cumsum(dim=-1)
                keep = (cum - probs <= top_p).sum(-1, keepdim=True).clamp(min=1) - 1
                thr = sorted_logits.gather(-1, keep)
                lg = lg.masked_fill(lg < thr, float("-inf"))
                return _gumbel(lg.contiguous())
            if top_k and 0 < top_k < logits.shape[-1]:
                lg = (logits.float() / max(temperature, 1e-6)).contiguous()
                thr = torch.topk(lg, top_k, dim=-1).values[:, -1].contiguous()
                if dev_offset:
                    return ext.gumbel_sample_dev(lg, 1.0, thr, seed, offset)
                return ext.gumbel_sample(lg, 1.0, thr, seed, offset)
            # fp32 and bf16 logits both sample natively (no cast kernel)
            lg = logits.contiguous() if logits.dtype in (torch.float32, torch.bfloat16) \
                else logits.float().contiguous()
            if dev_offset:
                return ext.gumbel_sample_dev(lg, float(temperature), None, seed, offset)
            return ext.gumbel_sample(lg, float(temperature), None, seed, offset)
    return reference.sample_token(logits, temperature, top_k, top_p, generator)


def _top_p_filter(logits: torch.Tensor, top_p: float) -> torch.Tensor:
    sorted_logits, sorted_idx = torch.sort(logits, descending=True, dim=-1)
    probs = torch.softmax(sorted_logits, dim=-1)
    cum = probs.cumsum(dim=-1)
    remove = cum - probs > top_p
    sorted_logits = sorted_logits.masked_fill(remove, float("-inf"))
    return torch.full_like(logits, float("-inf")).scatter(-1, sorted_idx, sorted_logits)


# --------------------------------------------------------------------------
# attention decode (single new token vs KV cache)
# --------------------------------------------------------------------------


def attention_decode(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    seq_lens: torch.Tensor,
    scale: float,
    seq_starts: Optional[torch.Tensor] = None,
    alibi_slopes: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Fused decode attention: q [B, Hq, 1, D] vs cache [B, Hkv, S, D]
    with per-row valid key range [seq_starts[b], seq_lens[b]) -> [B, Hq, 1, D]
    (``seq_starts`` handles left-padded prompts).

    Memory-bound flash-decode kernel; online softmax, no
    [B, H, S] score materialization.  ``alibi_slopes`` [Hq] fp32 (one slope
    per QUERY head) adds ``slope[h] * (key - seq_starts[b])`` to the scaled
    scores (Bloom).
    """
    if q.is_cuda:
        ext = _require_ext("attention_decode")
        if ext is not None:
            ss = None if seq_starts is None else seq_starts.to(torch.int32).contiguous()
            return ext.attention_decode(
                q.contiguous(), k_cache.contiguous(), v_cache.contiguous(),
                seq_lens.to(torch.int32).contiguous(), scale, ss, alibi_slopes,
            )
    # reference: masked SDPA
    B, Hq, _, D = q.shape
    Hkv = k_cache.shape[1]
    S = k_cache.shape[2]
    qf = q.float()
    kf = k_cache.float()
    vf = v_cache.float()
    if Hkv != Hq:
        rep = Hq // Hkv
        kf = kf.repeat_interleave(rep, dim=1)
        vf = vf.repeat_interleave(rep, dim=1)
    scores = torch.matmul(qf, kf.transpose(-1, -2)) * scale  # [B, Hq, 1, S]
    pos = torch.arange(S, device=q.device).view(1, 1, 1, S)
    mask = pos >= seq_lens.view(B, 1, 1, 1)
    if seq_starts is not None:
        mask = mask | (pos < seq_starts.view(B, 1, 1, 1))
    if alibi_slopes is not None:
        key_pos = pos if seq_starts is None else (pos - seq_starts.view(B, 1, 1, 1)).clamp(min=0)
        scores = scores + alibi_slopes.float().view(1, Hq, 1, 1) * key_pos.float()
    scores = scores.masked_fill(mask, float("-inf"))
    probs = torch.softmax(scores, dim=-1)
    return torch.matmul(probs, vf).to(q.dtype)


# --------------------------------------------------------------------------
# causal softmax (training attention: rocBLAS GEMM + this fused kernel)
# --------------------------------------------------------------------------


class _CausalSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, start_pos, key_starts, ext):
        probs = ext.causal_softmax_fwd(scores.contiguous(), start_pos, key_starts)
        ctx.save_for_backward(probs)
        return probs

    @staticmethod
    def backward(ctx, grad_out):
        (probs,) = ctx.saved_tensors
        ext = _require_ext("causal_softmax")
        return ext.causal_softmax_bwd(probs, grad_out.contiguous()), None, None, None


def causal_softmax(
    scores: torch.Tensor, start_pos: int = 0, key_starts: Optional[torch.Tensor] = None
) -> torch.Tensor:
    """Causal-masked softmax of attention scores [B, H, Tq, Tk] (fused mask +
    online softmax; SURVEY.md K2's softmax half — GEMMs ride rocBLAS).

    ``key_starts`` [B] marks the first valid key per batch row (left-padding).
    """
    if scores.is_cuda:
        ext = _require_ext("causal_softmax")
        if ext is not None:
            if key_starts is not None:
                key_starts = key_starts.to(torch.int32).contiguous()
            return _CausalSoftmax.apply(scores, start_pos, key_starts, ext)
    return reference.causal_softmax(scores, start_pos, key_starts)


def flash_prefill(q, k, v, key_starts=None, start_pos: int = 0, scale: float = 1.0,
                  tk=None, alibi_slopes=None):
    """Forward-only flash attention for prefill / the no_grad experience pass
    (csrc/flash_prefill.hip): q [B,Hq,T,D] (bf16), k/v [B,Hkv,Sk,D] with the
    first ``tk`` tokens valid (cache prefill passes the whole cache), causal +
    left-pad masking via ``key_starts``.  ``alibi_slopes`` [Hq] fp32 adds
    ``slope[h] * (key - key_starts[b])`` to the scaled scores inside the tile
    loop (Bloom).  Returns [B,Hq,T,D] bf16; the [B,H,T,T] scores never
    materialize."""
    ext = _require_ext("flash_prefill")
    if ext is None or not q.is_cuda:
        return reference.flash_prefill(q, k, v, key_starts, start_pos, scale, tk,
                                       alibi_slopes=alibi_slopes)
    ks = key_starts.to(torch.int32).contiguous() if key_starts is not None else None
    return ext.flash_prefill(q.contiguous(), k, v, ks, int(start_pos), float(scale),
                             int(tk) if tk is not None else 0, alibi_slopes)


class _FlashAttention(torch.autograd.Function):
    """Differentiable flash attention, causal (training prefill: start_pos ==
    0, Tk == T) and seq2seq alike: forward saves the per-row logsumexp,
    backward recomputes P from it tile-by-tile (csrc/flash_backward.hip) — the
    [B,H,T,T] scores never materialize in either direction.  ``alibi_slopes``,
    ``rel_bias`` and ``key_mask`` are constants here (not trainable; the
    kernels produce no bias gradient)."""

    @staticmethod
    def forward(ctx, q, k, v, key_starts, alibi_slopes, rel_bias, bias_zero, key_mask, causal,
                start_pos, scale, ext):
        out, lse = ext.flash_prefill_lse(q, k, v, key_starts, start_pos, scale, 0, True,
                                         alibi_slopes, rel_bias, bias_zero, key_mask, causal)
        ctx.save_for_backward(q, k, v, out, lse)
        # the backward kernels have no start_pos: the bias index is
        # key - (start_pos + row) + bias_zero, so the offset folds into bias_zero
        ctx.bwd_args = (key_starts, scale, alibi_slopes, rel_bias, bias_zero - start_pos,
                        key_mask, causal)
        ctx.ext = ext
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        dq, dk, dv = ctx.ext.flash_prefill_bwd(q, k, v, out, dout, lse, *ctx.bwd_args)
        return (dq, dk, dv) + (None,) * 9


def flash_attention(q, k, v, key_starts=None, scale: float = 1.0, alibi_slopes=None):
    """Differentiable flash attention for the TRAINING forward (full causal
    self-attention, no cache): q [B,Hq,T,D] bf16, k/v [B,Hkv,T,D].  On CPU or
    without the extension, falls back to the fp32 reference (autograd handles
    the backward there)."""
    ext = _require_ext("flash_attention")
    if ext is None or not q.is_cuda:
        return reference.flash_prefill(q, k, v, key_starts, 0, scale,
                                       alibi_slopes=alibi_slopes).to(q.dtype)
    ks = key_starts.to(torch.int32).contiguous() if key_starts is not None else None
    return _FlashAttention.apply(q.contiguous(), k.contiguous(), v.contiguous(), ks,
                                 alibi_slopes, None, 0, None, True, 0, float(scale), ext)


# --------------------------------------------------------------------------
# seq2seq (T5) attention: relative-position bias, key masks, cross-attention
# --------------------------------------------------------------------------


def t5_rel_bias(table: torch.Tensor, q_len: int, k_len: int, q_offset: int = 0,
                bidirectional: bool = True, num_buckets: int = 32,
                max_distance: int = 128) -> Tuple[torch.Tensor, int]:
    """The T5 relative-position bias in the form the kernels read: a per-head
    Toeplitz vector ``rel_bias`` [H, L] fp32 and ``bias_zero``, the index of
    relative position 0 (``reference.t5_rel_bias`` has the layout).  Plain
    torch on every device — one embedding lookup of L rows — and differentiable
    with respect to ``table`` (the [num_buckets, H] embedding weight)."""
    return reference.t5_rel_bias(table, q_len, k_len, q_offset, bidirectional, num_buckets,
                                 max_distance)


def seq2seq_attention(q, k, v, rel_bias=None, bias_zero: int = 0, key_mask=None,
                      causal: bool = False, start_pos: int = 0, scale: float = 1.0):
    """Flash attention for encoder-decoder models (csrc/flash_prefill.hip and
    flash_backward.hip in their seq2seq modes): q [B,Hq,Tq,D] bf16, k/v
    [B,Hkv,Tk,D], ``Tq != Tk`` allowed when not ``causal`` (cross-attention).

    ``rel_bias`` [Hq, L] fp32 with ``bias_zero`` is the Toeplitz T5 bias of
    ``t5_rel_bias``; ``key_mask`` [B, Tk] is any visibility mask (nonzero =
    visible, no contiguity assumed, no host sync; a contiguous uint8 mask is
    used as it is, anything else is converted here on every call); a query row
    with no visible key returns zeros.  K and V rows at masked keys must be
    finite (they enter the backward as ``0 * x``).  Under ``no_grad``, or when no input requires grad, the
    forward-only kernel runs; otherwise the forward saves the row logsumexp
    and the backward kernels produce dq/dk/dv.  ``rel_bias`` gets NO gradient
    from the kernels, so a bias that requires grad is an error under grad mode
    (models keep a trainable table on the eager path).  On CPU the fp32
    reference runs."""
    if rel_bias is not None and rel_bias.requires_grad and torch.is_grad_enabled():
        raise RuntimeError(
            "seq2seq_attention: rel_bias requires grad, but the kernels produce no bias "
            "gradient; detach it or keep this attention on the eager path")
    ext = _require_ext("seq2seq_attention")
    if ext is None or not q.is_cuda:
        return reference.seq2seq_attention(q, k, v, rel_bias, bias_zero, key_mask, causal,
                                           start_pos, scale).to(q.dtype)
    km = None
    if key_mask is not None:
        km = key_mask if key_mask.dtype == torch.uint8 else (key_mask != 0).to(torch.uint8)
        km = km.contiguous()
    rb = rel_bias.detach() if rel_bias is not None else None
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    needs_grad = torch.is_grad_enabled() and (q.requires_grad or k.requires_grad
                                              or v.requires_grad)
    if not needs_grad:
        return ext.flash_prefill(q, k, v, None, int(start_pos), float(scale), 0, None, rb,
                                 int(bias_zero), km, bool(causal))
    if causal and (start_pos != 0 or q.shape[2] != k.shape[2]):
        raise RuntimeError("seq2seq_attention: causal training needs Tq == Tk and start_pos == 0")
    return _FlashAttention.apply(q, k, v, None, None, rb, int(bias_zero), km, bool(causal),
                                 int(start_pos), float(scale), ext)


def seq2seq_decode_enabled(head_dim: int) -> bool:
    """Does T5 generation take the cached kernel step at this head dim?
    ``TRLX_AMD_NO_S2S_DECODE=1`` keeps the eager ``past`` loop (the escape
    hatch and the A/B baseline of profiles/t5_decode_notes.md)."""
    return (head_dim in SEQ2SEQ_DECODE_HEAD_DIMS
            and os.environ.get("TRLX_AMD_NO_S2S_DECODE") != "1")


def seq2seq_decode_attention(q, k_new, v_new, k_cache, v_cache, cache_idx, rel_bias=None,
                             bias_zero: int = 0, scale: float = 1.0):
    """The T5 self-attention of ONE new token (csrc/s2s_decode.hip): q, k_new,
    v_new [B, H, D] bf16 are its three projections, ``cache_idx`` a one-element
    int64 tensor ON THE DEVICE holding its position ``pos``.  Appends k_new /
    v_new IN PLACE to row ``pos`` of the preallocated caches [B, H, S, D] and
    attends over keys 0..pos inclusive; ``rel_bias`` [H, L] fp32 with
    ``bias_zero`` is the Toeplitz bias of ``t5_rel_bias`` (index clamped to
    [0, L)).  ``pos`` is never read on the host, so a captured graph replays
    the step for every token; a ``pos`` outside [0, S) writes nothing and
    returns zeros.  Returns [B, H, 1, D].  On CPU the fp32 reference runs."""
    B, H, D = k_cache.shape[0], k_cache.shape[1], k_cache.shape[3]
    q, k_new, v_new = (t.reshape(B, H, D) for t in (q, k_new, v_new))
    ext = _require_ext("seq2seq_decode_attention") if q.is_cuda else None
    if ext is None:
        return reference.seq2seq_decode_attention(q, k_new, v_new, k_cache, v_cache, cache_idx,
                                                  rel_bias, bias_zero, scale)
    rb = rel_bias.detach() if rel_bias is not None else None
    return ext.seq2seq_decode_attention(q.contiguous(), k_new.contiguous(), v_new.contiguous(),
                                        k_cache, v_cache, cache_idx, rb, int(bias_zero),
                                        float(scale))


def seq2seq_cross_decode_attention(q, k, v, key_mask=None, scale: float = 1.0):
    """The T5 cross-attention of one new token: q [B, H, 1, D] bf16 against the
    prompt's k / v [B, H, Tk, D] under ``key_mask`` [B, Tk] uint8 (nonzero =
    visible, any pattern).  Masked keys are skipped — never loaded — so stale or
    non-finite rows behind the mask cannot leak; a row with no visible key
    returns zeros.  Returns [B, H, 1, D].  On CPU the fp32 reference runs."""
    ext = _require_ext("seq2seq_cross_decode_attention") if q.is_cuda else None
    if ext is None:
        return reference.seq2seq_cross_decode_attention(q, k, v, key_mask, scale)
    return ext.seq2seq_cross_decode_attention(q.contiguous(), k, v, key_mask, float(scale))
