"""Pure-PyTorch reference implementations of every custom op.

These are the numerics ground truth for the HIP kernels (tests compare the
gfx950 kernels against these in fp32) and the CPU execution path for tests on
machines without a GPU.  On a GPU box the dispatcher in ``trlx_amd.ops``
refuses to fall back here unless explicitly allowed — the HIP path must be
the one that runs.
"""

import math
from typing import Optional, Tuple

import torch


def logprobs_of_labels(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """Per-token log-probabilities of ``labels`` under ``logits``.

    Parity: reference trlx/utils/modeling.py:213-219 (``logprobs_of_labels``).
    ``logits``: [..., V]; ``labels``: [...] int64 -> [...] float.
    """
    logprobs = torch.nn.functional.log_softmax(logits.float(), dim=-1)
    return torch.gather(logprobs, -1, labels.unsqueeze(-1)).squeeze(-1)


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """RMSNorm over the last dim (Llama-style)."""
    dtype = x.dtype
    x = x.float()
    var = x.pow(2).mean(-1, keepdim=True)
    x = x * torch.rsqrt(var + eps)
    return (x * weight.float()).to(dtype)


def layernorm(
    x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], eps: float = 1e-5
) -> torch.Tensor:
    """LayerNorm over the last dim."""
    dtype = x.dtype
    out = torch.nn.functional.layer_norm(x.float(), (x.shape[-1],), weight.float(), None if bias is None else bias.float(), eps)
    return out.to(dtype)


_GATED_ACT_FNS = {
    "gelu": torch.nn.functional.gelu,
    "gelu_new": lambda x: torch.nn.functional.gelu(x, approximate="tanh"),
    "relu": torch.nn.functional.relu,
    "silu": torch.nn.functional.silu,
}


def gated_act(gate: torch.Tensor, up: Optional[torch.Tensor] = None,
              act: str = "silu") -> torch.Tensor:
    """``act(g) * u`` in the input dtype: ``g, u = gate, up``, or the two halves
    of a fused ``gate`` [..., 2I] when ``up`` is None.  The expression the gated
    MLPs spell out themselves when ``ops.gated_act_enabled()`` is off."""
    fn = _GATED_ACT_FNS[act]
    if up is None:
        i = gate.shape[-1] // 2
        return fn(gate[..., :i]) * gate[..., i:]
    return fn(gate) * up


def lora_linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
                lora_A: torch.Tensor, lora_B: torch.Tensor, scaling: float,
                x_lora: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``x W^T + bias + scaling * (x_lora A^T) B^T``: a linear with a LoRA adapter,
    the line ``LoRALinear`` spells out itself when ``ops.lora_enabled()`` is off.
    ``x_lora`` is the adapter's input where it differs from ``x`` (dropout)."""
    xa = x if x_lora is None else x_lora
    lora = torch.nn.functional.linear(
        torch.nn.functional.linear(xa.to(lora_A.dtype), lora_A), lora_B)
    return torch.nn.functional.linear(x, weight, bias) + scaling * lora


def rope_cos_sin(
    seq_len: int,
    dim: int,
    base: float = 10000.0,
    device: Optional[torch.device] = None,
    dtype: torch.dtype = torch.float32,
    position_offset: int = 0,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Host-precomputed RoPE tables ``[seq_len, dim/2]`` (guide: precompute
    trig on host — on-device sinf/cosf turns memory-bound into VALU-bound)."""
    inv_freq = 1.0 / (base ** (torch.arange(0, dim, 2, device=device, dtype=torch.float32) / dim))
    t = torch.arange(position_offset, position_offset + seq_len, device=device, dtype=torch.float32)
    freqs = torch.outer(t, inv_freq)
    return freqs.cos().to(dtype), freqs.sin().to(dtype)


def apply_rope(
    q: torch.Tensor,
    k: torch.Tensor,
    cos: torch.Tensor,
    sin: torch.Tensor,
    interleaved: bool = False,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Apply rotary embedding to q, k of shape [B, H, T, D].

    ``cos``/``sin``: [T, D/2].  ``interleaved=True`` rotates (x0,x1),(x2,x3)
    pairs (GPT-J/NeoX style); ``False`` rotates (x_i, x_{i+D/2}) halves
    (Llama style).
    """

    def rot(x):
        xf = x.float()
        if interleaved:
            x1 = xf[..., 0::2]
            x2 = xf[..., 1::2]
        else:
            half = x.shape[-1] // 2
            x1 = xf[..., :half]
            x2 = xf[..., half:]
        c = cos.float().view(1, 1, cos.shape[0], cos.shape[1])
        s = sin.float().view(1, 1, sin.shape[0], sin.shape[1])
        o1 = x1 * c - x2 * s
        o2 = x2 * c + x1 * s
        if interleaved:
            out = torch.stack((o1, o2), dim=-1).flatten(-2)
        else:
            out = torch.cat((o1, o2), dim=-1)
        return out.to(x.dtype)

    return rot(q), rot(k)


def gae_advantages_and_returns(
    values: torch.Tensor,
    rewards: torch.Tensor,
    gamma: float,
    lam: float,
    use_whitening: bool = True,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Generalized Advantage Estimation over the response dimension.

    Parity: reference trlx/models/modeling_ppo.py:136-173
    (``PPOConfig.get_advantages_and_returns``): reverse scan
    delta_t = r_t + gamma * V_{t+1} - V_t, A_t = delta_t + gamma*lam*A_{t+1};
    returns = A + V; advantages whitened.
    ``values``/``rewards``: [B, T] over response tokens only.
    """
    T = rewards.shape[1]
    lastgaelam = torch.zeros_like(rewards[:, 0])
    advantages_reversed = []
    vals = values.float()
    rews = rewards.float()
    for t in reversed(range(T)):
        nextvalues = vals[:, t + 1] if t < T - 1 else torch.zeros_like(vals[:, 0])
        delta = rews[:, t] + gamma * nextvalues - vals[:, t]
        lastgaelam = delta + gamma * lam * lastgaelam
        advantages_reversed.append(lastgaelam)
    advantages = torch.stack(advantages_reversed[::-1], dim=1)
    returns = advantages + vals
    if use_whitening:
        advantages = whiten(advantages)
    return advantages.detach(), returns


def whiten(xs: torch.Tensor, shift_mean: bool = True, distributed: bool = False, group=None) -> torch.Tensor:
    """Whiten to zero mean / unit variance (optionally over a process group).

    Parity: reference trlx/utils/modeling.py:200-210.
    """
    if distributed:
        from ..utils.modeling import get_global_statistics

        mean, var, _ = get_global_statistics(xs, group=group)
    else:
        var, mean = torch.var_mean(xs)
    whitened = (xs - mean) * torch.rsqrt(var + 1e-8)
    if not shift_mean:
        whitened += mean
    return whitened


def sample_token(
    logits: torch.Tensor,
    temperature: float = 1.0,
    top_k: int = 0,
    top_p: float = 1.0,
    generator: Optional[torch.Generator] = None,
) -> torch.Tensor:
    """One sampling step over ``logits`` [B, V] -> token ids [B].

    Greedy when temperature == 0.  Filtering order matches HF: top-k then
    top-p on the temperature-scaled distribution.
    """
    if temperature == 0.0:
        return logits.argmax(dim=-1)
    logits = logits.float() / temperature
    if top_k and top_k > 0 and top_k < logits.shape[-1]:
        kth = torch.topk(logits, top_k, dim=-1).values[..., -1, None]
        logits = logits.masked_fill(logits < kth, float("-inf"))
    if top_p is not None and 0.0 < top_p < 1.0:
        sorted_logits, sorted_idx = torch.sort(logits, descending=True, dim=-1)
        probs = torch.softmax(sorted_logits, dim=-1)
        cum = probs.cumsum(dim=-1)
        # keep the smallest set whose cumulative prob >= top_p (HF semantics:
        # remove tokens with cumulative probability above the threshold,
        # keeping at least the first)
        remove = cum - probs > top_p
        sorted_logits = sorted_logits.masked_fill(remove, float("-inf"))
        logits = torch.full_like(logits, float("-inf")).scatter(-1, sorted_idx, sorted_logits)
    probs = torch.softmax(logits, dim=-1)
    return torch.multinomial(probs, 1, generator=generator).squeeze(-1)


def select_threshold(scores: torch.Tensor, top_k: int = 0, top_p: float = 1.0) -> torch.Tensor:
    """The keep-threshold of every row of ``scores`` [B, V] under top-k then
    top-p (HF order): a token is kept iff its score is >= the threshold, so
    tied scores are kept together.  ``-inf`` scores are masked and never kept.

    top-k (``0 < k < V``): t_k is the k-th largest finite score (all finite
    scores stay when there are fewer than k).  top-p (``0 < p < 1``), over the
    top-k survivors: with w = exp(s - max s) and Z = sum w, s_i is kept iff
    the mass of the strictly larger survivors is <= p * Z (the maximum is
    always kept).  The threshold is the smallest kept score; ``-inf`` when no
    filter is active or the row has no finite score.  fp64 inside; returns
    fp32 [B] (exactly one of the row's scores).
    """
    V = scores.shape[-1]
    k_on = bool(top_k) and 0 < top_k < V
    p_on = top_p is not None and 0.0 < top_p < 1.0
    out = torch.full((scores.shape[0],), float("-inf"), dtype=torch.float32)
    if not (k_on or p_on):
        return out
    for b, row in enumerate(scores.detach().cpu().double()):
        s = row[row > float("-inf")].sort(descending=True).values
        if s.numel() == 0:
            continue
        if k_on:
            s = s[s >= s[min(top_k, s.numel()) - 1]]
        if p_on:
            w = torch.exp(s - s[0])
            # mass strictly above each score: ties share the mass above their first member
            first = torch.searchsorted(-s, -s, right=False)
            above = (w.cumsum(0) - w)[first]
            s = s[above <= top_p * w.sum()]
        out[b] = s[-1].float()
    return out


def causal_softmax(
    scores: torch.Tensor, start_pos: int = 0, key_starts: Optional[torch.Tensor] = None
) -> torch.Tensor:
    """Causal-masked softmax over the last dim of [B, H, Tq, Tk] scores.

    Query position i (global position start_pos + i) may attend to key
    positions <= start_pos + i; keys before ``key_starts[b]`` (left padding)
    are masked out.  Fully-masked rows produce zeros.
    """
    dtype = scores.dtype
    Tq, Tk = scores.shape[-2], scores.shape[-1]
    q_pos = torch.arange(Tq, device=scores.device).unsqueeze(-1) + start_pos
    k_pos = torch.arange(Tk, device=scores.device).unsqueeze(0)
    mask = (k_pos > q_pos).view(1, 1, Tq, Tk)
    if key_starts is not None:
        B = scores.shape[0]
        pad = k_pos.view(1, 1, 1, Tk) < key_starts.view(B, 1, 1, 1)
        mask = mask | pad
    scores = scores.float().masked_fill(mask, float("-inf"))
    probs = torch.softmax(scores, dim=-1)
    # rows with no valid keys (fully masked) -> 0 instead of NaN
    probs = torch.nan_to_num(probs, nan=0.0)
    return probs.to(dtype)


def fused_adamw(
    params: list,
    grads: list,
    exp_avgs: list,
    exp_avg_sqs: list,
    master_params: list,
    step: int,
    lr: float,
    beta1: float,
    beta2: float,
    eps: float,
    weight_decay: float,
) -> None:
    """Multi-tensor AdamW with fp32 master weights; params may be bf16 and are
    re-cast from the updated masters."""
    bc1 = 1 - beta1**step
    bc2 = 1 - beta2**step
    for p, g, m, v, mp in zip(params, grads, exp_avgs, exp_avg_sqs, master_params):
        gf = g.float()
        m.mul_(beta1).add_(gf, alpha=1 - beta1)
        v.mul_(beta2).addcmul_(gf, gf, value=1 - beta2)
        mp.mul_(1 - lr * weight_decay)
        denom = (v / bc2).sqrt_().add_(eps)
        mp.addcdiv_(m, denom, value=-lr / bc1)
        p.copy_(mp.to(p.dtype))


# ---- 8-bit AdamW (csrc/adamw8.hip; the state format is written out there) ----

ADAMW8_QB = 256  # elements per quantization block
_E4M3_MAX = 448.0
_U64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15


def _i64(c: int) -> int:
    """The int64 with the bits of the uint64 ``c``."""
    return c - (1 << 64) if c >= 1 << 63 else c


def _shr(z: torch.Tensor, k: int) -> torch.Tensor:
    """Logical right shift of int64 bits."""
    return (z >> k) & ((1 << (64 - k)) - 1)


def _splitmix64(z):
    """common.h splitmix64 on a python int (mod 2^64) or on int64 tensor bits."""
    if isinstance(z, int):
        z = (z + _GOLDEN) & _U64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _U64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _U64
        return z ^ (z >> 31)
    z = z + _i64(_GOLDEN)
    z = (z ^ _shr(z, 30)) * _i64(0xBF58476D1CE4E5B9)
    z = (z ^ _shr(z, 27)) * _i64(0x94D049BB133111EB)
    return z ^ _shr(z, 31)


def _f32(x: float) -> float:
    """``x`` rounded to fp32, as the kernel's float arguments are."""
    return torch.tensor(x, dtype=torch.float32).item()


def _sqrt32(x: torch.Tensor) -> torch.Tensor:
    """The correctly rounded fp32 square root, as sqrtf on the device is.  The CPU
    torch.sqrt of a large fp32 tensor is a vector-library call that is 1 ulp
    off for about 0.7 % of its inputs; rounding the fp64 root is exact (fp64
    carries more than twice fp32's bits plus two)."""
    return x.double().sqrt().float()


def _per_element(scales: torch.Tensor, n: int) -> torch.Tensor:
    return scales.repeat_interleave(ADAMW8_QB)[:n]


def adamw8_dequant(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """fp32 moments of e4m3 ``codes`` uint8 [n] and ``scales`` fp32 [ceil(n/256)]."""
    return codes.view(torch.float8_e4m3fn).float() * _per_element(scales, codes.numel())


def _adamw8_scales(x: torch.Tensor) -> torch.Tensor:
    """absmax of every 256-element block (a short tail block: of its real
    elements) times 1/448."""
    n = x.numel()
    nb = -(-n // ADAMW8_QB)
    padded = torch.zeros(nb * ADAMW8_QB, dtype=torch.float32, device=x.device)
    padded[:n] = x.abs()
    return padded.view(nb, ADAMW8_QB).amax(dim=1) * _f32(1.0 / _E4M3_MAX)


def _scaled(x: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """x / scale clamped to +-448; 0 in a block whose scale is 0."""
    s = _per_element(scales, x.numel())
    y = torch.where(s > 0, x / torch.where(s > 0, s, torch.ones_like(s)), torch.zeros_like(x))
    return y.clamp(-_E4M3_MAX, _E4M3_MAX)


def adamw8_stochastic_round(y: torch.Tensor, idx: torch.Tensor, seed: int,
                            step: int) -> torch.Tensor:
    """fp32 ``y`` in [0, 448] rounded down or up to the e4m3 grid, up with the
    probability of its fraction: e = max(floor(log2 y), -6), grid step 2^(e-3),
    q = min(floor(y / step + r) * step, 448) with r = (h >> 40) 2^-24 and
    h = splitmix64(key ^ splitmix64(idx)), key = splitmix64(seed ^ golden * step).
    ``idx`` int64: the elements' indices in the unsharded arena.  The min: the
    fp32 sum y / step + r can round up past a y on the grid (r within 2^-21 of
    1), and from 448, every block's absmax, the next step is 480, which e4m3
    does not have and would store as NaN."""
    key = _splitmix64((seed ^ (_GOLDEN * step)) & _U64)
    h = _splitmix64(_splitmix64(idx) ^ _i64(key))
    r = _shr(h, 40).float() * 2.0 ** -24
    e = (((y.view(torch.int32) >> 23) & 0xFF) - 127).clamp(min=-6)
    inv_step = ((130 - e) << 23).view(torch.float32)
    grid = ((124 + e) << 23).view(torch.float32)
    return (torch.floor(y * inv_step + r) * grid).clamp(max=_E4M3_MAX)


def adamw8_step(p, master, g, m8, m_scale, u8, u_scale, step: int, lr: float, beta1: float,
                beta2: float, eps: float, weight_decay: float, grad_scale: float = 1.0,
                seed: int = 0, index_base: int = 0) -> None:
    """One AdamW step on a flat arena with 8-bit moment state, in place: the CPU
    path of ``FusedAdamW8bit`` and the bit-level definition ``fused_adamw8`` is
    tested against.  m = e4m3(m8) * m_scale[block], u = sqrt(v) = e4m3(u8) *
    u_scale[block], one fp32 scale = absmax / 448 per 256 elements; m is encoded
    round-to-nearest-even, u by ``adamw8_stochastic_round``.  Every operation is
    one fp32 rounding, in the order of the kernel (no fused multiply-add)."""
    n = p.numel()
    lr, b1, b2, eps = _f32(lr), _f32(beta1), _f32(beta2), _f32(eps)
    omb1, omb2 = _f32(1.0 - b1), _f32(1.0 - b2)  # fp32 subtractions: exact in double
    lrwd = _f32(lr * _f32(weight_decay))
    # divisors as tensors: a tensor / python-scalar may multiply by the reciprocal
    bc1 = torch.full((n,), 1.0 - beta1 ** step, dtype=torch.float32)
    bc2 = torch.full((n,), 1.0 - beta2 ** step, dtype=torch.float32)

    gf = g.float() * _f32(grad_scale)
    u = adamw8_dequant(u8, u_scale)
    m = b1 * adamw8_dequant(m8, m_scale) + omb1 * gf
    v = b2 * (u * u) + omb2 * (gf * gf)
    w = master - lrwd * master
    w = w - (lr * (m / bc1)) / (_sqrt32(v / bc2) + eps)
    un = _sqrt32(v)

    new_ms, new_us = _adamw8_scales(m), _adamw8_scales(un)
    idx = torch.arange(index_base, index_base + n, dtype=torch.int64)
    q = adamw8_stochastic_round(_scaled(un, new_us), idx, seed, step)
    m8.copy_(_scaled(m, new_ms).to(torch.float8_e4m3fn).view(torch.uint8))
    u8.copy_(q.to(torch.float8_e4m3fn).view(torch.uint8))
    m_scale.copy_(new_ms)
    u_scale.copy_(new_us)
    master.copy_(w)
    if not (p.dtype == torch.float32 and p.data_ptr() == master.data_ptr()):
        p.copy_(w.to(p.dtype))


def kv_quantize_fp8(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The fp8 KV-cache format, bit for bit (csrc/kv_fp8.hip reproduces every
    code and scale): rows ``x[..., D]`` -> e4m3 ``codes`` uint8 ``[..., D]`` and
    one fp32 ``scale [...]`` per row.  scale = absmax / 448 (one fp32 division),
    code = round-to-nearest-even of x / scale clamped to +-448, so no NaN code
    (0x7F / 0xFF) is ever produced; an all-zero row has scale 0 and codes 0."""
    xf = x.float()
    amax = xf.abs().amax(dim=-1, keepdim=True)
    # divisor as a tensor: a tensor / python-scalar may multiply by the reciprocal
    scale = amax / torch.full_like(amax, _E4M3_MAX)
    live = scale > 0
    y = torch.where(live, xf / torch.where(live, scale, torch.ones_like(scale)),
                    torch.zeros_like(xf)).clamp(-_E4M3_MAX, _E4M3_MAX)
    return y.to(torch.float8_e4m3fn).view(torch.uint8), scale.squeeze(-1)


def kv_dequantize_fp8(codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """fp32 rows of ``kv_quantize_fp8``'s output: e4m3(code) * scale."""
    return codes.view(torch.float8_e4m3fn).float() * scale.unsqueeze(-1)


def kv_store_fp8(k, v, k8, k_scale, v8, v_scale, start) -> None:
    """Quantize k, v ``[B, Hkv, T, D]`` into the fp8 cache at positions
    ``start + t`` (clamped into the cache): ``start`` an int, a one-element
    tensor, or one position per batch row ``[B]``."""
    B, _, T, _ = k.shape
    S = k8.shape[2]
    if not torch.is_tensor(start):
        start = torch.tensor([int(start)])
    rows = start.reshape(-1).long().to(k8.device).expand(B)
    pos = (rows.view(B, 1) + torch.arange(T, device=k8.device).view(1, T)).clamp(0, S - 1)
    b = torch.arange(B, device=k8.device).view(B, 1)
    for x, codes, scale in ((k, k8, k_scale), (v, v8, v_scale)):
        c, s = kv_quantize_fp8(x)
        codes[b, :, pos] = c.transpose(1, 2)
        scale[b, :, pos] = s.transpose(1, 2)


def flash_prefill(q, k, v, key_starts=None, start_pos: int = 0, scale: float = 1.0, tk=None,
                  alibi_slopes=None):
    """fp32 reference for the flash prefill kernel (masking semantics match
    causal_softmax: key j visible to query i iff key_start <= j <= start_pos+i).
    ``alibi_slopes`` [Hq] adds slope[h] * max(j - key_start, 0) to the scaled
    scores (ALiBi; the bias depends on the key position only)."""
    B, Hq, T, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    tkv = int(tk) if tk else Sk
    kk = k[:, :, :tkv].float()
    vv = v[:, :, :tkv].float()
    if Hq != Hkv:
        rep = Hq // Hkv
        kk = kk.repeat_interleave(rep, dim=1)
        vv = vv.repeat_interleave(rep, dim=1)
    scores = torch.matmul(q.float() * scale, kk.transpose(-1, -2))
    i = torch.arange(T, device=q.device).view(1, 1, T, 1)
    j = torch.arange(tkv, device=q.device).view(1, 1, 1, tkv)
    mask = j <= (start_pos + i)
    if key_starts is not None:
        mask = mask & (j >= key_starts.view(B, 1, 1, 1).to(q.device))
    if alibi_slopes is not None:
        key_pos = j if key_starts is None else j - key_starts.view(B, 1, 1, 1).to(q.device)
        scores = scores + (alibi_slopes.float().to(q.device).view(1, Hq, 1, 1)
                           * key_pos.clamp(min=0).float())
    scores = scores.masked_fill(~mask, float("-inf"))
    probs = torch.softmax(scores, dim=-1)
    probs = torch.nan_to_num(probs, nan=0.0)
    return torch.matmul(probs, vv).to(q.dtype)


# --------------------------------------------------------------------------
# T5 / seq2seq attention: Toeplitz relative-position bias + arbitrary key mask
# --------------------------------------------------------------------------


def relative_position_bucket(relative_position: torch.Tensor, bidirectional: bool,
                             num_buckets: int, max_distance: int) -> torch.Tensor:
    """T5's log-bucketed relative positions (semantics of the T5 paper)."""
    ret = torch.zeros_like(relative_position)
    n = -relative_position
    if bidirectional:
        num_buckets //= 2
        ret = ret + (n < 0).long() * num_buckets
        n = n.abs()
    else:
        n = torch.clamp(n, min=0)
    max_exact = num_buckets // 2
    is_small = n < max_exact
    val_large = max_exact + (
        torch.log(n.float() / max_exact + 1e-9) / math.log(max_distance / max_exact)
        * (num_buckets - max_exact)
    ).long()
    val_large = torch.clamp(val_large, max=num_buckets - 1)
    return ret + torch.where(is_small, n, val_large)


def t5_rel_bias(table: torch.Tensor, q_len: int, k_len: int, q_offset: int = 0,
                bidirectional: bool = True, num_buckets: int = 32,
                max_distance: int = 128) -> Tuple[torch.Tensor, int]:
    """The T5 position bias as a per-head Toeplitz vector.

    The bias of (query position ``q_offset + i``, key ``j``) depends only on
    ``j - (q_offset + i)``, so ``[H, Tq, Tk]`` collapses to ``[H, L]`` with
    ``L = q_offset + q_len - 1 + k_len`` and relative position 0 at index
    ``bias_zero = q_offset + q_len - 1``:
    ``dense[h, i, j] == vec[h, j - (q_offset + i) + bias_zero]``.
    ``table``: the ``[num_buckets, H]`` embedding weight; the lookup is an
    embedding, so the result is differentiable with respect to it.
    Returns ``(vec [H, L] fp32 contiguous, bias_zero)``."""
    zero = q_offset + q_len - 1
    L = zero + k_len
    rel = torch.arange(L, device=table.device) - zero
    buckets = relative_position_bucket(rel, bidirectional, num_buckets, max_distance)
    vec = torch.nn.functional.embedding(buckets, table)  # [L, H]
    return vec.t().float().contiguous(), zero


def gather_rel_bias(rel_bias: torch.Tensor, bias_zero: int, q_len: int, k_len: int,
                    start_pos: int = 0) -> torch.Tensor:
    """Dense [H, Tq, Tk] bias from the Toeplitz vector of ``t5_rel_bias``
    (query row i stands at position ``start_pos + i``)."""
    qpos = torch.arange(q_len, device=rel_bias.device)[:, None] + start_pos
    key = torch.arange(k_len, device=rel_bias.device)[None, :]
    return rel_bias[:, key - qpos + bias_zero]


def seq2seq_attention(q, k, v, rel_bias=None, bias_zero: int = 0, key_mask=None,
                      causal: bool = False, start_pos: int = 0, scale: float = 1.0):
    """fp32 reference for the seq2seq (T5) modes of the flash kernels: q
    [B,Hq,Tq,D], k/v [B,Hkv,Tk,D] with Tq != Tk allowed.  The score of (query
    row i, key j) is ``scale * q.k + rel_bias[h, j - (start_pos + i) +
    bias_zero]``; key j is visible iff ``key_mask[b, j] != 0`` (any mask, not
    only padding) and, under ``causal``, ``j <= start_pos + i``.  A row with no
    visible key returns zeros."""
    B, Hq, Tq, D = q.shape
    Hkv, Tk = k.shape[1], k.shape[2]
    kk, vv = k.float(), v.float()
    if Hq != Hkv:
        kk = kk.repeat_interleave(Hq // Hkv, dim=1)
        vv = vv.repeat_interleave(Hq // Hkv, dim=1)
    scores = torch.matmul(q.float() * scale, kk.transpose(-1, -2))
    if rel_bias is not None:
        scores = scores + gather_rel_bias(rel_bias.float(), bias_zero, Tq, Tk, start_pos)[None]
    visible = torch.ones(B, 1, Tq, Tk, dtype=torch.bool, device=q.device)
    if key_mask is not None:
        visible = visible & (key_mask.to(q.device) != 0).view(B, 1, 1, Tk)
    if causal:
        i = torch.arange(Tq, device=q.device).view(1, 1, Tq, 1)
        j = torch.arange(Tk, device=q.device).view(1, 1, 1, Tk)
        visible = visible & (j <= start_pos + i)
    scores = scores.masked_fill(~visible, float("-inf"))
    probs = torch.nan_to_num(torch.softmax(scores, dim=-1), nan=0.0)
    return torch.matmul(probs, vv).to(q.dtype)


def seq2seq_decode_attention(q, k_new, v_new, k_cache, v_cache, cache_idx, rel_bias=None,
                             bias_zero: int = 0, scale: float = 1.0):
    """fp32 reference for the T5 self-attention decode step (csrc/s2s_decode.hip):
    q / k_new / v_new [B, H, D] are the projections of the one new token at
    position ``pos = cache_idx[0]``.  Writes k_new / v_new IN PLACE into row
    ``pos`` of the caches [B, H, S, D], then attends over keys 0..pos inclusive
    with score ``scale * q.k + rel_bias[h, clamp(key - pos + bias_zero, 0, L-1)]``.
    A ``pos`` outside [0, S) writes nothing and returns zeros, as the kernel
    does.  Returns [B, H, 1, D]."""
    B, H, D = q.shape
    S = k_cache.shape[2]
    pos = int(cache_idx.reshape(-1)[0])
    if not 0 <= pos < S:
        return torch.zeros(B, H, 1, D, dtype=q.dtype, device=q.device)
    k_cache[:, :, pos] = k_new.to(k_cache.dtype)
    v_cache[:, :, pos] = v_new.to(v_cache.dtype)
    kk = k_cache[:, :, : pos + 1].float()
    vv = v_cache[:, :, : pos + 1].float()
    scores = torch.matmul((q.float() * scale).unsqueeze(2), kk.transpose(-1, -2))  # [B,H,1,pos+1]
    if rel_bias is not None:
        L = rel_bias.shape[1]
        idx = (torch.arange(pos + 1, device=q.device) - pos + bias_zero).clamp(0, L - 1)
        scores = scores + rel_bias.float()[:, idx].view(1, H, 1, pos + 1)
    probs = torch.softmax(scores, dim=-1)
    return torch.matmul(probs, vv).to(q.dtype)


def seq2seq_cross_decode_attention(q, k, v, key_mask=None, scale: float = 1.0):
    """fp32 reference for the T5 cross-attention decode step: q [B, H, 1, D]
    against k / v [B, H, Tk, D]; key j of row b is visible iff
    ``key_mask[b, j] != 0`` (any mask).  Masked keys are skipped, not weighted
    by zero: non-finite K/V rows behind the mask do not reach the output.  A
    row with no visible key returns zeros."""
    B, H, _, D = q.shape
    Tk = k.shape[2]
    kk, vv = k.float(), v.float()
    visible = torch.ones(B, 1, 1, Tk, dtype=torch.bool, device=q.device)
    if key_mask is not None:
        visible = (key_mask.to(q.device) != 0).view(B, 1, 1, Tk)
        keep = visible.view(B, 1, Tk, 1)
        kk = torch.where(keep, kk, torch.zeros_like(kk))
        vv = torch.where(keep, vv, torch.zeros_like(vv))
    scores = torch.matmul(q.float() * scale, kk.transpose(-1, -2))
    scores = scores.masked_fill(~visible, float("-inf"))
    probs = torch.nan_to_num(torch.softmax(scores, dim=-1), nan=0.0)
    return torch.matmul(probs, vv).to(q.dtype)
