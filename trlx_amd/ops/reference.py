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
