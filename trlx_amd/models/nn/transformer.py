"""Native causal transformer for MI355X.

This is the compute path of the framework — the reference delegates it to HF
transformers + Apex/Megatron; here it is a single decoder
implementation whose hot ops (norms, RoPE, causal softmax, decode attention,
logprob gather, sampling) dispatch to the gfx950 HIP kernels in
``trlx_amd.ops``, with plain GEMMs on hipBLASLt via ``torch.nn.functional``.

Design points:
- one module covers GPT-2 / GPT-J / NeoX / OPT / Llama via TransformerConfig
  flags (no per-arch branch classes like reference modeling_ppo.py:547-1222);
- fused QKV / gate-up projections (one GEMM instead of 2-3);
- preallocated contiguous KV cache + fused flash-decode kernel for generation;
- ``forward(..., hidden_at_layer=k)`` returns the pre-layer-k hidden state so
  the hydra frozen branch (reference modeling_ppo.py:385-544) re-runs only the
  top layers without a second trunk pass;
- left-padded prompts carried as (position_ids, key_starts) instead of dense
  [B, 1, T, T] masks.
"""

import math
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops
from ...ops.reference import rope_cos_sin
from ...parallel import topo
from ...parallel.tp import ColumnParallelLinear, RowParallelLinear
from .config import TransformerConfig


class Norm(nn.Module):
    """RMSNorm/LayerNorm routed to the fused HIP kernels."""

    def __init__(self, cfg: TransformerConfig, hidden: Optional[int] = None):
        super().__init__()
        h = hidden or cfg.hidden_size
        self.kind = cfg.norm
        self.eps = cfg.norm_eps
        self.weight = nn.Parameter(torch.ones(h))
        self.bias = nn.Parameter(torch.zeros(h)) if cfg.norm == "layernorm" else None

    def forward(self, x):
        if self.kind == "rmsnorm":
            return ops.rmsnorm(x, self.weight, self.eps)
        return ops.layernorm(x, self.weight, self.bias, self.eps)

    def forward_add(self, x, res):
        """Fused residual + norm: returns (norm(x + res), x + res) in one
        kernel (the elementwise residual adds were 5.6% of cycle kernel time,
        profile r01)."""
        if self.kind == "rmsnorm":
            return ops.rmsnorm_add(x, res, self.weight, self.eps)
        return ops.layernorm_add(x, res, self.weight, self.bias, self.eps)


def alibi_slopes(num_heads: int) -> torch.Tensor:
    """Standard ALiBi head slopes (Bloom; closest-power-of-two scheme)."""

    def pow2_slopes(n):
        start = 2.0 ** (-(2.0 ** -(math.log2(n) - 3)))
        return [start * (start ** i) for i in range(n)]

    if math.log2(num_heads).is_integer():
        vals = pow2_slopes(num_heads)
    else:
        closest = 2 ** math.floor(math.log2(num_heads))
        vals = pow2_slopes(closest) + pow2_slopes(2 * closest)[0::2][: num_heads - closest]
    return torch.tensor(vals, dtype=torch.float32)


@dataclass
class AttentionContext:
    """Per-forward positional/masking state shared by all layers."""

    position_ids: torch.Tensor  # [B, T] int32
    key_starts: Optional[torch.Tensor]  # [B] int32 (left-pad offsets)
    start_pos: int  # global position of query 0 (decode steps)
    seq_lens: Optional[torch.Tensor] = None  # [B] int32 (decode: cache fill)
    # device scalar cache write index: enables the fused decode_prep kernel
    # and hipGraph capture (no host-side position state)
    cache_idx: Optional[torch.Tensor] = None
    # PER-ROW cache write positions [B] (continuous-batching decode: slots
    # sit at different depths); mutually exclusive with cache_idx
    cache_rows: Optional[torch.Tensor] = None
    # ALiBi (Bloom): per-head slopes [H_local] fp32.  The flash and decode
    # kernels take these directly and add slope * (key - key_start) in-tile
    alibi_slopes: Optional[torch.Tensor] = None
    # dense ALiBi bias [B, H_local, 1, T_keys]: built lazily by dense_alibi()
    # and ONLY for the materializing attention path (never in a graph step)
    alibi: Optional[torch.Tensor] = None
    # PREFIX_TUNING: per-layer K/V params + the cache positions they occupy
    prefix_kv: Optional[object] = None
    virtual_slots: Optional[torch.Tensor] = None  # [B, n] long

    def dense_alibi(self, batch: int, num_keys: int) -> torch.Tensor:
        """ALiBi bias per KEY position (Bloom semantics: mask-aware positions,
        pads at bias 0) as a dense [B, H_local, 1, num_keys] fp32 tensor that
        broadcasts over queries; cached across the layers of one forward."""
        if self.alibi is None or self.alibi.shape[-1] != num_keys:
            slopes = self.alibi_slopes
            j = torch.arange(num_keys, device=slopes.device).unsqueeze(0)
            ks = (self.key_starts.unsqueeze(1) if self.key_starts is not None
                  else torch.zeros(batch, 1, device=slopes.device))
            key_pos = (j - ks).clamp(min=0).float()  # [B, Tk]
            self.alibi = slopes.view(1, -1, 1, 1) * key_pos[:, None, None, :]
        return self.alibi


class KVCache:
    """Preallocated contiguous KV cache sized for HBM3E residency."""

    def __init__(self, num_layers: int, batch: int, num_kv_heads: int, max_len: int, head_dim: int,
                 device, dtype):
        # zero-init: unwritten slots must be finite (masked-out positions can
        # still flow through 0*x products in the eager reference path)
        self.k = [
            torch.zeros(batch, num_kv_heads, max_len, head_dim, device=device, dtype=dtype)
            for _ in range(num_layers)
        ]
        self.v = [
            torch.zeros(batch, num_kv_heads, max_len, head_dim, device=device, dtype=dtype)
            for _ in range(num_layers)
        ]
        self.max_len = max_len
        self.cur_len = 0

    def update(self, layer: int, k: torch.Tensor, v: torch.Tensor, start: int) -> Tuple[torch.Tensor, torch.Tensor]:
        T = k.shape[2]
        assert start + T <= self.max_len, "KV cache overflow"
        self.k[layer][:, :, start : start + T] = k
        self.v[layer][:, :, start : start + T] = v
        return self.k[layer], self.v[layer]

    def update_rows(self, layer: int, k: torch.Tensor, v: torch.Tensor,
                    rows: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Single-token append at PER-ROW positions (continuous batching:
        each slot decodes at its own depth).  k/v [B, Hkv, 1, D], rows [B]."""
        b = torch.arange(k.shape[0], device=k.device)
        self.k[layer][b, :, rows.long()] = k[:, :, 0]
        self.v[layer][b, :, rows.long()] = v[:, :, 0]
        return self.k[layer], self.v[layer]


class Attention(nn.Module):
    def __init__(self, cfg: TransformerConfig, layer_idx: int):
        super().__init__()
        self.cfg = cfg
        self.layer_idx = layer_idx
        tp = topo.tp_size()
        assert cfg.num_heads % tp == 0 and cfg.num_kv_heads % tp == 0, \
            f"heads ({cfg.num_heads}/{cfg.num_kv_heads}) must divide tp={tp}"
        # local (per-TP-rank) head counts; attention runs on the local shard
        self.num_heads = cfg.num_heads // tp
        self.num_kv_heads = cfg.num_kv_heads // tp
        self.head_dim = cfg.head_dim
        self.scale = cfg.attn_scale if cfg.attn_scale is not None else 1.0 / math.sqrt(cfg.head_dim)
        if tp > 1:
            # column-parallel qkv (head-aligned shard), row-parallel output
            self.qkv_proj = ColumnParallelLinear(cfg.hidden_size, cfg.qkv_out, bias=cfg.attn_bias)
            self.o_proj = RowParallelLinear(cfg.num_heads * cfg.head_dim, cfg.hidden_size,
                                            bias=cfg.attn_bias)
        else:
            self.qkv_proj = nn.Linear(cfg.hidden_size, cfg.qkv_out, bias=cfg.attn_bias)
            self.o_proj = nn.Linear(cfg.num_heads * cfg.head_dim, cfg.hidden_size, bias=cfg.attn_bias)
        self.rot = int(cfg.head_dim * cfg.rope_pct) if cfg.position_encoding == "rope" else 0
        if self.rot % 2:
            self.rot -= 1
        self.attn_pdrop = cfg.attn_pdrop

    def forward(self, x, ctx: AttentionContext, rope_tables, kv_cache: Optional[KVCache] = None):
        B = x.shape[0]
        qkv = dense(self.qkv_proj, x)
        # under sequence parallelism the projection gathers the full sequence
        T = qkv.shape[1]

        def project(out):  # attention output [B, H, T, D] -> o_proj of [B, T, H*D]
            return dense(self.o_proj, out.transpose(1, 2).reshape(B, T, -1))

        # fused single-token decode path: decode_prep (split+RoPE+cache
        # append) + flash-decode attention, fully device-side (hipGraph-safe)
        if (T == 1 and kv_cache is not None and ctx.cache_idx is not None
                and ctx.seq_lens is not None and x.is_cuda
                and self.head_dim in ops.DECODE_HEAD_DIMS):
            # (unsupported head dims fall through to the eager T=1 math below)
            cos_sin = rope_tables if self.cfg.position_encoding == "rope" else (None, None)
            if self.num_heads == self.num_kv_heads:
                # MHA: split+RoPE+append and attention in ONE kernel (the
                # per-head k/v append and the attention read are same-block)
                out = ops.fused_decode_attention(
                    qkv, kv_cache.k[self.layer_idx], kv_cache.v[self.layer_idx],
                    ctx.seq_lens, ctx.key_starts, cos_sin[0], cos_sin[1], ctx.cache_idx,
                    self.rot, self.cfg.rope_interleaved, self.scale,
                    alibi_slopes=ctx.alibi_slopes,
                )
            else:
                q = ops.decode_prep(
                    qkv, kv_cache.k[self.layer_idx], kv_cache.v[self.layer_idx], ctx.cache_idx,
                    self.num_heads, cos_sin[0], cos_sin[1], ctx.key_starts, self.rot,
                    self.cfg.rope_interleaved,
                )
                out = ops.attention_decode(q, kv_cache.k[self.layer_idx],
                                           kv_cache.v[self.layer_idx],
                                           ctx.seq_lens, self.scale, seq_starts=ctx.key_starts,
                                           alibi_slopes=ctx.alibi_slopes)
            return project(out)

        if x.is_cuda and x.dtype == torch.bfloat16 and ops.extension_available():
            # fused split + RoPE + q-scale (one kernel fwd, one bwd)
            use_rope = self.cfg.position_encoding == "rope"
            cos, sin = rope_tables if use_rope else (None, None)
            q, k, v = ops.qkv_prep(
                qkv, self.num_heads, self.num_kv_heads, self.head_dim, cos, sin,
                positions=ctx.position_ids if use_rope else None, qscale=self.scale,
                rot=self.rot, interleaved=self.cfg.rope_interleaved,
            )
            pre_scaled = True
        else:
            qd = self.num_heads * self.head_dim
            kd = self.num_kv_heads * self.head_dim
            q = qkv[..., :qd].view(B, T, self.num_heads, self.head_dim).transpose(1, 2).contiguous()
            k = qkv[..., qd : qd + kd].view(B, T, self.num_kv_heads, self.head_dim).transpose(1, 2).contiguous()
            v = qkv[..., qd + kd :].view(B, T, self.num_kv_heads, self.head_dim).transpose(1, 2).contiguous()
            pre_scaled = False

            if self.cfg.position_encoding == "rope":
                cos, sin = rope_tables
                q, k = ops.apply_rope(q, k, cos, sin, positions=ctx.position_ids,
                                      interleaved=self.cfg.rope_interleaved, rot=self.rot)

        if ctx.prefix_kv is not None:
            # PREFIX_TUNING: overwrite K/V at the virtual slots with this
            # layer's trained prefix (post-RoPE positions; prefixes unrotated)
            pk = ctx.prefix_kv.prefix_k[self.layer_idx].to(k.dtype)
            pv = ctx.prefix_kv.prefix_v[self.layer_idx].to(v.dtype)
            B_, n_ = ctx.virtual_slots.shape
            idx = ctx.virtual_slots.view(B_, 1, n_, 1).expand(B_, k.shape[1], n_, k.shape[3])
            k = k.scatter(2, idx, pk.unsqueeze(0).expand(B_, -1, -1, -1))
            v = v.scatter(2, idx, pv.unsqueeze(0).expand(B_, -1, -1, -1))

        # what both flash directions need; each adds its grad mode and gate
        flash_common = (
            T > 1 and x.is_cuda and q.dtype == torch.bfloat16
            and (self.attn_pdrop == 0 or not self.training)
            and ops.extension_available()
        )
        flash_ok = (
            flash_common and not torch.is_grad_enabled()
            # head dim + TRLX_AMD_NO_FLASH_PREFILL, per the measured defaults
            and ops.flash_enabled(self.head_dim, train=False)
        )
        if kv_cache is not None:
            if pre_scaled:
                # cache stores unscaled k (decode kernel scales q itself)
                pass
            if ctx.cache_rows is not None:
                k_full, v_full = kv_cache.update_rows(self.layer_idx, k, v, ctx.cache_rows)
            else:
                k_full, v_full = kv_cache.update(self.layer_idx, k, v, ctx.start_pos)
            if (T == 1 and ctx.seq_lens is not None
                    and (not x.is_cuda or self.head_dim in ops.DECODE_HEAD_DIMS)):
                # fused flash-decode kernel (qkv_prep may already have scaled
                # q: passing self.scale again double-scaled the PP/direct
                # decode path on GPU — caught by the ctx-level decode test)
                out = ops.attention_decode(q, k_full, v_full, ctx.seq_lens,
                                           1.0 if pre_scaled else self.scale,
                                           seq_starts=ctx.key_starts,
                                           alibi_slopes=ctx.alibi_slopes)
                return project(out)
            if flash_ok:
                # cache prefill through the flash kernel: reads the cache
                # tensors in place (allocated stride Sk, valid start_pos+T)
                out = ops.flash_prefill(q, k_full, v_full, ctx.key_starts, ctx.start_pos,
                                        1.0 if pre_scaled else self.scale,
                                        tk=ctx.start_pos + T, alibi_slopes=ctx.alibi_slopes)
                return project(out)
            k = k_full[:, :, : ctx.start_pos + T]
            v = v_full[:, :, : ctx.start_pos + T]
        elif flash_ok:
            # no_grad experience/training-free forward: online-softmax flash
            # attention — the [B, H, T, T] scores never materialize
            # (the memory wall at seq 1024-2048)
            out = ops.flash_prefill(q.contiguous(), k.contiguous(), v.contiguous(),
                                    ctx.key_starts, ctx.start_pos,
                                    1.0 if pre_scaled else self.scale,
                                    alibi_slopes=ctx.alibi_slopes)
            return project(out)

        flash_train_ok = (
            flash_common and torch.is_grad_enabled() and kv_cache is None and ctx.start_pos == 0
            # head dim + TRLX_AMD_NO_FLASH_PREFILL / TRLX_AMD_NO_FLASH_TRAIN
            and ops.flash_enabled(self.head_dim, train=True)
        )
        if flash_train_ok:
            # TRAINING forward: differentiable flash attention — forward saves
            # the row logsumexp, backward recomputes P tile-by-tile
            # (csrc/flash_backward.hip); [B, H, T, T] never materializes in
            # either direction
            out = ops.flash_attention(q, k, v, ctx.key_starts,
                                      1.0 if pre_scaled else self.scale,
                                      alibi_slopes=ctx.alibi_slopes)
            return project(out)

        # prefill / training: rocBLAS batched GEMMs + fused causal softmax
        if self.num_kv_heads != self.num_heads:
            rep = self.num_heads // self.num_kv_heads
            k = k.repeat_interleave(rep, dim=1)
            v = v.repeat_interleave(rep, dim=1)
        qs = q if pre_scaled else q * self.scale
        scores = torch.matmul(qs, k.transpose(-1, -2))
        if ctx.alibi_slopes is not None:
            # the one consumer of the dense [B, H, 1, Tk] bias (built here, on
            # demand: the kernels above take the slopes themselves)
            scores = scores + ctx.dense_alibi(B, scores.shape[-1]).to(scores.dtype)
        probs = ops.causal_softmax(scores.contiguous(), ctx.start_pos, ctx.key_starts)
        if self.attn_pdrop > 0 and self.training:
            probs = F.dropout(probs, self.attn_pdrop)
        out = torch.matmul(probs, v)
        return project(out)


def dense(lin, x, act_code=0, act_fn=None):
    """Projection dispatch: plain nn.Linear goes through the fused skinny
    streaming GEMM during decode (ops.skinny_linear handles eligibility);
    parallel linears keep their collective path, with the activation applied
    after."""
    if type(lin) is nn.Linear:
        return ops.skinny_linear(x, lin.weight, lin.bias, act_code)
    y = lin(x)
    return act_fn(y) if act_fn is not None else y


_ACTS = {
    "gelu": F.gelu,
    "gelu_new": lambda x: F.gelu(x, approximate="tanh"),
    "relu": F.relu,
    "silu": F.silu,
}


class MLP(nn.Module):
    def __init__(self, cfg: TransformerConfig):
        super().__init__()
        self.swiglu = cfg.swiglu
        tp = topo.tp_size()
        i = cfg.intermediate_size
        assert i % tp == 0, f"intermediate {i} must divide tp={tp}"
        if tp > 1:
            if cfg.swiglu:
                self.gate_up_proj = ColumnParallelLinear(cfg.hidden_size, 2 * i, bias=cfg.mlp_bias)
            else:
                self.fc_in = ColumnParallelLinear(cfg.hidden_size, i, bias=cfg.mlp_bias)
            self.down_proj = RowParallelLinear(i, cfg.hidden_size, bias=cfg.mlp_bias)
        else:
            if cfg.swiglu:
                self.gate_up_proj = nn.Linear(cfg.hidden_size, 2 * i, bias=cfg.mlp_bias)
            else:
                self.fc_in = nn.Linear(cfg.hidden_size, i, bias=cfg.mlp_bias)
            self.down_proj = nn.Linear(i, cfg.hidden_size, bias=cfg.mlp_bias)
        self.act = _ACTS[cfg.activation]
        self.act_code = ops.ACT_CODES.get(cfg.activation)
        self.isize = i // tp

    def forward(self, x):
        if self.swiglu:
            gu = dense(self.gate_up_proj, x)
            return dense(self.down_proj, self.act(gu[..., : self.isize]) * gu[..., self.isize :])
        if self.act_code is None:
            return dense(self.down_proj, self.act(dense(self.fc_in, x)))
        return dense(self.down_proj, dense(self.fc_in, x, self.act_code, self.act))


class Block(nn.Module):
    def __init__(self, cfg: TransformerConfig, layer_idx: int):
        super().__init__()
        self.cfg = cfg
        self.ln_1 = Norm(cfg)
        self.attn = Attention(cfg, layer_idx)
        # GPT-J shares one norm for the parallel branches; NeoX has two
        self.shared_parallel_norm = cfg.parallel_residual and cfg.arch_name == "gptj"
        if not self.shared_parallel_norm:
            self.ln_2 = Norm(cfg)
        self.mlp = MLP(cfg)
        self.resid_pdrop = cfg.resid_pdrop

    def _drop(self, x):
        if self.resid_pdrop > 0 and self.training:
            return F.dropout(x, self.resid_pdrop)
        return x

    def forward(self, x, ctx, rope_tables, kv_cache=None, res=None):
        """Deferred-residual protocol: the true stream at block input is
        ``x + res`` (res=None means x IS the stream).  The pending add is
        fused into this block's first norm; the block returns its own
        pending pair (branch_out, stream) for the next block.
        """
        if self.cfg.parallel_residual:
            if res is None:
                s = x
                h1 = self.ln_1(x)
            else:
                h1, s = self.ln_1.forward_add(x, res)
            h2 = h1 if self.shared_parallel_norm else self.ln_2(s)
            out = self._drop(self.attn(h1, ctx, rope_tables, kv_cache)) + self._drop(self.mlp(h2))
            return out, s
        if res is None:
            s = x
            h1 = self.ln_1(x)
        else:
            h1, s = self.ln_1.forward_add(x, res)
        a = self._drop(self.attn(h1, ctx, rope_tables, kv_cache))
        h2, s2 = self.ln_2.forward_add(a, s)
        m = self._drop(self.mlp(h2))
        return m, s2


def insert_virtual_rows(h, attention_mask, n, virt_values=None):
    """Insert ``n`` virtual slots BETWEEN each row's left pads and its real
    tokens (the pad-aware analog of peft's prepend: the masked prefix stays
    contiguous, so key_starts/flash-kernel semantics hold unchanged).

    Returns (h2 [B,T+n,H], mask2 [B,T+n], slots [B,n] cache positions of the
    virtual tokens, strip_idx [B,T] gather indices recovering the real
    positions from a T+n-length output).  ``virt_values`` [n, H] fills the
    slots (zeros when None — prefix tuning overwrites K/V per layer anyway).
    """
    B, T, H = h.shape
    device = h.device
    if attention_mask is not None:
        p = (T - attention_mask.sum(-1)).long()  # left-pad count per row
    else:
        p = torch.zeros(B, dtype=torch.long, device=device)
    pos = torch.arange(T + n, device=device).unsqueeze(0)  # [1, T+n]
    pe = p.unsqueeze(1)
    is_virt = (pos >= pe) & (pos < pe + n)
    src = torch.where(pos < pe, pos, (pos - n).clamp(min=0)).clamp(max=T - 1)
    h2 = torch.gather(h, 1, src.unsqueeze(-1).expand(B, T + n, H))
    if virt_values is not None:
        virt_idx = (pos - pe).clamp(0, n - 1)
        vfill = virt_values[virt_idx]  # [B, T+n, H]
        h2 = torch.where(is_virt.unsqueeze(-1), vfill.to(h2.dtype), h2)
    else:
        h2 = h2.masked_fill(is_virt.unsqueeze(-1), 0)
    if attention_mask is not None:
        mask2 = torch.where(is_virt, torch.ones_like(is_virt, dtype=attention_mask.dtype),
                            torch.gather(attention_mask, 1, src))
    else:
        mask2 = is_virt.to(torch.long) | (pos >= pe + n).to(torch.long)
        mask2 = torch.ones(B, T + n, dtype=torch.long, device=device)
    slots = pe + torch.arange(n, device=device).unsqueeze(0)  # [B, n]
    t_pos = torch.arange(T, device=device).unsqueeze(0)
    strip_idx = torch.where(t_pos < pe, t_pos, t_pos + n)  # [B, T]
    return h2, mask2, slots, strip_idx


def _strip_virtual(t, strip_idx):
    """Gather the real positions back out of a T+n-length tensor."""
    if t is None:
        return None
    B, T = strip_idx.shape
    if t.dim() == 3:
        return torch.gather(t, 1, strip_idx.unsqueeze(-1).expand(B, T, t.shape[-1]))
    return torch.gather(t, 1, strip_idx)


@dataclass
class TransformerOutput:
    logits: Optional[torch.Tensor] = None
    last_hidden_state: Optional[torch.Tensor] = None
    hidden_at_layer: Optional[torch.Tensor] = None


class CausalTransformer(nn.Module):
    """The native decoder-only LM."""

    def __init__(self, config: TransformerConfig):
        super().__init__()
        self.config = config
        cfg = config
        self.embed_tokens = nn.Embedding(cfg.vocab_size, cfg.hidden_size)
        if cfg.position_encoding == "learned":
            off = cfg.extra.get("position_offset", 0)
            self.embed_positions = nn.Embedding(cfg.max_position_embeddings + off, cfg.hidden_size)
        else:
            self.embed_positions = None
        self.embed_norm = Norm(cfg) if cfg.extra.get("pre_embed_norm") else None
        self.layers = nn.ModuleList(Block(cfg, i) for i in range(cfg.num_layers))
        self.final_norm = Norm(cfg)
        self.lm_head = nn.Linear(cfg.hidden_size, cfg.vocab_size, bias=cfg.lm_head_bias)
        if cfg.tie_word_embeddings:
            self.lm_head.weight = self.embed_tokens.weight
        self.embd_pdrop = cfg.embd_pdrop
        self.gradient_checkpointing = False
        # PEFT virtual-token adapters (models/lora.py apply_peft):
        # PROMPT_TUNING sets soft_prompt, PREFIX_TUNING sets prefix_kv
        self.soft_prompt = None
        self.prefix_kv = None
        self.num_virtual_tokens = 0
        if cfg.position_encoding == "rope":
            rot = int(cfg.head_dim * cfg.rope_pct)
            rot -= rot % 2
            cos, sin = rope_cos_sin(cfg.max_position_embeddings, rot, cfg.rope_base)
            self.register_buffer("rope_cos", cos, persistent=False)
            self.register_buffer("rope_sin", sin, persistent=False)
        else:
            self.rope_cos = self.rope_sin = None
        # ALiBi head slopes (this TP rank's heads), built once: a per-forward
        # host->device copy could not be captured into the decode graph
        self.register_buffer("alibi_slopes", self._local_alibi_slopes(), persistent=False)
        self.sequence_parallel = False
        self.apply(self._init_weights)

    def _local_alibi_slopes(self) -> Optional[torch.Tensor]:
        if self.config.position_encoding != "alibi":
            return None
        slopes = alibi_slopes(self.config.num_heads)
        tp = topo.tp_size()
        if tp > 1:
            hl = self.config.num_heads // tp
            slopes = slopes[topo.tp_rank() * hl : (topo.tp_rank() + 1) * hl].contiguous()
        return slopes

    def _apply(self, fn, *args, **kwargs):
        # .to(bf16)/.half() cast every floating buffer; the kernels need the
        # slopes in fp32 at full precision, so rebuild them after a dtype cast
        super()._apply(fn, *args, **kwargs)
        buf = self._buffers.get("alibi_slopes")
        if buf is not None and buf.dtype != torch.float32:
            self._buffers["alibi_slopes"] = self._local_alibi_slopes().to(buf.device)
        return self

    def set_sequence_parallel(self, enabled: bool):
        """Toggle Megatron-style sequence parallelism (activations sharded
        along T across the TP group in the norm/residual segments; gathered at
        column-parallel inputs, reduce-scattered at row-parallel outputs).
        The reference flips this around generation (modeling_nemo_ppo.py:
        820-836); here SP engages automatically only for cache-less forwards
        with T divisible by the TP size."""
        from ...parallel.tp import ColumnParallelLinear, RowParallelLinear

        self.sequence_parallel = enabled
        for m in self.modules():
            if isinstance(m, (ColumnParallelLinear, RowParallelLinear)):
                m.sequence_parallel = enabled

    def _init_weights(self, module):
        if isinstance(module, (nn.Linear, ColumnParallelLinear, RowParallelLinear)):
            module.weight.data.normal_(mean=0.0, std=0.02)
            if module.bias is not None:
                module.bias.data.zero_()
        elif isinstance(module, nn.Embedding):
            module.weight.data.normal_(mean=0.0, std=0.02)

    # --- helpers -----------------------------------------------------------

    def _sp_flags_on(self) -> bool:
        from ...parallel.tp import ColumnParallelLinear

        for m in self.modules():
            if isinstance(m, ColumnParallelLinear):
                return m.sequence_parallel
        return False

    def _set_sp_flags(self, enabled: bool):
        from ...parallel.tp import ColumnParallelLinear, RowParallelLinear

        for m in self.modules():
            if isinstance(m, (ColumnParallelLinear, RowParallelLinear)):
                m.sequence_parallel = enabled

    def embed_parameters(self):
        params = list(self.embed_tokens.parameters())
        if self.embed_positions is not None:
            params += list(self.embed_positions.parameters())
        return params

    @property
    def rope_tables(self):
        return (self.rope_cos, self.rope_sin) if self.rope_cos is not None else None

    def make_context(self, input_ids, attention_mask, start_pos: int,
                     seq_lens: Optional[torch.Tensor] = None,
                     key_starts: Optional[torch.Tensor] = None,
                     position_ids: Optional[torch.Tensor] = None) -> AttentionContext:
        B, T = input_ids.shape[:2]
        device = input_ids.device
        if position_ids is not None:
            position_ids = position_ids.to(torch.int32)
        elif attention_mask is not None:
            mask = attention_mask.to(torch.int32)
            position_ids = (mask.cumsum(-1) - 1).clamp(min=0).to(torch.int32)
            key_starts = (T - mask.sum(-1)).to(torch.int32)  # left-pad counts
        else:
            position_ids = (
                torch.arange(start_pos, start_pos + T, device=device, dtype=torch.int32)
                .unsqueeze(0).expand(B, T).contiguous()
            )
        return AttentionContext(position_ids=position_ids, key_starts=key_starts,
                                start_pos=start_pos, seq_lens=seq_lens,
                                alibi_slopes=self.alibi_slopes)

    def run_layers(self, h, ctx, kv_cache=None, from_layer: int = 0, to_layer: Optional[int] = None):
        to_layer = len(self.layers) if to_layer is None else to_layer
        res = None
        for i in range(from_layer, to_layer):
            h, res = self.layers[i](h, ctx, self.rope_tables, kv_cache, res=res)
        return h if res is None else h + res

    # --- main entry --------------------------------------------------------

    def forward(
        self,
        input_ids: torch.Tensor,
        attention_mask: Optional[torch.Tensor] = None,
        position_ids: Optional[torch.Tensor] = None,
        kv_cache: Optional[KVCache] = None,
        start_pos: int = 0,
        seq_lens: Optional[torch.Tensor] = None,
        key_starts: Optional[torch.Tensor] = None,
        hidden_at_layer: Optional[int] = None,
        return_logits: bool = True,
        cache_idx: Optional[torch.Tensor] = None,
        cache_rows: Optional[torch.Tensor] = None,
        logits_slice: Optional[Tuple[int, int]] = None,
    ) -> TransformerOutput:
        """hidden_at_layer=k stashes the hidden state FED INTO layer k
        (negative counts from the end: -2 = input of the 2nd-to-last layer)."""
        # PEFT virtual tokens: insert adapter slots between each row's left
        # pads and real tokens at prefill/training time (decode steps reuse
        # the prefix already in the KV cache); outputs are stripped back to
        # the caller's T positions at the end
        nv = self.num_virtual_tokens if (self.soft_prompt is not None
                                         or self.prefix_kv is not None) else 0
        strip_idx = None
        if nv and start_pos == 0 and cache_idx is None:
            h = self.embed_tokens(input_ids)
            virt = self.soft_prompt.embeddings if self.soft_prompt is not None else None
            h, attention_mask, slots, strip_idx = insert_virtual_rows(h, attention_mask, nv, virt)
            ctx = self.make_context(h[..., 0], attention_mask, start_pos, seq_lens, None, None)
            ctx.cache_idx = cache_idx
            if self.prefix_kv is not None:
                ctx.prefix_kv = self.prefix_kv
                ctx.virtual_slots = slots
        else:
            ctx = self.make_context(input_ids, attention_mask, start_pos, seq_lens, key_starts,
                                    position_ids)
            ctx.cache_idx = cache_idx
            ctx.cache_rows = cache_rows
            h = self.embed_tokens(input_ids)
        if self.embed_norm is not None:
            h = self.embed_norm(h)
        if self.embed_positions is not None:
            off = self.config.extra.get("position_offset", 0)
            h = h + self.embed_positions(ctx.position_ids.long() + off)
        if self.embd_pdrop > 0 and self.training:
            h = F.dropout(h, self.embd_pdrop)

        # sequence parallelism: shard activations along T for the
        # norm/residual segments (SP stays off for KV-cached generation)
        sp_active = (self.sequence_parallel and topo.tp_size() > 1 and kv_cache is None
                     and input_ids.shape[1] % topo.tp_size() == 0)
        if sp_active != self._sp_flags_on():
            self._set_sp_flags(sp_active)
        if sp_active:
            from ...parallel.tp import scatter_to_sp

            h = scatter_to_sp(h)

        n = len(self.layers)
        # hidden_at_layer: int -> single stash (tensor result); list of ints
        # -> multiple stashes (dict result, keyed by the REQUESTED values) —
        # the hydra reference branch and the trainable value branch can hook
        # different depths
        multi = isinstance(hidden_at_layer, (list, tuple))
        wanted = list(hidden_at_layer) if multi else (
            [hidden_at_layer] if hidden_at_layer is not None else [])
        stash_for = {}
        for w in wanted:
            stash_for.setdefault(w % n, []).append(w)
        hidden_at = {} if multi else None
        res = None
        use_ckpt = self.gradient_checkpointing and self.training and torch.is_grad_enabled()
        for i, layer in enumerate(self.layers):
            if i in stash_for:
                # materialize the true stream at this layer's input (the
                # pending residual is otherwise deferred into its norm)
                stream = h if res is None else h + res
                if multi:
                    for w in stash_for[i]:
                        hidden_at[w] = stream
                else:
                    hidden_at = stream
            if use_ckpt:
                # activation checkpointing: recompute the
                # block in backward instead of saving activations
                h, res = torch.utils.checkpoint.checkpoint(
                    lambda hh, rr, _l=layer: _l(hh, ctx, self.rope_tables, kv_cache, res=rr),
                    h, res, use_reentrant=False)
            else:
                h, res = layer(h, ctx, self.rope_tables, kv_cache, res=res)
        if res is None:
            h = self.final_norm(h)
        else:
            h, _ = self.final_norm.forward_add(h, res)
        if sp_active:
            # the loss region downstream is replicated on every TP rank ->
            # slice-backward gather (see _GatherFromSPReplicated)
            from ...parallel.tp import gather_from_sp_replicated

            h = gather_from_sp_replicated(h)
            if isinstance(hidden_at, dict):
                hidden_at = {k: gather_from_sp_replicated(v) for k, v in hidden_at.items()}
            elif hidden_at is not None:
                hidden_at = gather_from_sp_replicated(hidden_at)
        if strip_idx is not None:
            # drop the virtual positions: callers see their original T
            h = _strip_virtual(h, strip_idx)
            if isinstance(hidden_at, dict):
                hidden_at = {kk: _strip_virtual(v, strip_idx) for kk, v in hidden_at.items()}
            elif hidden_at is not None:
                hidden_at = _strip_virtual(hidden_at, strip_idx)
        logits = None
        if return_logits:
            # logits_slice: compute the [V]-wide projection only where the
            # loss needs it (PPO: response positions — the lm_head GEMM and
            # its backward are the largest single kernels in the train step)
            # .contiguous(): a T-slice view makes the lm_head GEMM run as a
            # B-batched strided GEMM with M=resp_len per batch (measured
            # 480 us vs 152 us for the flat [B*resp, V] GEMM)
            hs = h if logits_slice is None else h[:, logits_slice[0] : logits_slice[1]].contiguous()
            logits = self.lm_head(hs)
        return TransformerOutput(logits=logits, last_hidden_state=h, hidden_at_layer=hidden_at)

    def new_kv_cache(self, batch: int, max_len: int, device=None, dtype=None) -> KVCache:
        p = next(self.parameters())
        kv_heads_local = self.config.num_kv_heads // topo.tp_size()
        return KVCache(len(self.layers), batch, kv_heads_local, max_len,
                       self.config.head_dim, device or p.device, dtype or p.dtype)

    def num_parameters(self) -> int:
        return sum(p.numel() for p in self.parameters())
