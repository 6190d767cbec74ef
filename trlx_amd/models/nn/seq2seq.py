"""Native T5-family encoder-decoder transformer.

Parity target: the reference's seq2seq support (SURVEY.md C11 seq2seq
wrappers, flan-t5 examples).  Architecture follows T5: RMSNorm (the fused HIP
kernel), relative-position-bucket attention bias held by layer 0 of each
stack, UNSCALED q@k^T scores, relu or gated-gelu FFN, and the d_model^-0.5
output rescale under tied embeddings.

Attention: full-sequence passes (encoder, teacher-forced decoder, cross-
attention, the hydra and value branches) can run in the gfx950 flash kernels'
seq2seq modes (``ops.seq2seq_attention``: non-causal, Toeplitz relative-
position bias, arbitrary key mask, Tq != Tk) — bf16 on the GPU, head dim 64 or
128, and ``ops.seq2seq_flash_enabled`` (on by default at both head dims, see
profiles/t5_attention_notes.md; ``TRLX_AMD_NO_FLASH_PREFILL`` /
``TRLX_AMD_NO_FLASH_TRAIN`` = 1 turn it off).  The kernels produce no gradient for the
learned bias, so a layer whose bias table requires grad keeps the eager path
(rocBLAS GEMMs + additive-bias softmax) under grad mode: with
``num_layers_unfrozen > 0`` the tables are frozen and every attention
qualifies; a fully unfrozen T5 trains its self-attention eager (its cross-
attention and its no_grad passes still qualify).  Everything on CPU stays
eager.  Dropout is not applied to attention probabilities on either path.
Norms, logprob gathers and sampling hit the gfx950 kernels.

Generation: on the GPU in bf16 at a head dim in
``ops.SEQ2SEQ_DECODE_HEAD_DIMS`` (64, 128) the per-token step is
``decode_step`` over a preallocated ``Seq2SeqDecodeState`` — self-attention
caches appended in place at a device-side index, cross K/V projected once per
call into static buffers, a uint8 key mask, the decoder's Toeplitz bias vector
recomputed from the table on every call — through the two decode kernels of
csrc/s2s_decode.hip, and ``generation.Seq2SeqDecodeEngine`` replays it as one
hipGraph per token (``TRLX_AMD_NO_GRAPHS=1`` or a shaping fn that is not
graph-safe: the same kernels in a plain loop).  ``TRLX_AMD_NO_S2S_DECODE=1``,
other head dims, other dtypes and the CPU keep the eager ``past_kv`` loop
(``torch.cat`` cache, dense bias, additive masks), which measured 3.6-4.9x
slower at t5-small size (profiles/t5_decode_notes.md).
"""

from dataclasses import dataclass, field
from typing import Any, Dict, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops
from ...ops.reference import relative_position_bucket  # noqa: F401  (re-exported)


@dataclass
class Seq2SeqConfig:
    vocab_size: int = 32128
    d_model: int = 512
    d_kv: int = 64
    num_heads: int = 8
    d_ff: int = 2048
    num_layers: int = 6
    num_decoder_layers: Optional[int] = None
    relative_attention_num_buckets: int = 32
    relative_attention_max_distance: int = 128
    layer_norm_epsilon: float = 1e-6
    feed_forward_proj: str = "relu"  # "relu" | "gated-gelu"
    dropout_rate: float = 0.0
    tie_word_embeddings: bool = True
    decoder_start_token_id: int = 0
    pad_token_id: int = 0
    eos_token_id: int = 1
    arch_name: str = "t5"
    extra: Dict[str, Any] = field(default_factory=dict)

    def __post_init__(self):
        if self.num_decoder_layers is None:
            self.num_decoder_layers = self.num_layers

    @property
    def is_gated(self) -> bool:
        return self.feed_forward_proj.startswith("gated")

    def to_dict(self):
        return dict(self.__dict__)

    @classmethod
    def from_dict(cls, d):
        return cls(**d)


class T5Norm(nn.Module):
    """T5LayerNorm == RMSNorm (the fused HIP kernel path)."""

    def __init__(self, d_model: int, eps: float):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d_model))
        self.eps = eps

    def forward(self, x):
        return ops.rmsnorm(x, self.weight, self.eps)


def _extend_mask(mask: Optional[torch.Tensor], dtype=torch.float32) -> Optional[torch.Tensor]:
    """[B, T] 1/0 -> additive [B, 1, 1, T]."""
    if mask is None:
        return None
    return (1.0 - mask[:, None, None, :].float()) * torch.finfo(dtype).min


class RelBias:
    """The position bias of one pass over a stack, in both forms, each built
    lazily where its path runs: ``dense()`` is ``owner.compute_bias`` ([1, H,
    Tq, Tk], the eager path's additive bias) and ``vec()`` the Toeplitz vector
    ``(rel_bias [H, L] fp32, bias_zero)`` the kernels read.  ``owner`` is the
    attention layer that holds the table."""

    def __init__(self, owner: "T5Attention", q_len: int, k_len: int, device, q_offset: int = 0):
        self.owner, self.q_len, self.k_len, self.q_offset = owner, q_len, k_len, q_offset
        self.device = device
        self._dense = None
        self._vec = None

    @property
    def table(self) -> torch.Tensor:
        return self.owner.relative_attention_bias.weight

    def dense(self) -> torch.Tensor:
        if self._dense is None:
            self._dense = self.owner.compute_bias(self.q_len, self.k_len, self.device,
                                                  q_offset=self.q_offset)
        return self._dense

    def vec(self) -> Tuple[torch.Tensor, int]:
        if self._vec is None:
            cfg = self.owner.cfg
            self._vec = ops.t5_rel_bias(
                self.table, self.q_len, self.k_len, self.q_offset, self.owner.bidirectional,
                cfg.relative_attention_num_buckets, cfg.relative_attention_max_distance)
        return self._vec


class AttnMask:
    """What one attention call may see, in both forms: the raw ``key_mask``
    [B, Tk] (1 = visible, or None) plus the ``causal`` flag for the kernels,
    and ``additive()``, the [B, 1, Tq, Tk] float mask the eager path adds to
    the scores — built on first use only (like make_context's ALiBi bias)."""

    def __init__(self, key_mask: Optional[torch.Tensor], causal: bool = False, q_len: int = 0,
                 past_len: int = 0, device=None):
        self.key_mask, self.causal = key_mask, causal
        self.q_len, self.past_len, self.device = q_len, past_len, device
        self._additive = None
        self._built = False
        self._uint8 = None

    def uint8(self) -> Optional[torch.Tensor]:
        """``key_mask`` as the contiguous uint8 [B, Tk] the kernels read,
        converted once per pass, not once per attention call."""
        if self._uint8 is None and self.key_mask is not None:
            km = self.key_mask
            if km.dtype != torch.uint8:
                km = (km != 0).to(torch.uint8)
            self._uint8 = km.contiguous()
        return self._uint8

    def additive(self) -> Optional[torch.Tensor]:
        if not self._built:
            self._built = True
            mask = None
            if self.causal:  # causal mask over [T, past+T]
                total = self.past_len + self.q_len
                causal = torch.ones(self.q_len, total, device=self.device).tril(
                    diagonal=self.past_len)
                mask = (1.0 - causal[None, None]) * torch.finfo(torch.float32).min
                if self.key_mask is not None:
                    mask = mask + _extend_mask(self.key_mask)
            else:
                mask = _extend_mask(self.key_mask)
            self._additive = mask
        return self._additive


@dataclass
class AttnContext:
    """Masks of one pass over a stack: ``self_attn`` for the stack's own
    tokens, ``cross`` for the encoder keys (decoder stacks only)."""
    self_attn: AttnMask
    cross: Optional[AttnMask] = None


def encoder_context(attention_mask: Optional[torch.Tensor]) -> AttnContext:
    return AttnContext(AttnMask(attention_mask))


def decoder_context(q_len: int, device, attention_mask: Optional[torch.Tensor] = None,
                    decoder_attention_mask: Optional[torch.Tensor] = None,
                    past_len: int = 0) -> AttnContext:
    """The one place decoder-side masks are built: ``Seq2SeqTransformer.decode``,
    the hydra branch and the value branch all pass over decoder blocks with a
    causal self-attention mask (+ optional decoder padding) and the encoder's
    padding mask on the cross-attention."""
    return AttnContext(
        AttnMask(decoder_attention_mask, causal=True, q_len=q_len, past_len=past_len,
                 device=device),
        AttnMask(attention_mask))


def run_decoder_blocks(blocks, hidden, enc_out, attention_mask=None,
                       decoder_attention_mask=None, position_bias=None):
    """Full-sequence pass of ``hidden`` through decoder ``blocks`` (the model's
    own top layers or a branch's copies of them) with the decoder-side masks."""
    ctx = decoder_context(hidden.shape[1], hidden.device, attention_mask,
                          decoder_attention_mask)
    h = hidden
    for block in blocks:
        h, position_bias, _, _ = block(h, enc_out=enc_out, position_bias=position_bias, ctx=ctx)
    return h


def _on_gpu_bf16(t: torch.Tensor) -> bool:
    return t.is_cuda and t.dtype == torch.bfloat16


class T5Attention(nn.Module):
    def __init__(self, cfg: Seq2SeqConfig, has_bias: bool, bidirectional: bool):
        super().__init__()
        inner = cfg.num_heads * cfg.d_kv
        self.q = nn.Linear(cfg.d_model, inner, bias=False)
        self.k = nn.Linear(cfg.d_model, inner, bias=False)
        self.v = nn.Linear(cfg.d_model, inner, bias=False)
        self.o = nn.Linear(inner, cfg.d_model, bias=False)
        self.num_heads = cfg.num_heads
        self.d_kv = cfg.d_kv
        self.bidirectional = bidirectional
        self.cfg = cfg
        self.relative_attention_bias = (
            nn.Embedding(cfg.relative_attention_num_buckets, cfg.num_heads) if has_bias else None
        )

    def compute_bias(self, q_len: int, k_len: int, device, q_offset: int = 0) -> torch.Tensor:
        """[1, H, Tq, Tk] additive bias."""
        ctx = torch.arange(q_len, device=device)[:, None] + q_offset
        mem = torch.arange(k_len, device=device)[None, :]
        rel = mem - ctx
        buckets = relative_position_bucket(
            rel, self.bidirectional, self.cfg.relative_attention_num_buckets,
            self.cfg.relative_attention_max_distance,
        )
        bias = self.relative_attention_bias(buckets)  # [Tq, Tk, H]
        return bias.permute(2, 0, 1).unsqueeze(0)

    def _shape(self, x, B, T):
        return x.view(B, T, self.num_heads, self.d_kv).transpose(1, 2)

    def _takes_kernel(self, q, k, v, mask, position_bias, past_kv, attn_mask) -> bool:
        """Does this call run in ``ops.seq2seq_attention``?  A full-sequence
        pass on the GPU in bf16 whose masks came as an ``AttnMask`` and whose
        bias (if any) as a ``RelBias`` with a table that gets no gradient."""
        if attn_mask is None or mask is not None or past_kv is not None:
            return False
        if not (_on_gpu_bf16(q) and _on_gpu_bf16(k) and _on_gpu_bf16(v)):
            return False
        grad = torch.is_grad_enabled()
        if position_bias is not None:
            if not isinstance(position_bias, RelBias):
                return False
            if grad and position_bias.table.requires_grad:
                return False  # the kernels produce no gradient for the learned bias
        train = grad and (q.requires_grad or k.requires_grad or v.requires_grad)
        return ops.seq2seq_flash_enabled(self.d_kv, train)

    def forward(self, x, kv_input=None, mask=None, position_bias=None, past_kv=None,
                attn_mask: Optional[AttnMask] = None):
        """``mask``: additive float mask [B, 1, Tq, Tk] (0 / -inf), or
        ``attn_mask``: the same visibility as an ``AttnMask`` (raw key mask +
        causal flag; the additive form is built only if the eager path runs).
        ``position_bias``: a dense [1, H, Tq, Tk] tensor or a ``RelBias``; with
        ``attn_mask`` a layer that owns a table creates a ``RelBias``.
        Returns (out, position_bias, new_kv)."""
        B, Tq, _ = x.shape
        q = self._shape(self.q(x), B, Tq)
        if kv_input is None:  # self-attention
            k = self._shape(self.k(x), B, Tq)
            v = self._shape(self.v(x), B, Tq)
            if past_kv is not None:
                k = torch.cat([past_kv[0], k], dim=2)
                v = torch.cat([past_kv[1], v], dim=2)
            new_kv = (k, v)
        elif past_kv is not None:  # cached cross-attention
            k, v = past_kv
            new_kv = past_kv
        else:
            Tk = kv_input.shape[1]
            k = self._shape(self.k(kv_input), B, Tk)
            v = self._shape(self.v(kv_input), B, Tk)
            new_kv = (k, v)

        if position_bias is None and self.relative_attention_bias is not None:
            q_offset = k.shape[2] - Tq
            if attn_mask is not None:
                position_bias = RelBias(self, Tq, k.shape[2], x.device, q_offset=q_offset)
            else:
                position_bias = self.compute_bias(Tq, k.shape[2], x.device, q_offset=q_offset)

        # T5: NO 1/sqrt(d) scaling
        if self._takes_kernel(q, k, v, mask, position_bias, past_kv, attn_mask):
            vec, zero = position_bias.vec() if position_bias is not None else (None, 0)
            out = ops.seq2seq_attention(q, k, v, rel_bias=vec, bias_zero=zero,
                                        key_mask=attn_mask.uint8(), causal=attn_mask.causal,
                                        start_pos=0, scale=1.0)
            return self.o(out.transpose(1, 2).reshape(B, Tq, -1)), position_bias, new_kv

        scores = torch.matmul(q, k.transpose(-1, -2)).float()
        if mask is None and attn_mask is not None:
            mask = attn_mask.additive()
        dense = position_bias.dense() if isinstance(position_bias, RelBias) else position_bias
        if dense is not None:
            scores = scores + dense.float()
        if mask is not None:
            scores = scores + mask.float()
        probs = torch.softmax(scores, dim=-1).to(v.dtype)
        out = torch.matmul(probs, v).transpose(1, 2).reshape(B, Tq, -1)
        return self.o(out), position_bias, new_kv


class T5FFN(nn.Module):
    def __init__(self, cfg: Seq2SeqConfig):
        super().__init__()
        if cfg.is_gated:
            self.wi_0 = nn.Linear(cfg.d_model, cfg.d_ff, bias=False)
            self.wi_1 = nn.Linear(cfg.d_model, cfg.d_ff, bias=False)
        else:
            self.wi = nn.Linear(cfg.d_model, cfg.d_ff, bias=False)
        self.wo = nn.Linear(cfg.d_ff, cfg.d_model, bias=False)
        self.gated = cfg.is_gated

    def forward(self, x):
        if self.gated:
            h = F.gelu(self.wi_0(x), approximate="tanh") * self.wi_1(x)
        else:
            h = F.relu(self.wi(x))
        return self.wo(h)


class T5Block(nn.Module):
    def __init__(self, cfg: Seq2SeqConfig, is_decoder: bool, has_bias: bool):
        super().__init__()
        self.is_decoder = is_decoder
        self.self_norm = T5Norm(cfg.d_model, cfg.layer_norm_epsilon)
        self.self_attn = T5Attention(cfg, has_bias, bidirectional=not is_decoder)
        if is_decoder:
            self.cross_norm = T5Norm(cfg.d_model, cfg.layer_norm_epsilon)
            self.cross_attn = T5Attention(cfg, has_bias=False, bidirectional=True)
        self.ffn_norm = T5Norm(cfg.d_model, cfg.layer_norm_epsilon)
        self.ffn = T5FFN(cfg)

    def forward(self, x, enc_out=None, self_mask=None, cross_mask=None, position_bias=None,
                cross_bias=None, past_self_kv=None, past_cross_kv=None,
                ctx: Optional[AttnContext] = None):
        """Masks come either as additive tensors (``self_mask`` / ``cross_mask``)
        or as one ``AttnContext`` (``ctx``) that serves both attention paths."""
        h, position_bias, new_self_kv = self.self_attn(
            self.self_norm(x), mask=self_mask, position_bias=position_bias, past_kv=past_self_kv,
            attn_mask=ctx.self_attn if ctx is not None and self_mask is None else None)
        x = x + h
        new_cross_kv = None
        if self.is_decoder and enc_out is not None:
            h, _, new_cross_kv = self.cross_attn(
                self.cross_norm(x), kv_input=enc_out, mask=cross_mask, position_bias=cross_bias,
                past_kv=past_cross_kv,
                attn_mask=ctx.cross if ctx is not None and cross_mask is None else None)
            x = x + h
        x = x + self.ffn(self.ffn_norm(x))
        return x, position_bias, new_self_kv, new_cross_kv


class Seq2SeqDecodeState:
    """Everything ``Seq2SeqTransformer.decode_step`` reads besides the weights,
    preallocated once and reused by every generate call (and by the captured
    graph of ``generation.Seq2SeqDecodeEngine``, which bakes the addresses in):

    - ``self_k`` / ``self_v``: per-layer self-attention caches [B, H, S, D],
      appended in place at ``cache_idx`` (``S`` decoder positions);
    - ``cross_k`` / ``cross_v``: per-layer cross-attention K/V [B, H, Tcap, D];
    - ``key_mask``: uint8 [B, Tcap], zero beyond the current prompt, so a
      shorter prompt reuses the buffers (whatever lies behind the mask is
      skipped by the kernel, never read);
    - ``rel_bias`` [H, S] fp32 with ``bias_zero = S - 1``: the decoder's
      Toeplitz bias vector for one query at any position < S;
    - ``cache_idx``: int64 [1] on the device, the position of the next token.
    """

    def __init__(self, model: "Seq2SeqTransformer", batch: int, enc_capacity: int,
                 max_positions: int, device, dtype):
        cfg = model.config
        H, D = cfg.num_heads, cfg.d_kv
        n = len(model.decoder_blocks)
        self.batch, self.enc_capacity, self.max_positions = batch, enc_capacity, max_positions

        def buf(length):
            return [torch.zeros(batch, H, length, D, dtype=dtype, device=device) for _ in range(n)]

        self.self_k, self.self_v = buf(max_positions), buf(max_positions)
        self.cross_k, self.cross_v = buf(enc_capacity), buf(enc_capacity)
        self.key_mask = torch.zeros(batch, enc_capacity, dtype=torch.uint8, device=device)
        self.rel_bias = torch.zeros(H, max_positions, dtype=torch.float32, device=device)
        self.bias_zero = max_positions - 1
        self.cache_idx = torch.zeros(1, dtype=torch.long, device=device)

    @torch.no_grad()
    def begin(self, model: "Seq2SeqTransformer", enc_out: torch.Tensor,
              attention_mask: Optional[torch.Tensor] = None):
        """Start a generate call: everything below is written INTO the existing
        buffers.  The bias vector is recomputed from the table on every call —
        the table may have been trained since the last one — and so are the
        cross K/V, from this call's encoder output."""
        B, T, _ = enc_out.shape
        assert B == self.batch and T <= self.enc_capacity, (B, T)
        cfg = model.config
        H, D = cfg.num_heads, cfg.d_kv
        owner = model.decoder_blocks[0].self_attn
        vec, zero = ops.t5_rel_bias(
            owner.relative_attention_bias.weight, 1, 1, self.max_positions - 1, False,
            cfg.relative_attention_num_buckets, cfg.relative_attention_max_distance)
        assert zero == self.bias_zero and vec.shape == self.rel_bias.shape
        self.rel_bias.copy_(vec)
        for i, block in enumerate(model.decoder_blocks):
            ca = block.cross_attn
            self.cross_k[i][:, :, :T].copy_(ca.k(enc_out).view(B, T, H, D).transpose(1, 2))
            self.cross_v[i][:, :, :T].copy_(ca.v(enc_out).view(B, T, H, D).transpose(1, 2))
        self.key_mask.zero_()
        if attention_mask is None:
            self.key_mask[:, :T].fill_(1)
        else:
            self.key_mask[:, :T].copy_(attention_mask != 0)
        self.cache_idx.zero_()


@dataclass
class Seq2SeqOutput:
    logits: Optional[torch.Tensor] = None
    last_hidden_state: Optional[torch.Tensor] = None
    encoder_last_hidden_state: Optional[torch.Tensor] = None
    decoder_hidden_at_layer: Optional[torch.Tensor] = None


class Seq2SeqTransformer(nn.Module):
    """T5-family encoder-decoder LM."""

    def __init__(self, config: Seq2SeqConfig):
        super().__init__()
        self.config = config
        cfg = config
        self.shared = nn.Embedding(cfg.vocab_size, cfg.d_model)
        self.encoder_blocks = nn.ModuleList(
            T5Block(cfg, is_decoder=False, has_bias=(i == 0)) for i in range(cfg.num_layers)
        )
        self.encoder_final_norm = T5Norm(cfg.d_model, cfg.layer_norm_epsilon)
        self.decoder_blocks = nn.ModuleList(
            T5Block(cfg, is_decoder=True, has_bias=(i == 0)) for i in range(cfg.num_decoder_layers)
        )
        self.decoder_final_norm = T5Norm(cfg.d_model, cfg.layer_norm_epsilon)
        self.lm_head = nn.Linear(cfg.d_model, cfg.vocab_size, bias=False)
        if cfg.tie_word_embeddings:
            self.lm_head.weight = self.shared.weight
        self.apply(self._init_weights)

    def _init_weights(self, module):
        if isinstance(module, nn.Linear):
            module.weight.data.normal_(0.0, 0.02)
        elif isinstance(module, nn.Embedding):
            module.weight.data.normal_(0.0, 0.02)

    # --- encoder ------------------------------------------------------------

    def encode(self, input_ids, attention_mask=None):
        h = self.shared(input_ids)
        ctx = encoder_context(attention_mask)
        bias = None
        for block in self.encoder_blocks:
            h, bias, _, _ = block(h, position_bias=bias, ctx=ctx)
        return self.encoder_final_norm(h)

    # --- decoder ------------------------------------------------------------

    def decode(self, decoder_input_ids, enc_out, attention_mask=None,
               decoder_attention_mask=None, past=None, hidden_at_layer=None):
        """``past``: list of (self_kv, cross_kv) per layer for incremental
        decoding.  Returns (hidden, new_past, hidden_at)."""
        B, T = decoder_input_ids.shape
        h = self.shared(decoder_input_ids)
        past_len = past[0][0][0].shape[2] if past is not None and past[0][0] is not None else 0
        ctx = decoder_context(T, h.device, attention_mask, decoder_attention_mask,
                              past_len=past_len)

        bias = None
        new_past = []
        n = len(self.decoder_blocks)
        # int -> single stash (tensor); list -> dict keyed by requested values
        multi = isinstance(hidden_at_layer, (list, tuple))
        wanted = list(hidden_at_layer) if multi else (
            [hidden_at_layer] if hidden_at_layer is not None else [])
        stash_for = {}
        for w in wanted:
            stash_for.setdefault(w % n, []).append(w)
        hidden_at = {} if multi else None
        for i, block in enumerate(self.decoder_blocks):
            if i in stash_for:
                if multi:
                    for w in stash_for[i]:
                        hidden_at[w] = h
                else:
                    hidden_at = h
            p_self = past[i][0] if past is not None else None
            p_cross = past[i][1] if past is not None else None
            h, bias, self_kv, cross_kv = block(
                h, enc_out=enc_out, position_bias=bias, past_self_kv=p_self,
                past_cross_kv=p_cross, ctx=ctx)
            new_past.append((self_kv, cross_kv))
        return self.decoder_final_norm(h), new_past, hidden_at

    def new_decode_state(self, batch: int, enc_capacity: int, max_positions: int,
                         device=None, dtype=None) -> Seq2SeqDecodeState:
        w = self.shared.weight
        return Seq2SeqDecodeState(self, batch, enc_capacity, max_positions,
                                  device if device is not None else w.device,
                                  dtype if dtype is not None else w.dtype)

    def decode_step(self, cur_tok: torch.Tensor, state: Seq2SeqDecodeState) -> torch.Tensor:
        """One decoder token over a preallocated ``state`` (after
        ``state.begin``): ``cur_tok`` [B, 1] is the token at position
        ``state.cache_idx``.  Per block the two decode-attention ops
        (``ops.seq2seq_decode_attention`` appends this token's K/V to the self
        cache in place, ``ops.seq2seq_cross_decode_attention`` reads the
        prompt's K/V under the key mask): no ``torch.cat``, no dense bias, no
        additive mask, no host read — the step is the same work for every
        token, so it can be captured once.  Does NOT advance ``cache_idx``
        (every layer reads it; the caller bumps it after the step).
        Returns the final-normed hidden state [B, 1, d_model]."""
        B = cur_tok.shape[0]
        H, D = self.config.num_heads, self.config.d_kv
        h = self.shared(cur_tok.view(B, 1))
        for i, block in enumerate(self.decoder_blocks):
            sa = block.self_attn
            x = block.self_norm(h)
            a = ops.seq2seq_decode_attention(
                sa.q(x).view(B, H, D), sa.k(x).view(B, H, D), sa.v(x).view(B, H, D),
                state.self_k[i], state.self_v[i], state.cache_idx,
                rel_bias=state.rel_bias, bias_zero=state.bias_zero, scale=1.0)  # T5: unscaled
            h = h + sa.o(a.view(B, 1, H * D))
            ca = block.cross_attn
            q = ca.q(block.cross_norm(h)).view(B, H, 1, D)
            a = ops.seq2seq_cross_decode_attention(q, state.cross_k[i], state.cross_v[i],
                                                   key_mask=state.key_mask, scale=1.0)
            h = h + ca.o(a.view(B, 1, H * D))
            h = h + block.ffn(block.ffn_norm(h))
        return self.decoder_final_norm(h)

    def decoder_bias(self, q_len: int, device) -> RelBias:
        """The decoder's self-attention position bias for a full pass over
        ``q_len`` tokens, as the hydra and value branches need it to re-enter
        the stack above block 0 (which owns the table)."""
        return RelBias(self.decoder_blocks[0].self_attn, q_len, q_len, device)

    def project(self, hidden):
        if self.config.tie_word_embeddings:
            hidden = hidden * (self.config.d_model ** -0.5)
        return self.lm_head(hidden)

    # --- full forward ---------------------------------------------------------

    def forward(self, input_ids, attention_mask=None, decoder_input_ids=None,
                decoder_attention_mask=None, hidden_at_layer=None, return_logits=True,
                logits_slice=None):
        enc = self.encode(input_ids, attention_mask)
        dec, _, hidden_at = self.decode(decoder_input_ids, enc, attention_mask,
                                        decoder_attention_mask, hidden_at_layer=hidden_at_layer)
        logits = None
        if return_logits:
            ds = dec if logits_slice is None else dec[:, logits_slice[0] : logits_slice[1]]
            logits = self.project(ds)
        return Seq2SeqOutput(logits=logits, last_hidden_state=dec,
                             encoder_last_hidden_state=enc, decoder_hidden_at_layer=hidden_at)

    # --- generation -------------------------------------------------------------

    @torch.no_grad()
    def generate(self, input_ids, attention_mask=None, max_new_tokens: int = 32,
                 do_sample: bool = True, temperature: float = 1.0, top_k: int = 0,
                 top_p: float = 1.0, eos_token_id: Optional[int] = None,
                 pad_token_id: Optional[int] = None, seed: Optional[int] = None,
                 shaping_fn=None, **kwargs):
        """Returns decoder token ids [B, 1 + T_gen] starting with
        decoder_start_token_id (HF seq2seq convention).

        On the GPU in bf16 at a head dim in ``ops.SEQ2SEQ_DECODE_HEAD_DIMS`` the
        per-token step is ``decode_step`` inside ``generation.
        Seq2SeqDecodeEngine``: one hipGraph replay per token, or the same
        kernels in a plain loop under ``TRLX_AMD_NO_GRAPHS=1`` or with a
        ``shaping_fn`` not declared ``graph_safe_shaping=True``.  Everything
        else — CPU, other dtypes or head dims, ``TRLX_AMD_NO_S2S_DECODE=1`` —
        takes the eager ``past`` loop below."""
        cfg = self.config
        B = input_ids.shape[0]
        device = input_ids.device
        eos = eos_token_id if eos_token_id is not None else cfg.eos_token_id
        pad = pad_token_id if pad_token_id is not None else cfg.pad_token_id
        if (device.type == "cuda" and self.shared.weight.dtype == torch.bfloat16
                and ops.seq2seq_decode_enabled(cfg.d_kv) and B > 0 and max_new_tokens > 0):
            from .generation import seq2seq_generate

            return seq2seq_generate(
                self, input_ids, attention_mask, max_new_tokens=max_new_tokens,
                do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p,
                eos_token_id=eos, pad_token_id=pad, seed=seed, shaping_fn=shaping_fn,
                graph_safe_shaping=bool(kwargs.get("graph_safe_shaping", False)))
        if seed is None:
            seed = int(torch.randint(0, 2**31 - 1, (1,)).item())

        enc = self.encode(input_ids, attention_mask)
        cur = torch.full((B, 1), cfg.decoder_start_token_id, dtype=torch.long, device=device)
        out_tokens = [cur]
        finished = torch.zeros(B, dtype=torch.bool, device=device)
        past = None
        for step in range(max_new_tokens):
            h, past, _ = self.decode(cur, enc, attention_mask, past=past)
            logits = self.project(h[:, -1:, :])[:, 0].float()
            if shaping_fn is not None:
                logits = shaping_fn(logits, h[:, -1], cur[:, -1])
            if do_sample:
                tok = ops.sample_token(logits, temperature, top_k, top_p, seed=seed, offset=step)
            else:
                tok = logits.argmax(-1)
            tok = torch.where(finished, torch.full_like(tok, pad), tok)
            out_tokens.append(tok.unsqueeze(1))
            finished = finished | (tok == eos)
            cur = tok.unsqueeze(1)
            if bool(finished.all()):
                break
        return torch.cat(out_tokens, dim=1)

    def num_parameters(self):
        return sum(p.numel() for p in self.parameters())


# ---------------------------------------------------------------------------
# HF interop
# ---------------------------------------------------------------------------


def seq2seq_config_from_hf(hf: dict) -> Seq2SeqConfig:
    proj = hf.get("feed_forward_proj", "relu")
    return Seq2SeqConfig(
        vocab_size=hf["vocab_size"],
        d_model=hf["d_model"],
        d_kv=hf["d_kv"],
        num_heads=hf["num_heads"],
        d_ff=hf["d_ff"],
        num_layers=hf["num_layers"],
        num_decoder_layers=hf.get("num_decoder_layers", hf["num_layers"]),
        relative_attention_num_buckets=hf.get("relative_attention_num_buckets", 32),
        relative_attention_max_distance=hf.get("relative_attention_max_distance", 128),
        layer_norm_epsilon=hf.get("layer_norm_epsilon", 1e-6),
        feed_forward_proj=proj,
        tie_word_embeddings=hf.get("tie_word_embeddings", True),
        decoder_start_token_id=hf.get("decoder_start_token_id", 0),
        pad_token_id=hf.get("pad_token_id", 0),
        eos_token_id=hf.get("eos_token_id", 1),
    )


def seq2seq_config_to_hf(cfg: Seq2SeqConfig) -> dict:
    return {
        "model_type": "t5",
        "architectures": ["T5ForConditionalGeneration"],
        "vocab_size": cfg.vocab_size,
        "d_model": cfg.d_model,
        "d_kv": cfg.d_kv,
        "num_heads": cfg.num_heads,
        "d_ff": cfg.d_ff,
        "num_layers": cfg.num_layers,
        "num_decoder_layers": cfg.num_decoder_layers,
        "relative_attention_num_buckets": cfg.relative_attention_num_buckets,
        "relative_attention_max_distance": cfg.relative_attention_max_distance,
        "layer_norm_epsilon": cfg.layer_norm_epsilon,
        "feed_forward_proj": cfg.feed_forward_proj,
        "tie_word_embeddings": cfg.tie_word_embeddings,
        "decoder_start_token_id": cfg.decoder_start_token_id,
        "pad_token_id": cfg.pad_token_id,
        "eos_token_id": cfg.eos_token_id,
    }


def seq2seq_state_dict_from_hf(cfg: Seq2SeqConfig, hf: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    out = {"shared.weight": hf["shared.weight"]}

    def attn(dst, src):
        for a, b in (("q", "q"), ("k", "k"), ("v", "v"), ("o", "o")):
            out[f"{dst}.{a}.weight"] = hf[f"{src}.{a}.weight"]

    for i in range(cfg.num_layers):
        src = f"encoder.block.{i}.layer"
        dst = f"encoder_blocks.{i}"
        attn(f"{dst}.self_attn", f"{src}.0.SelfAttention")
        if i == 0:
            out[f"{dst}.self_attn.relative_attention_bias.weight"] = hf[
                f"{src}.0.SelfAttention.relative_attention_bias.weight"]
        out[f"{dst}.self_norm.weight"] = hf[f"{src}.0.layer_norm.weight"]
        if cfg.is_gated:
            out[f"{dst}.ffn.wi_0.weight"] = hf[f"{src}.1.DenseReluDense.wi_0.weight"]
            out[f"{dst}.ffn.wi_1.weight"] = hf[f"{src}.1.DenseReluDense.wi_1.weight"]
        else:
            out[f"{dst}.ffn.wi.weight"] = hf[f"{src}.1.DenseReluDense.wi.weight"]
        out[f"{dst}.ffn.wo.weight"] = hf[f"{src}.1.DenseReluDense.wo.weight"]
        out[f"{dst}.ffn_norm.weight"] = hf[f"{src}.1.layer_norm.weight"]
    for i in range(cfg.num_decoder_layers):
        src = f"decoder.block.{i}.layer"
        dst = f"decoder_blocks.{i}"
        attn(f"{dst}.self_attn", f"{src}.0.SelfAttention")
        if i == 0:
            out[f"{dst}.self_attn.relative_attention_bias.weight"] = hf[
                f"{src}.0.SelfAttention.relative_attention_bias.weight"]
        out[f"{dst}.self_norm.weight"] = hf[f"{src}.0.layer_norm.weight"]
        attn(f"{dst}.cross_attn", f"{src}.1.EncDecAttention")
        out[f"{dst}.cross_norm.weight"] = hf[f"{src}.1.layer_norm.weight"]
        if cfg.is_gated:
            out[f"{dst}.ffn.wi_0.weight"] = hf[f"{src}.2.DenseReluDense.wi_0.weight"]
            out[f"{dst}.ffn.wi_1.weight"] = hf[f"{src}.2.DenseReluDense.wi_1.weight"]
        else:
            out[f"{dst}.ffn.wi.weight"] = hf[f"{src}.2.DenseReluDense.wi.weight"]
        out[f"{dst}.ffn.wo.weight"] = hf[f"{src}.2.DenseReluDense.wo.weight"]
        out[f"{dst}.ffn_norm.weight"] = hf[f"{src}.2.layer_norm.weight"]
    out["encoder_final_norm.weight"] = hf["encoder.final_layer_norm.weight"]
    out["decoder_final_norm.weight"] = hf["decoder.final_layer_norm.weight"]
    if not cfg.tie_word_embeddings and "lm_head.weight" in hf:
        out["lm_head.weight"] = hf["lm_head.weight"]
    return out


def seq2seq_state_dict_to_hf(cfg: Seq2SeqConfig, sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    out = {
        "shared.weight": sd["shared.weight"],
        "encoder.embed_tokens.weight": sd["shared.weight"],
        "decoder.embed_tokens.weight": sd["shared.weight"],
        "lm_head.weight": sd.get("lm_head.weight", sd["shared.weight"]),
        "encoder.final_layer_norm.weight": sd["encoder_final_norm.weight"],
        "decoder.final_layer_norm.weight": sd["decoder_final_norm.weight"],
    }

    def attn(dst, src):
        for a in "qkvo":
            out[f"{dst}.{a}.weight"] = sd[f"{src}.{a}.weight"]

    for i in range(cfg.num_layers):
        dst = f"encoder.block.{i}.layer"
        src = f"encoder_blocks.{i}"
        attn(f"{dst}.0.SelfAttention", f"{src}.self_attn")
        if i == 0:
            out[f"{dst}.0.SelfAttention.relative_attention_bias.weight"] = sd[
                f"{src}.self_attn.relative_attention_bias.weight"]
        out[f"{dst}.0.layer_norm.weight"] = sd[f"{src}.self_norm.weight"]
        if cfg.is_gated:
            out[f"{dst}.1.DenseReluDense.wi_0.weight"] = sd[f"{src}.ffn.wi_0.weight"]
            out[f"{dst}.1.DenseReluDense.wi_1.weight"] = sd[f"{src}.ffn.wi_1.weight"]
        else:
            out[f"{dst}.1.DenseReluDense.wi.weight"] = sd[f"{src}.ffn.wi.weight"]
        out[f"{dst}.1.DenseReluDense.wo.weight"] = sd[f"{src}.ffn.wo.weight"]
        out[f"{dst}.1.layer_norm.weight"] = sd[f"{src}.ffn_norm.weight"]
    for i in range(cfg.num_decoder_layers):
        dst = f"decoder.block.{i}.layer"
        src = f"decoder_blocks.{i}"
        attn(f"{dst}.0.SelfAttention", f"{src}.self_attn")
        if i == 0:
            out[f"{dst}.0.SelfAttention.relative_attention_bias.weight"] = sd[
                f"{src}.self_attn.relative_attention_bias.weight"]
        out[f"{dst}.0.layer_norm.weight"] = sd[f"{src}.self_norm.weight"]
        attn(f"{dst}.1.EncDecAttention", f"{src}.cross_attn")
        out[f"{dst}.1.layer_norm.weight"] = sd[f"{src}.cross_norm.weight"]
        if cfg.is_gated:
            out[f"{dst}.2.DenseReluDense.wi_0.weight"] = sd[f"{src}.ffn.wi_0.weight"]
            out[f"{dst}.2.DenseReluDense.wi_1.weight"] = sd[f"{src}.ffn.wi_1.weight"]
        else:
            out[f"{dst}.2.DenseReluDense.wi.weight"] = sd[f"{src}.ffn.wi.weight"]
        out[f"{dst}.2.DenseReluDense.wo.weight"] = sd[f"{src}.ffn.wo.weight"]
        out[f"{dst}.2.layer_norm.weight"] = sd[f"{src}.ffn_norm.weight"]
    return out
