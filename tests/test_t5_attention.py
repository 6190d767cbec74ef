"""T5 attention through the seq2seq modes of the flash kernels, CPU side: the
Toeplitz form of the relative-position bias, the fp32 reference every GPU
numerics test compares against, the dispatch gate and the model routing.

The reference is checked against the eager ``T5Attention`` math itself
(additive ``finfo.min`` masks + dense bias), so tests/test_t5_attention_gpu.py
measures the kernels against what the model computed before them."""

import pytest
import torch

from trlx_amd import ops
from trlx_amd.models.nn import seq2seq
from trlx_amd.models.nn.seq2seq import (
    AttnMask,
    Seq2SeqConfig,
    T5Attention,
    decoder_context,
    encoder_context,
)
from trlx_amd.ops import reference

SHAPES = [(40, 100, 0), (70, 130, 0), (130, 70, 0), (6, 70, 64), (1, 300, 299)]


def _attn(bidirectional, d_kv=16, heads=4, has_bias=True):
    torch.manual_seed(0)
    cfg = Seq2SeqConfig(vocab_size=32, d_model=32, d_kv=d_kv, num_heads=heads, d_ff=64,
                        num_layers=1)
    attn = T5Attention(cfg, has_bias=has_bias, bidirectional=bidirectional)
    if has_bias:
        attn.relative_attention_bias.weight.data.normal_(0.0, 2.0)
    return attn, cfg


# --------------------------------------------------------------------------
# t5_rel_bias
# --------------------------------------------------------------------------


@pytest.mark.parametrize("bidirectional", [True, False])
@pytest.mark.parametrize("Tq,Tk,q_offset", SHAPES)
def test_rel_bias_gathers_to_compute_bias_exactly(bidirectional, Tq, Tk, q_offset):
    attn, cfg = _attn(bidirectional)
    dense = attn.compute_bias(Tq, Tk, "cpu", q_offset=q_offset)  # [1, H, Tq, Tk]
    vec, zero = ops.t5_rel_bias(attn.relative_attention_bias.weight, Tq, Tk, q_offset,
                                bidirectional, cfg.relative_attention_num_buckets,
                                cfg.relative_attention_max_distance)
    L = q_offset + Tq - 1 + Tk
    assert vec.shape == (cfg.num_heads, L) and vec.dtype == torch.float32 and vec.is_contiguous()
    assert zero == q_offset + Tq - 1
    # the host checks of the kernels hold for exactly this (vec, zero)
    assert zero - (q_offset + Tq - 1) >= 0 and zero + Tk - 1 < L
    gathered = reference.gather_rel_bias(vec, zero, Tq, Tk, start_pos=q_offset)
    assert torch.equal(gathered, dense[0])


def test_rel_bias_gradient_reaches_the_table():
    attn, cfg = _attn(True)
    table = attn.relative_attention_bias.weight
    vec, zero = ops.t5_rel_bias(table, 5, 9, 0, True, cfg.relative_attention_num_buckets,
                                cfg.relative_attention_max_distance)
    assert vec.requires_grad
    w = torch.randn_like(vec)
    (vec * w).sum().backward()
    # d sum(vec * w) / d table[b, h] = sum of w[h, l] over the positions l in bucket b
    rel = torch.arange(vec.shape[1]) - zero
    buckets = reference.relative_position_bucket(rel, True, cfg.relative_attention_num_buckets,
                                                 cfg.relative_attention_max_distance)
    expect = torch.zeros_like(table).index_add_(0, buckets, w.t().contiguous())
    torch.testing.assert_close(table.grad, expect, atol=1e-6, rtol=1e-6)
    assert table.grad.abs().sum() > 0


# --------------------------------------------------------------------------
# reference.seq2seq_attention == the eager T5Attention math
# --------------------------------------------------------------------------


def _masks(B, Tk):
    """left-padded, right-padded and holed key masks, each row with a visible key"""
    left = torch.ones(B, Tk, dtype=torch.long)
    left[0, : Tk // 2] = 0
    left[1, :3] = 0
    right = torch.ones(B, Tk, dtype=torch.long)
    right[0, Tk // 3:] = 0
    right[1, -1:] = 0
    g = torch.Generator().manual_seed(3)
    holes = (torch.rand(B, Tk, generator=g) > 0.4).long()
    holes[:, 0] = 1  # key 0 visible: under causal masking every query row keeps a key
    return {"none": None, "left": left, "right": right, "holes": holes}


def _eager(q, k, v, dense_bias, key_mask, causal):
    """The eager T5Attention sequence, verbatim: additive finfo.min masks."""
    Tq, Tk = q.shape[2], k.shape[2]
    scores = torch.matmul(q, k.transpose(-1, -2)).float()
    if dense_bias is not None:
        scores = scores + dense_bias.float()
    mask = AttnMask(key_mask, causal=causal, q_len=Tq, past_len=Tk - Tq, device="cpu").additive()
    if mask is not None:
        scores = scores + mask.float()
    return torch.matmul(torch.softmax(scores, dim=-1), v)


@pytest.mark.parametrize("mask_kind", ["none", "left", "right", "holes"])
@pytest.mark.parametrize("causal,Tq,Tk", [(False, 9, 21), (False, 21, 9), (True, 17, 17)])
@pytest.mark.parametrize("with_bias", [True, False])
def test_reference_matches_eager_math(mask_kind, causal, Tq, Tk, with_bias):
    torch.manual_seed(1)
    B, H, D = 2, 4, 16
    q, k, v = torch.randn(B, H, Tq, D), torch.randn(B, H, Tk, D), torch.randn(B, H, Tk, D)
    key_mask = _masks(B, Tk)[mask_kind]
    if causal and key_mask is not None:
        key_mask[:, 0] = 1  # every causal row keeps a visible key
    attn, cfg = _attn(not causal)
    vec = zero = dense = None
    if with_bias:
        dense = attn.compute_bias(Tq, Tk, "cpu").detach()
        vec, zero = ops.t5_rel_bias(attn.relative_attention_bias.weight.detach(), Tq, Tk, 0,
                                    not causal, cfg.relative_attention_num_buckets,
                                    cfg.relative_attention_max_distance)
    ref = reference.seq2seq_attention(q, k, v, vec, zero or 0, key_mask, causal)
    torch.testing.assert_close(ref, _eager(q, k, v, dense, key_mask, causal),
                               atol=1e-5, rtol=1e-5)
    # the public op on CPU is the same reference
    torch.testing.assert_close(ops.seq2seq_attention(q, k, v, vec, zero or 0, key_mask, causal),
                               ref)


def test_reference_rows_without_a_visible_key_are_zero():
    torch.manual_seed(2)
    B, H, Tq, Tk, D = 2, 2, 5, 7, 16
    q, k, v = torch.randn(B, H, Tq, D), torch.randn(B, H, Tk, D), torch.randn(B, H, Tk, D)
    key_mask = torch.ones(B, Tk, dtype=torch.long)
    key_mask[1] = 0
    out = reference.seq2seq_attention(q, k, v, key_mask=key_mask)
    assert torch.isfinite(out).all()
    assert torch.count_nonzero(out[1]) == 0 and torch.count_nonzero(out[0]) > 0
    # causal: rows before the first visible key have nothing to see
    key_mask = torch.ones(B, Tq, dtype=torch.long)
    key_mask[:, :2] = 0
    out = reference.seq2seq_attention(q, k[:, :, :Tq], v[:, :, :Tq], key_mask=key_mask,
                                      causal=True)
    assert torch.count_nonzero(out[:, :, :2]) == 0 and torch.count_nonzero(out[:, :, 2]) > 0


def test_start_pos_shifts_bias_and_causal_line():
    torch.manual_seed(4)
    B, H, T, D = 1, 2, 12, 16
    q, k, v = torch.randn(B, H, T, D), torch.randn(B, H, T, D), torch.randn(B, H, T, D)
    attn, cfg = _attn(False, heads=H)
    vec, zero = ops.t5_rel_bias(attn.relative_attention_bias.weight.detach(), T, T, 0, False)
    full = reference.seq2seq_attention(q, k, v, vec, zero, None, True)
    chunk = reference.seq2seq_attention(q[:, :, 8:], k, v, vec, zero, None, True, start_pos=8)
    torch.testing.assert_close(chunk, full[:, :, 8:])


def test_bias_that_requires_grad_is_rejected_under_grad_mode():
    q = k = v = torch.randn(1, 2, 4, 16)
    vec = torch.zeros(2, 7, requires_grad=True)
    with pytest.raises(RuntimeError, match="rel_bias"):
        ops.seq2seq_attention(q, k, v, vec, 3)
    with torch.no_grad():
        ops.seq2seq_attention(q, k, v, vec, 3)


# --------------------------------------------------------------------------
# gate
# --------------------------------------------------------------------------


def test_seq2seq_flash_gate(monkeypatch):
    monkeypatch.delenv("TRLX_AMD_NO_FLASH_PREFILL", raising=False)
    monkeypatch.delenv("TRLX_AMD_NO_FLASH_TRAIN", raising=False)
    for d in (64, 128):  # unset: the measured default sets decide
        assert ops.seq2seq_flash_enabled(d, False) == (d in ops.SEQ2SEQ_FLASH_PREFILL_DEFAULT_DIMS)
        assert ops.seq2seq_flash_enabled(d, True) == (d in ops.SEQ2SEQ_FLASH_TRAIN_DEFAULT_DIMS)
    assert set(ops.SEQ2SEQ_FLASH_TRAIN_DEFAULT_DIMS) <= set(ops.SEQ2SEQ_FLASH_HEAD_DIMS)
    assert set(ops.SEQ2SEQ_FLASH_PREFILL_DEFAULT_DIMS) <= set(ops.SEQ2SEQ_FLASH_HEAD_DIMS)
    # 0: on for every instantiated head dim and no other
    monkeypatch.setenv("TRLX_AMD_NO_FLASH_PREFILL", "0")
    monkeypatch.setenv("TRLX_AMD_NO_FLASH_TRAIN", "0")
    assert all(ops.seq2seq_flash_enabled(d, t) for d in (64, 128) for t in (False, True))
    assert not any(ops.seq2seq_flash_enabled(d, t) for d in (16, 96, 256) for t in (False, True))
    # NO_FLASH_TRAIN=1 stops training only
    monkeypatch.setenv("TRLX_AMD_NO_FLASH_TRAIN", "1")
    assert all(ops.seq2seq_flash_enabled(d, False) for d in (64, 128))
    assert not any(ops.seq2seq_flash_enabled(d, True) for d in (64, 128))
    # NO_FLASH_PREFILL=1 stops both
    monkeypatch.setenv("TRLX_AMD_NO_FLASH_TRAIN", "0")
    monkeypatch.setenv("TRLX_AMD_NO_FLASH_PREFILL", "1")
    assert not any(ops.seq2seq_flash_enabled(d, t) for d in (64, 128) for t in (False, True))
    # prefill unset + train 0: training on, forward follows its default set
    monkeypatch.delenv("TRLX_AMD_NO_FLASH_PREFILL")
    assert all(ops.seq2seq_flash_enabled(d, True) for d in (64, 128))


# --------------------------------------------------------------------------
# routing
# --------------------------------------------------------------------------


@pytest.fixture
def recorder(monkeypatch):
    """The kernel path with its device test waved through and the op replaced
    by a recorder that computes the fp32 reference."""
    calls = []

    def fake(q, k, v, rel_bias=None, bias_zero=0, key_mask=None, causal=False, start_pos=0,
             scale=1.0):
        calls.append(dict(rel_bias=rel_bias, bias_zero=bias_zero, key_mask=key_mask,
                          causal=causal, Tq=q.shape[2], Tk=k.shape[2]))
        return reference.seq2seq_attention(q, k, v, rel_bias, bias_zero, key_mask, causal,
                                           start_pos, scale)

    monkeypatch.setattr(seq2seq, "_on_gpu_bf16", lambda t: True)
    monkeypatch.setattr(ops, "seq2seq_attention", fake)
    monkeypatch.setenv("TRLX_AMD_NO_FLASH_PREFILL", "0")
    monkeypatch.setenv("TRLX_AMD_NO_FLASH_TRAIN", "0")
    return calls


def test_attention_routing(recorder):
    attn, cfg = _attn(True, d_kv=64, heads=2)
    x = torch.randn(2, 11, cfg.d_model)
    key_mask = torch.ones(2, 11, dtype=torch.long)
    key_mask[0, 7:] = 0
    ctx = encoder_context(key_mask)

    # a table that requires grad, under grad mode: eager
    eager_out, bias, _ = attn(x, attn_mask=ctx.self_attn)
    assert recorder == [] and isinstance(bias, seq2seq.RelBias)

    # the same under no_grad: kernel, with the Toeplitz vector and the raw mask
    with torch.no_grad():
        out, _, _ = attn(x, attn_mask=ctx.self_attn)
    assert len(recorder) == 1
    call = recorder[0]
    assert call["rel_bias"].shape == (2, 21) and call["bias_zero"] == 10
    assert call["key_mask"].dtype == torch.uint8 and call["causal"] is False
    assert torch.equal(call["key_mask"], key_mask.to(torch.uint8))
    torch.testing.assert_close(out, eager_out, atol=1e-5, rtol=1e-5)

    # frozen table under grad mode: kernel
    attn.relative_attention_bias.weight.requires_grad_(False)
    out, _, _ = attn(x, attn_mask=ctx.self_attn)
    assert len(recorder) == 2
    torch.testing.assert_close(out, eager_out, atol=1e-5, rtol=1e-5)

    # legacy keyword arguments (additive mask / dense bias) never take it
    attn(x, mask=ctx.self_attn.additive())
    attn(x, attn_mask=ctx.self_attn, position_bias=attn.compute_bias(11, 11, "cpu"))
    assert len(recorder) == 2

    # the per-token step (past_kv) stays eager
    with torch.no_grad():
        _, _, kv = attn(x, attn_mask=ctx.self_attn)
        assert len(recorder) == 3
        step_ctx = decoder_context(1, "cpu", past_len=11)
        attn(x[:, :1], past_kv=kv, attn_mask=step_ctx.self_attn)
    assert len(recorder) == 3

    # head dims outside the instantiated set stay eager
    small, cfg16 = _attn(True, d_kv=16)
    with torch.no_grad():
        small(torch.randn(1, 5, cfg16.d_model), attn_mask=AttnMask(None))
    assert len(recorder) == 3


def test_model_routing_matches_eager(recorder, monkeypatch):
    """Whole model: encoder, decoder self- and cross-attention all route to
    the op (no_grad), and the logits equal the eager path's."""
    from trlx_amd.models.nn.seq2seq import Seq2SeqTransformer

    torch.manual_seed(5)
    cfg = Seq2SeqConfig(vocab_size=50, d_model=32, d_kv=64, num_heads=2, d_ff=64, num_layers=2)
    model = Seq2SeqTransformer(cfg).eval()
    ids = torch.randint(2, 50, (2, 9))
    mask = torch.ones_like(ids)
    mask[0, :3] = 0
    dec = torch.randint(2, 50, (2, 6))
    dmask = torch.ones_like(dec)
    dmask[1, 4:] = 0
    with torch.no_grad():
        got = model(ids, mask, dec, dmask).logits
    assert len(recorder) == 2 + 2 * 2  # encoder layers + (self, cross) per decoder layer
    assert [c["causal"] for c in recorder] == [False, False, True, False, True, False]
    assert recorder[3]["Tq"] == 6 and recorder[3]["Tk"] == 9 and recorder[3]["rel_bias"] is None
    # the int64 masks are converted for the kernels once per pass, not per call
    assert recorder[0]["key_mask"] is recorder[1]["key_mask"]
    assert recorder[2]["key_mask"] is recorder[4]["key_mask"]
    assert recorder[3]["key_mask"] is recorder[5]["key_mask"]
    assert all(c["key_mask"].dtype == torch.uint8 for c in recorder)
    monkeypatch.setenv("TRLX_AMD_NO_FLASH_PREFILL", "1")
    with torch.no_grad():
        want = model(ids, mask, dec, dmask).logits
    assert len(recorder) == 6
    torch.testing.assert_close(got, want, atol=1e-4, rtol=1e-4)
