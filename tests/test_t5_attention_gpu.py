"""The seq2seq (T5) modes of the gfx950 flash kernels — non-causal, Toeplitz
relative-position bias, arbitrary key mask, Tq != Tk — against the fp32
reference (``reference.seq2seq_attention``, itself checked against the eager
T5 math in tests/test_t5_attention.py) on the same bf16 inputs.

Tolerances are the project's own for these kernels (test_alibi_gpu.py,
test_flash_backward.py): 3e-2 on outputs, 8e-2 on gradients; the modes add one
fp32 add and a predicate inside the same bf16-in / fp32-accumulate structure.
K and V rows at masked keys hold 1e4 and the bias tables are N(0, 2) per head,
and every case first shows on the reference alone that a bias shifted by one
position, or a mask ignored, moves the output by more than the tolerance — a
wrong index or a leaked key cannot hide under it."""

import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from trlx_amd import ops
    from trlx_amd.ops import reference

DEV = "cuda"
OUT_TOL = dict(atol=3e-2, rtol=3e-2)
GRAD_TOL = dict(atol=8e-2, rtol=8e-2)
B, H = 2, 4
POISON = 1e4


def _rand(*shape):
    return (torch.randn(*shape, device=DEV) * 0.5).bfloat16()


def _key_mask(kind, Tk):
    if kind == "none":
        return None
    m = torch.ones(B, Tk, dtype=torch.uint8, device=DEV)
    if kind == "right":
        m[0, Tk - 9:] = 0
        m[1, Tk // 2:] = 0
    elif kind == "holes":
        g = torch.Generator().manual_seed(7)
        m = (torch.rand(B, Tk, generator=g) > 0.4).to(torch.uint8).to(DEV)
        m[:, 0] = 1  # every causal row keeps a visible key
    elif kind == "left70":  # the whole first 64-key tile is masked
        m[0, :70] = 0
        m[1, :5] = 0
    return m


def _bias(Tq, Tk, bidirectional, q_offset=0):
    table = torch.randn(32, H, device=DEV) * 2.0  # N(0, 2), different per head
    return ops.t5_rel_bias(table, Tq, Tk, q_offset, bidirectional)


def _inputs(Tq, Tk, D, key_mask):
    q, k, v = _rand(B, H, Tq, D), _rand(B, H, Tk, D), _rand(B, H, Tk, D)
    if key_mask is not None:  # a leaked key is worth 1e4
        hidden = (key_mask == 0)[:, None, :, None].expand(B, H, Tk, D)
        k = torch.where(hidden, torch.full_like(k, POISON), k)
        v = torch.where(hidden, torch.full_like(v, POISON), v)
    return q, k, v


def _assert_inputs_matter(ref, q, k, v, vec, zero, key_mask, causal, start_pos=0):
    """On the reference alone: the bias index and the mask each move the
    output by more than the tolerance."""
    if vec is not None:
        shifted = reference.seq2seq_attention(q.float(), k.float(), v.float(),
                                              torch.roll(vec, 1, dims=1), zero, key_mask, causal,
                                              start_pos)
        moved = (shifted - ref).abs().max().item()
        assert moved > 3e-2, f"a bias shifted by one moves the reference by {moved:.3g}"
    if key_mask is not None:
        unmasked = reference.seq2seq_attention(q.float(), k.float(), v.float(), vec, zero or 0,
                                               None, causal, start_pos)
        moved = (unmasked - ref).abs().max().item()
        assert moved > 3e-2, f"ignoring the mask moves the reference by {moved:.3g}"


def _cases():
    out = []
    for Tq, Tk in [(40, 100), (64, 64), (70, 130), (130, 70)]:
        for causal in ([False, True] if Tq == Tk else [False]):
            masks = ["none", "right", "holes"] + (["left70"] if Tk == 130 else [])
            for mask in masks:
                for with_bias in (True, False):
                    out.append((Tq, Tk, causal, mask, with_bias))
    return out


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Tq,Tk,causal,mask,with_bias", _cases())
def test_forward_and_backward_vs_reference(Tq, Tk, causal, mask, with_bias, D):
    torch.manual_seed(0)
    key_mask = _key_mask(mask, Tk)
    q, k, v = _inputs(Tq, Tk, D, key_mask)
    vec, zero = _bias(Tq, Tk, not causal) if with_bias else (None, 0)
    dout = _rand(B, H, Tq, D)

    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    ref = reference.seq2seq_attention(qf, kf, vf, vec, zero, key_mask, causal)
    ref.backward(dout.float())
    ref = ref.detach()
    _assert_inputs_matter(ref, q, k, v, vec, zero, key_mask, causal)

    # forward-only kernel
    with torch.no_grad():
        out = ops.seq2seq_attention(q, k, v, vec, zero, key_mask, causal)
    assert out.dtype == torch.bfloat16 and out.shape == q.shape
    torch.testing.assert_close(out.float(), ref, **OUT_TOL)

    # forward (saves the logsumexp) + dKV / dQ kernels
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = ops.seq2seq_attention(qg, kg, vg, vec, zero, key_mask, causal)
    out.backward(dout)
    torch.testing.assert_close(out.float(), ref, **OUT_TOL)
    torch.testing.assert_close(vg.grad.float(), vf.grad, **GRAD_TOL)
    torch.testing.assert_close(kg.grad.float(), kf.grad, **GRAD_TOL)
    torch.testing.assert_close(qg.grad.float(), qf.grad, **GRAD_TOL)


@pytest.mark.parametrize("D", [64, 128])
def test_fully_masked_batch_row(D):
    """No visible key: zeros out, lse = +inf, nothing flows back — and the
    other batch row is unaffected."""
    torch.manual_seed(1)
    Tq, Tk = 70, 130
    key_mask = _key_mask("holes", Tk)
    key_mask[1] = 0
    q, k, v = _inputs(Tq, Tk, D, key_mask)
    vec, zero = _bias(Tq, Tk, True)
    dout = _rand(B, H, Tq, D)

    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    ref = reference.seq2seq_attention(qf, kf, vf, vec, zero, key_mask, False)
    ref.backward(dout.float())
    _assert_inputs_matter(ref.detach(), q, k, v, vec, zero, key_mask, False)

    ext = ops._require_ext("test")
    out, lse = ext.flash_prefill_lse(q, k, v, None, 0, 1.0, 0, True, None, vec, zero, key_mask,
                                     False)
    assert torch.isfinite(out).all()
    assert torch.count_nonzero(out[1]) == 0
    assert torch.isinf(lse[1]).all() and (lse[1] > 0).all() and torch.isfinite(lse[0]).all()
    torch.testing.assert_close(out.float(), ref.detach(), **OUT_TOL)

    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    ops.seq2seq_attention(qg, kg, vg, vec, zero, key_mask, False).backward(dout)
    for g in (qg.grad, kg.grad, vg.grad):
        assert torch.isfinite(g).all() and torch.count_nonzero(g[1]) == 0
    torch.testing.assert_close(vg.grad.float(), vf.grad, **GRAD_TOL)
    torch.testing.assert_close(kg.grad.float(), kf.grad, **GRAD_TOL)
    torch.testing.assert_close(qg.grad.float(), qf.grad, **GRAD_TOL)


@pytest.mark.parametrize("D", [64, 128])
def test_causal_chunk_with_start_pos(D):
    """Queries 64..129 as a chunk (start_pos=64) against all 130 keys equal the
    matching rows of the full causal pass: start_pos moves both the causal line
    and the bias index."""
    torch.manual_seed(2)
    T = 130
    key_mask = _key_mask("holes", T)
    q, k, v = _inputs(T, T, D, key_mask)
    vec, zero = _bias(T, T, False)
    ref = reference.seq2seq_attention(q.float(), k.float(), v.float(), vec, zero, key_mask, True)
    qc = q[:, :, 64:].contiguous()
    ref_c = reference.seq2seq_attention(qc.float(), k.float(), v.float(), vec, zero, key_mask,
                                        True, start_pos=64)
    torch.testing.assert_close(ref_c, ref[:, :, 64:], atol=1e-5, rtol=1e-5)
    _assert_inputs_matter(ref_c, qc, k, v, vec, zero, key_mask, True, start_pos=64)
    with torch.no_grad():
        full = ops.seq2seq_attention(q, k, v, vec, zero, key_mask, True)
        chunk = ops.seq2seq_attention(qc, k, v, vec, zero, key_mask, True, start_pos=64)
    torch.testing.assert_close(full.float(), ref, **OUT_TOL)
    torch.testing.assert_close(chunk.float(), full[:, :, 64:].float(), **OUT_TOL)
    torch.testing.assert_close(chunk.float(), ref_c, **OUT_TOL)


def test_host_checks():
    torch.manual_seed(3)
    D, Tq, Tk = 64, 40, 100
    ext = ops._require_ext("test")
    q, k, v = _rand(B, H, Tq, D), _rand(B, H, Tk, D), _rand(B, H, Tk, D)
    vec, zero = _bias(Tq, Tk, True)
    key_mask = _key_mask("right", Tk)
    slopes = torch.ones(H, device=DEV)
    key_starts = torch.zeros(B, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        ops.seq2seq_attention(q, k, v, vec, zero, key_mask)  # the valid call
        with pytest.raises(RuntimeError, match="does not cover"):  # too short for Tk
            ops.seq2seq_attention(q, k, v, vec[:, :-1].contiguous(), zero, key_mask)
        with pytest.raises(RuntimeError, match="does not cover"):  # too short for Tq
            ops.seq2seq_attention(q, k, v, vec, zero - 1, key_mask)
    with pytest.raises(RuntimeError, match="alibi_slopes"):
        ext.flash_prefill(q, k, v, None, 0, 1.0, 0, slopes, vec, zero, None, False)
    with pytest.raises(RuntimeError, match="key_starts"):
        ext.flash_prefill(q, k, v, key_starts, 0, 1.0, 0, None, None, 0, key_mask, False)
    with pytest.raises(RuntimeError, match="head dim"):
        ops.seq2seq_attention(_rand(B, H, Tq, 96), _rand(B, H, Tk, 96), _rand(B, H, Tk, 96))
    # causal training needs Tq == Tk: the op and the backward binding both say so
    with pytest.raises(RuntimeError, match="Tq == Tk"):
        ops.seq2seq_attention(q.clone().requires_grad_(True), k, v, causal=True)
    out, lse = ext.flash_prefill_lse(q, k, v, None, 0, 1.0, 0, True, None, None, 0, None, False)
    with pytest.raises(RuntimeError, match="Tk == T"):
        ext.flash_prefill_bwd(q, k, v, out, out, lse, None, 1.0, None, None, 0, None, True)
    # the same too-short bias in the backward
    with pytest.raises(RuntimeError, match="does not cover"):
        ext.flash_prefill_bwd(q, k, v, out, out, lse, None, 1.0, None,
                              vec[:, :-1].contiguous(), zero, None, False)


# --------------------------------------------------------------------------
# model level
# --------------------------------------------------------------------------


def _tiny_t5():
    from trlx_amd.models.nn.seq2seq import Seq2SeqConfig, Seq2SeqTransformer

    torch.manual_seed(4)
    cfg = Seq2SeqConfig(vocab_size=96, d_model=128, d_kv=64, num_heads=2, d_ff=256, num_layers=2)
    model = Seq2SeqTransformer(cfg)
    # the 0.02 init gives near-uniform attention and logits of a few 1e-2, under
    # the tolerance: unit embeddings (logits of order 1 through the tied head)
    # and sharper q/k (score std of a few units) make the comparison bite
    model.shared.weight.data.normal_(0.0, 1.0)
    for blocks in (model.encoder_blocks, model.decoder_blocks):
        blocks[0].self_attn.relative_attention_bias.weight.data.normal_(0.0, 1.0)
        for blk in blocks:
            blk.self_attn.q.weight.data.mul_(4.0)
            blk.self_attn.k.weight.data.mul_(4.0)
    return model, cfg


def _padded_batch(cfg):
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(2, cfg.vocab_size, (3, 37), generator=g).to(DEV)
    mask = torch.ones_like(ids)
    mask[0, :9] = 0   # left pad
    mask[1, 30:] = 0  # right pad
    dec = torch.randint(2, cfg.vocab_size, (3, 21), generator=g).to(DEV)
    dmask = torch.ones_like(dec)
    dmask[2, 15:] = 0
    return ids, mask, dec, dmask


def _kernels(monkeypatch, on):
    monkeypatch.setenv("TRLX_AMD_NO_FLASH_PREFILL", "0" if on else "1")
    monkeypatch.setenv("TRLX_AMD_NO_FLASH_TRAIN", "0" if on else "1")


def _record(monkeypatch):
    calls = []
    real = ops.seq2seq_attention

    def wrapped(q, k, v, rel_bias=None, bias_zero=0, key_mask=None, causal=False, **kw):
        calls.append((q.shape[2], k.shape[2], rel_bias is not None, causal,
                      torch.is_grad_enabled() and q.requires_grad))
        return real(q, k, v, rel_bias, bias_zero, key_mask, causal, **kw)

    monkeypatch.setattr(ops, "seq2seq_attention", wrapped)
    return calls


def test_model_logits_kernels_on_vs_off(monkeypatch):
    model, cfg = _tiny_t5()
    model = model.to(DEV).bfloat16().eval()
    ids, mask, dec, dmask = _padded_batch(cfg)
    calls = _record(monkeypatch)
    with torch.no_grad():
        _kernels(monkeypatch, False)
        eager = model(ids, mask, dec, dmask).logits.float()
        assert calls == []
        _kernels(monkeypatch, True)
        flash = model(ids, mask, dec, dmask).logits.float()
    assert len(calls) == 2 + 2 * 2
    assert eager.abs().max() > 10 * 3e-2  # the comparison is not about zeros
    torch.testing.assert_close(flash, eager, **OUT_TOL)


def _hydra_loss(model, batch):
    from trlx_amd.utils.modeling import logprobs_of_labels

    ids, mask, dec, dmask = batch
    out = model(ids, mask, dec, dmask, return_ref_logits=True)
    lp = logprobs_of_labels(out.logits[:, :-1], dec[:, 1:])
    ref_lp = logprobs_of_labels(out.ref_logits[:, :-1], dec[:, 1:])
    w = dmask[:, 1:].float()
    return (((lp - ref_lp.detach()) ** 2 + lp) * w).sum() / w.sum() + (out.values ** 2).mean()


def _rel_err(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def test_hydra_train_step_takes_the_kernels(monkeypatch):
    from trlx_amd.models.modeling_seq2seq import AutoModelForSeq2SeqLMWithHydraValueHead
    from trlx_amd.utils.modeling import freeze_bottom_seq2seq_layers

    base, cfg = _tiny_t5()
    model = AutoModelForSeq2SeqLMWithHydraValueHead(base, num_layers_unfrozen=1)
    freeze_bottom_seq2seq_layers(model.base_model, 1)
    model = model.to(DEV)
    model.cast_compute(torch.bfloat16)
    batch = _padded_batch(cfg)
    calls = _record(monkeypatch)

    grads = {}
    for on in (False, True):
        _kernels(monkeypatch, on)
        model.zero_grad(set_to_none=True)
        _hydra_loss(model, batch).backward()
        grads[on] = {n: p.grad.clone() for n, p in model.named_parameters()
                     if p.grad is not None}
        if not on:
            assert calls == []
    # encoder (2) + decoder self/cross (4) + frozen branch self/cross (2)
    assert len(calls) == 8
    Te, Td = 37, 21
    assert calls[:2] == [(Te, Te, True, False, False)] * 2
    assert [c[:4] for c in calls[2:6]] == [(Td, Td, True, True), (Td, Te, False, False)] * 2
    assert calls[4][4] and calls[5][4] and not calls[2][4]  # only the top block trains
    assert [c for c in calls[6:]] == [(Td, Td, True, True, False), (Td, Te, False, False, False)]

    top = [n for n in grads[True] if "decoder_blocks.1." in n]
    assert len(top) >= 8 and set(grads[True]) == set(grads[False])
    for n in top:
        torch.testing.assert_close(grads[True][n].float(), grads[False][n].float(), **GRAD_TOL)
        # scale-free form of the same 8e-2: parameter gradients can be far below
        # the absolute tolerance, where assert_close alone would say nothing
        err = _rel_err(grads[True][n], grads[False][n])
        print(f"{n}: relative gradient error {err:.3g}")
        assert err < 8e-2, n


def test_unfrozen_bias_table_still_gets_its_gradient(monkeypatch):
    """Everything trainable: the self-attention that owns a trainable table
    stays eager by design, cross-attention takes the kernels, and the table's
    gradient is the eager one."""
    model, cfg = _tiny_t5()
    model = model.to(DEV).bfloat16()
    ids, mask, dec, dmask = _padded_batch(cfg)
    calls = _record(monkeypatch)
    grads = {}
    for on in (False, True):
        _kernels(monkeypatch, on)
        model.zero_grad(set_to_none=True)
        logits = model(ids, mask, dec, dmask).logits.float()
        (logits.log_softmax(-1)[..., 3] * dmask).sum().backward()
        grads[on] = [copy.deepcopy(b[0].self_attn.relative_attention_bias.weight.grad)
                     for b in (model.encoder_blocks, model.decoder_blocks)]
    assert [c[:4] for c in calls] == [(21, 37, False, False)] * 2  # cross-attention only
    for got, want in zip(grads[True], grads[False]):
        assert want is not None and want.abs().max() > 0
        torch.testing.assert_close(got.float(), want.float(), **GRAD_TOL)
        err = _rel_err(got, want)  # scale-free 8e-2, as in the hydra test
        print(f"bias table: relative gradient error {err:.3g}, max |grad| {want.abs().max():.3g}")
        assert err < 8e-2
