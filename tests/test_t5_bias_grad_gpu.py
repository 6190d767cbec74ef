"""The bias-gradient kernel (csrc/flash_bwd_dbias.hip) behind
``ops.seq2seq_attention(..., bias_grad=True)`` against fp32 autograd through
``reference.seq2seq_attention`` on the same bf16 values.

The error is ``max|got - ref| / max|ref|`` per head, worst head.  TOL is twice
the worse of two measured worst cases over exactly these cases, capped at the
project's 8e-2 for these kernels: the eager bf16 T5Attention math it replaces
(dP rounded to bf16) against an fp64 reference, MEASURED_EAGER, and this kernel
(bf16 O inside Drow) against the fp32 reference, MEASURED_KERNEL
(profiles/t5_bias_grad_notes.md).  Every case first shows on the reference
alone that a gradient off by one index would miss TOL."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from test_t5_attention_gpu import _kernels, _padded_batch, _rel_err, _tiny_t5
    from trlx_amd import ops
    from trlx_amd.ops import reference

DEV = "cuda"
B, H = 3, 4  # three batch rows: uneven batch chunks
MEASURED_EAGER = 1.11e-2   # worst case: D=128, 130x130 causal, no mask
MEASURED_KERNEL = 1.29e-2  # worst case: D=64, 64x64 causal, holes
TOL = min(2 * max(MEASURED_EAGER, MEASURED_KERNEL), 8e-2)
SHAPES = [(40, 100, False), (64, 64, True), (70, 130, False), (130, 70, False), (130, 130, True)]
CASES = [(*s, m) for s in SHAPES for m in ("none", "holes")] + [(70, 130, False, "row_masked")]


def _rand(*shape):
    return (torch.randn(*shape, device=DEV) * 0.5).bfloat16()


def make_case(Tq, Tk, causal, mask, D):
    """Inputs as in test_t5_attention_gpu.py: 0.5 N(0,1) bf16, a N(0,2) table,
    K and V rows at masked keys poisoned with 1e4."""
    torch.manual_seed(0)
    key_mask = None
    if mask != "none":
        g = torch.Generator().manual_seed(7)
        key_mask = (torch.rand(B, Tk, generator=g) > 0.4).to(torch.uint8).to(DEV)
        key_mask[:, 0] = 1  # every causal row keeps a visible key
        if mask == "row_masked":
            key_mask[1] = 0
    q, k, v, dout = _rand(B, H, Tq, D), _rand(B, H, Tk, D), _rand(B, H, Tk, D), _rand(B, H, Tq, D)
    if key_mask is not None:
        hidden = (key_mask == 0)[:, None, :, None].expand(B, H, Tk, D)
        k = torch.where(hidden, torch.full_like(k, 1e4), k)
        v = torch.where(hidden, torch.full_like(v, 1e4), v)
    vec, zero = ops.t5_rel_bias(torch.randn(32, H, device=DEV) * 2.0, Tq, Tk, 0, not causal)
    return q, k, v, dout, vec, zero, key_mask


def head_err(got, ref):
    return ((got - ref).abs().amax(1) / ref.abs().amax(1)).max().item()


def kernel_grads(q, k, v, dout, vec, zero, key_mask, causal, bias_grad=True):
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    bias = vec.clone().requires_grad_(bias_grad)
    ops.seq2seq_attention(qg, kg, vg, bias, zero, key_mask, causal,
                          bias_grad=bias_grad).backward(dout)
    return bias.grad, qg.grad, kg.grad, vg.grad


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Tq,Tk,causal,mask", CASES)
def test_bias_gradient_vs_reference(Tq, Tk, causal, mask, D):
    q, k, v, dout, vec, zero, key_mask = make_case(Tq, Tk, causal, mask, D)
    want = vec.clone().requires_grad_()
    reference.seq2seq_attention(q.float(), k.float(), v.float(), want, zero, key_mask,
                                causal).backward(dout.float())
    ref = want.grad
    moved = head_err(torch.roll(ref, 1, dims=1), ref)
    assert moved > TOL, f"a gradient off by one index moves the reference by {moved:.3g}"

    got, dq, dk, dv = kernel_grads(q, k, v, dout, vec, zero, key_mask, causal)
    assert got.shape == vec.shape and got.dtype == torch.float32 and torch.isfinite(got).all()
    err = head_err(got, ref)
    print(f"bias gradient error {err:.3g} (max |ref| {ref.abs().max():.3g})")
    assert err < TOL

    # the third kernel changes nothing about dq / dk / dv, and repeats bit for bit
    again, *_ = kernel_grads(q, k, v, dout, vec, zero, key_mask, causal)
    assert torch.equal(again, got)
    _, dq0, dk0, dv0 = kernel_grads(q, k, v, dout, vec, zero, key_mask, causal, bias_grad=False)
    assert torch.equal(dq, dq0) and torch.equal(dk, dk0) and torch.equal(dv, dv0)


def test_unfrozen_t5_takes_the_kernels_when_switched_on(monkeypatch):
    """Everything trainable and TRLX_AMD_FLASH_T5_BIAS_GRAD=1: encoder and
    decoder self-attention reach the op with bias_grad=True, and both tables'
    gradients are the eager run's."""
    model, cfg = _tiny_t5()
    model = model.to(DEV).bfloat16()
    ids, mask, dec, dmask = _padded_batch(cfg)
    calls = []
    real = ops.seq2seq_attention

    def wrapped(q, k, v, rel_bias=None, *args, **kw):
        calls.append((rel_bias is not None, kw.get("bias_grad", False)))
        return real(q, k, v, rel_bias, *args, **kw)

    monkeypatch.setattr(ops, "seq2seq_attention", wrapped)
    monkeypatch.setenv("TRLX_AMD_FLASH_T5_BIAS_GRAD", "1")
    grads = {}
    for on in (False, True):
        _kernels(monkeypatch, on)
        model.zero_grad(set_to_none=True)
        logits = model(ids, mask, dec, dmask).logits.float()
        (logits.log_softmax(-1)[..., 3] * dmask).sum().backward()
        grads[on] = [b[0].self_attn.relative_attention_bias.weight.grad.clone()
                     for b in (model.encoder_blocks, model.decoder_blocks)]
        if not on:
            assert calls == []
    # two encoder layers, then decoder self / cross twice
    assert calls == [(True, True)] * 2 + [(True, True), (False, False)] * 2
    for got, want in zip(grads[True], grads[False]):
        assert want.abs().max() > 0
        err = _rel_err(got, want)
        print(f"bias table: relative gradient error {err:.3g}")
        assert err < 8e-2
