"""ALiBi (Bloom) through the gfx950 attention kernels: flash prefill, flash
forward+backward, flash-decode (GQA) and the fused MHA decode step take a
per-query-head slope vector; a tiny Bloom generates through the hipGraph
engine and trains/forwards through the flash kernels.

Tolerances are the project's own for the same kernels without the bias
(test_flash_prefill.py, test_flash_backward.py, test_ops.py): the bias is one
fp32 fma per score element inside the same bf16-in / fp32-accumulate structure.
Every kernel test first checks, on the fp32 reference alone, that the bias
moves the result by at least 10x the tolerance, so a kernel that ignored the
argument could not pass."""

import copy
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from trlx_amd import ops
    from trlx_amd.models.nn.transformer import alibi_slopes
    from trlx_amd.ops import reference

DEV = "cuda"


def _rand(*shape):
    return (torch.randn(*shape, device=DEV) * 0.5).bfloat16()


def _assert_bias_matters(ref_with, ref_without, tol):
    moved = (ref_with.float() - ref_without.float()).abs().max().item()
    assert moved >= 10 * tol, f"bias moves the reference by {moved:.3g} < 10 x {tol}"


# --------------------------------------------------------------------------
# flash prefill (forward only)
# --------------------------------------------------------------------------


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", [33, 64, 200])  # partial tile, exact tile, multi-tile + tail
def test_flash_prefill_alibi_vs_reference(D, T):
    torch.manual_seed(0)
    B, Hq = 3, 4
    q, k, v = _rand(B, Hq, T, D), _rand(B, Hq, T, D), _rand(B, Hq, T, D)
    key_starts = torch.tensor([0, 3, 7], device=DEV, dtype=torch.int32)
    slopes = alibi_slopes(Hq).to(DEV)
    scale = 1.0 / D ** 0.5

    ref = reference.flash_prefill(q.float(), k.float(), v.float(), key_starts, 0, scale,
                                  alibi_slopes=slopes)
    plain = reference.flash_prefill(q.float(), k.float(), v.float(), key_starts, 0, scale)
    _assert_bias_matters(ref, plain, 3e-2)

    out = ops.flash_prefill(q, k, v, key_starts, 0, scale, alibi_slopes=slopes)
    torch.testing.assert_close(out.float(), ref, atol=3e-2, rtol=3e-2)


def test_flash_prefill_alibi_gqa_cache_stride_and_chunk():
    """GQA (slopes per QUERY head) reading a cache with allocated stride
    Sk > tk, then a start_pos > 0 chunk (queries 64..95) against the same
    96 valid keys."""
    torch.manual_seed(1)
    B, Hq, Hkv, D, Sk, tk = 2, 8, 2, 64, 160, 96
    q = _rand(B, Hq, tk, D)
    kc = torch.zeros(B, Hkv, Sk, D, device=DEV).bfloat16()
    vc = torch.zeros(B, Hkv, Sk, D, device=DEV).bfloat16()
    kc[:, :, :tk] = _rand(B, Hkv, tk, D)
    vc[:, :, :tk] = _rand(B, Hkv, tk, D)
    ks = torch.tensor([0, 5], device=DEV, dtype=torch.int32)
    slopes = alibi_slopes(Hq).to(DEV)

    ref = reference.flash_prefill(q.float(), kc.float(), vc.float(), ks, 0, 0.125, tk=tk,
                                  alibi_slopes=slopes)
    plain = reference.flash_prefill(q.float(), kc.float(), vc.float(), ks, 0, 0.125, tk=tk)
    _assert_bias_matters(ref, plain, 3e-2)
    out = ops.flash_prefill(q, kc, vc, ks, 0, 0.125, tk=tk, alibi_slopes=slopes)
    torch.testing.assert_close(out.float(), ref, atol=3e-2, rtol=3e-2)

    qc = q[:, :, 64:].contiguous()
    _assert_bias_matters(ref[:, :, 64:], plain[:, :, 64:], 3e-2)
    out_c = ops.flash_prefill(qc, kc, vc, ks, 64, 0.125, tk=tk, alibi_slopes=slopes)
    ref_c = reference.flash_prefill(qc.float(), kc.float(), vc.float(), ks, 64, 0.125, tk=tk,
                                    alibi_slopes=slopes)
    torch.testing.assert_close(ref_c, ref[:, :, 64:], atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(out_c.float(), ref_c, atol=3e-2, rtol=3e-2)


# --------------------------------------------------------------------------
# flash attention forward + backward
# --------------------------------------------------------------------------


def _ref_grads(q, k, v, key_starts, scale, dout, slopes):
    qf = q.float().detach().requires_grad_(True)
    kf = k.float().detach().requires_grad_(True)
    vf = v.float().detach().requires_grad_(True)
    out = reference.flash_prefill(qf, kf, vf, key_starts, 0, scale, alibi_slopes=slopes)
    out.backward(dout.float())
    return out.detach(), qf.grad, kf.grad, vf.grad


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", [33, 64, 200])
def test_flash_attention_alibi_fwd_bwd_vs_autograd(D, T):
    torch.manual_seed(0)
    B, Hq = 3, 4
    q, k, v = _rand(B, Hq, T, D), _rand(B, Hq, T, D), _rand(B, Hq, T, D)
    dout = _rand(B, Hq, T, D)
    key_starts = torch.tensor([0, 3, 7], device=DEV, dtype=torch.int32)
    scale = 1.0 / D ** 0.5
    slopes = alibi_slopes(Hq).to(DEV).requires_grad_(True)

    ref_out, rdq, rdk, rdv = _ref_grads(q, k, v, key_starts, scale, dout, slopes.detach())
    plain = reference.flash_prefill(q.float(), k.float(), v.float(), key_starts, 0, scale)
    _assert_bias_matters(ref_out, plain, 3e-2)

    qg = q.detach().requires_grad_(True)
    kg = k.detach().requires_grad_(True)
    vg = v.detach().requires_grad_(True)
    out = ops.flash_attention(qg, kg, vg, key_starts, scale, alibi_slopes=slopes)
    out.backward(dout)

    torch.testing.assert_close(out.float(), ref_out, atol=3e-2, rtol=3e-2)
    torch.testing.assert_close(vg.grad.float(), rdv, atol=8e-2, rtol=8e-2)
    torch.testing.assert_close(kg.grad.float(), rdk, atol=8e-2, rtol=8e-2)
    torch.testing.assert_close(qg.grad.float(), rdq, atol=8e-2, rtol=8e-2)
    # the slopes are constants: no gradient comes back for them
    assert slopes.grad is None
    # left-pad positions carry exactly zero grad
    for b, ks in enumerate(key_starts.tolist()):
        if ks:
            assert torch.all(qg.grad[b, :, :ks] == 0)
            assert torch.all(kg.grad[b, :, :ks] == 0)
            assert torch.all(vg.grad[b, :, :ks] == 0)


def test_flash_attention_alibi_gqa_fwd_bwd():
    torch.manual_seed(1)
    B, Hq, Hkv, T, D = 2, 8, 2, 96, 64
    q, k, v = _rand(B, Hq, T, D), _rand(B, Hkv, T, D), _rand(B, Hkv, T, D)
    dout = _rand(B, Hq, T, D)
    ks = torch.tensor([0, 5], device=DEV, dtype=torch.int32)
    slopes = alibi_slopes(Hq).to(DEV)

    ref_out, rdq, rdk, rdv = _ref_grads(q, k, v, ks, 0.125, dout, slopes)
    plain = reference.flash_prefill(q.float(), k.float(), v.float(), ks, 0, 0.125)
    _assert_bias_matters(ref_out, plain, 3e-2)

    qg = q.detach().requires_grad_(True)
    kg = k.detach().requires_grad_(True)
    vg = v.detach().requires_grad_(True)
    out = ops.flash_attention(qg, kg, vg, ks, 0.125, alibi_slopes=slopes)
    out.backward(dout)
    torch.testing.assert_close(out.float(), ref_out, atol=3e-2, rtol=3e-2)
    torch.testing.assert_close(vg.grad.float(), rdv, atol=1e-1, rtol=8e-2)
    torch.testing.assert_close(kg.grad.float(), rdk, atol=1e-1, rtol=8e-2)
    torch.testing.assert_close(qg.grad.float(), rdq, atol=8e-2, rtol=8e-2)
    assert torch.all(kg.grad[1, :, :5] == 0) and torch.all(qg.grad[1, :, :5] == 0)


# --------------------------------------------------------------------------
# decode attention
# --------------------------------------------------------------------------


@pytest.mark.parametrize("D", [32, 64, 128, 256])
@pytest.mark.parametrize("gqa", [1, 4])
def test_attention_decode_alibi(D, gqa):
    torch.manual_seed(6)
    B, Hq, S = 4, 8, 257
    Hkv = Hq // gqa
    # query heads of one KV group share the SAME q vector: their outputs can
    # then differ only through the per-query-head slope
    q = _rand(B, Hkv, 1, D).repeat_interleave(gqa, dim=1).contiguous()
    k, v = _rand(B, Hkv, S, D), _rand(B, Hkv, S, D)
    seq_lens = torch.tensor([S, 100, 31, 1], dtype=torch.int32, device=DEV)
    starts = torch.tensor([0, 7, 0, 0], dtype=torch.int32, device=DEV)
    slopes = alibi_slopes(Hq).to(DEV)
    scale = 1.0 / math.sqrt(D)

    cpu = (q.float().cpu(), k.float().cpu(), v.float().cpu(), seq_lens.cpu(), scale)
    want = ops.attention_decode(*cpu, seq_starts=starts.cpu(), alibi_slopes=slopes.cpu())
    plain = ops.attention_decode(*cpu, seq_starts=starts.cpu())
    _assert_bias_matters(want, plain, 3e-2)

    out = ops.attention_decode(q, k, v, seq_lens, scale, seq_starts=starts, alibi_slopes=slopes)
    torch.testing.assert_close(out.float().cpu(), want, atol=3e-2, rtol=0)
    if gqa > 1:
        # slopes are indexed by the query head, not the KV head
        grp = out.float().view(B, Hkv, gqa, D)[0]  # row 0: 257 keys
        for a in range(gqa - 1):
            assert (grp[:, a] - grp[:, a + 1]).abs().max() > 3e-2


@pytest.mark.parametrize("D", [64, 128])
def test_fused_decode_attention_alibi(D):
    torch.manual_seed(7)
    B, H, S, idx = 3, 4, 40, 17
    qkv = _rand(B, 1, 3 * H * D)
    kc = torch.zeros(B, H, S, D, device=DEV).bfloat16()
    vc = torch.zeros(B, H, S, D, device=DEV).bfloat16()
    kc[:, :, :idx] = _rand(B, H, idx, D)
    vc[:, :, :idx] = _rand(B, H, idx, D)
    seq_lens = torch.full((B,), idx + 1, dtype=torch.int32, device=DEV)
    key_starts = torch.tensor([0, 2, 5], dtype=torch.int32, device=DEV)
    cache_idx = torch.tensor([idx], dtype=torch.long, device=DEV)
    slopes = alibi_slopes(H).to(DEV)
    scale = 1.0 / math.sqrt(D)

    # reference: append k/v by hand, then attention over the cache
    parts = qkv.view(B, 3, H, D)
    kr, vr = kc.clone(), vc.clone()
    kr[:, :, idx] = parts[:, 1]
    vr[:, :, idx] = parts[:, 2]
    cpu = (parts[:, 0].unsqueeze(2).float().cpu(), kr.float().cpu(), vr.float().cpu(),
           seq_lens.cpu(), scale)
    want = ops.attention_decode(*cpu, seq_starts=key_starts.cpu(), alibi_slopes=slopes.cpu())
    plain = ops.attention_decode(*cpu, seq_starts=key_starts.cpu())
    _assert_bias_matters(want, plain, 3e-2)

    out = ops.fused_decode_attention(qkv, kc, vc, seq_lens, key_starts, None, None, cache_idx,
                                     0, False, scale, alibi_slopes=slopes)
    assert out.shape == (B, H, 1, D)
    torch.testing.assert_close(out.float().cpu(), want, atol=3e-2, rtol=0)
    # the appended rows are the qkv slices, bit for bit; nothing else moved
    assert torch.equal(kc, kr) and torch.equal(vc, vr)


def test_fused_decode_attention_rejects_alibi_with_rope():
    B, H, S, D = 2, 2, 8, 64
    qkv = _rand(B, 1, 3 * H * D)
    kc = torch.zeros(B, H, S, D, device=DEV).bfloat16()
    vc = torch.zeros_like(kc)
    seq_lens = torch.ones(B, dtype=torch.int32, device=DEV)
    cache_idx = torch.zeros(1, dtype=torch.long, device=DEV)
    cos = torch.ones(S, D // 2, device=DEV)
    sin = torch.zeros(S, D // 2, device=DEV)
    with pytest.raises(RuntimeError, match="mutually exclusive"):
        ops.fused_decode_attention(qkv, kc, vc, seq_lens, None, cos, sin, cache_idx, D, False,
                                   0.125, alibi_slopes=alibi_slopes(H).to(DEV))
    with pytest.raises(RuntimeError, match="one slope per query head"):
        ops.attention_decode(_rand(B, H, 1, D), kc, vc, seq_lens, 0.125,
                             alibi_slopes=alibi_slopes(2 * H).to(DEV))


# --------------------------------------------------------------------------
# model level: tiny Bloom
# --------------------------------------------------------------------------


def _tiny_bloom_cfg():
    from trlx_amd.models.nn.config import preset

    cfg = preset("bloom-560m")
    cfg.num_layers = 2
    cfg.hidden_size = 256
    cfg.num_heads = 4
    cfg.num_kv_heads = 4
    cfg.intermediate_size = 512
    cfg.vocab_size = 1024
    return cfg


def test_bloom_graph_decode_matches_eager_greedy():
    """ALiBi models decode through the hipGraph engine, with the same decode
    kernels as the eager loop (exact greedy equality, as for GPT-2)."""
    from trlx_amd.models.nn.generation import GenerateConfig, generate
    from trlx_amd.models.nn.transformer import CausalTransformer

    torch.manual_seed(0)
    m = CausalTransformer(_tiny_bloom_cfg()).cuda().to(torch.bfloat16).eval()
    assert m.alibi_slopes.dtype == torch.float32 and m.alibi_slopes.is_cuda
    ids = torch.randint(3, 1000, (4, 12), device=DEV)
    mask = torch.ones_like(ids)
    mask[0, :5] = 0
    mask[2, :2] = 0

    gen_e = GenerateConfig(max_new_tokens=9, do_sample=False, eos_token_id=None, use_graph=False)
    out_eager = generate(m, ids, mask, gen=gen_e)
    assert getattr(m, "_decode_engine", None) is None
    gen_g = GenerateConfig(max_new_tokens=9, do_sample=False, eos_token_id=None, use_graph=True)
    out_graph = generate(m, ids, mask, gen=gen_g)
    assert torch.equal(out_eager, out_graph), (out_eager != out_graph).nonzero()
    # the graph path ran, and a second call reuses the captured graph
    engine = getattr(m, "_decode_engine", None)
    assert engine is not None and engine.graph is not None
    out_graph2 = generate(m, ids, mask, gen=gen_g)
    assert torch.equal(out_graph2, out_graph)
    assert m._decode_engine is engine


@pytest.fixture(scope="module")
def bloom_pair():
    """The same tiny Bloom twice: fp32 on the CPU (materializing attention,
    fp32 dense bias: the reference) and bf16 on the GPU (flash kernels), with
    the reference logits / loss / grads of one CE step computed once."""
    from trlx_amd.models.nn.transformer import CausalTransformer

    torch.manual_seed(3)
    ref_model = CausalTransformer(_tiny_bloom_cfg()).eval()
    gpu_model = copy.deepcopy(ref_model).cuda().bfloat16().eval()
    ids = torch.randint(3, 1000, (4, 130))
    mask = torch.ones_like(ids)
    mask[0, :9] = 0

    with torch.no_grad():
        ref_logits = ref_model(ids, attention_mask=mask).logits
    loss, grads = _ce_step(ref_model, ids, mask)
    ref_model.zero_grad(set_to_none=True)
    return dict(gpu=gpu_model, ids=ids.cuda(), mask=mask.cuda(), ref_logits=ref_logits,
                ref_loss=loss, ref_grads=grads)


def _ce_step(model, ids, mask):
    model.zero_grad(set_to_none=True)
    logits = model(ids, attention_mask=mask).logits
    loss = torch.nn.functional.cross_entropy(
        logits[:, :-1].flatten(0, 1).float(), ids[:, 1:].flatten())
    loss.backward()
    return loss.item(), {n: p.grad.detach().float().cpu().clone()
                         for n, p in model.named_parameters() if p.grad is not None}


def _spy(monkeypatch, name):
    calls = []
    real = getattr(ops, name)

    def wrapper(*args, **kwargs):
        calls.append(kwargs.get("alibi_slopes"))
        return real(*args, **kwargs)

    monkeypatch.setattr(ops, name, wrapper)
    return calls


def test_bloom_bf16_flash_vs_fp32_cpu_and_routing(bloom_pair, monkeypatch):
    """bf16 GPU Bloom (flash kernels with in-tile ALiBi) against the fp32 CPU
    copy of the same model: no_grad logits and the parameter grads of one CE
    step, at the limits of test_model_training_grads_flash_vs_materializing
    (relative max-error 0.12, |dloss| 5e-2).  The fp32 model is the reference
    on purpose: the bf16 materializing path rounds the bias itself.  Spies
    show the flash kernels served both passes, slopes included."""
    model, ids, mask = bloom_pair["gpu"], bloom_pair["ids"], bloom_pair["mask"]
    prefill_calls = _spy(monkeypatch, "flash_prefill")
    train_calls = _spy(monkeypatch, "flash_attention")

    with torch.no_grad():
        logits = model(ids, attention_mask=mask).logits
    assert len(prefill_calls) == 2 and not train_calls  # one per layer
    assert all(s is not None for s in prefill_calls)
    ref_logits = bloom_pair["ref_logits"]
    rel = (logits.float().cpu() - ref_logits).abs().max() / ref_logits.abs().max()
    print("logits rel max err", rel.item())
    assert rel < 0.12, rel.item()

    loss, grads = _ce_step(model, ids, mask)
    model.zero_grad(set_to_none=True)
    assert len(train_calls) == 2 and len(prefill_calls) == 2
    assert all(s is not None for s in train_calls)
    print("loss", loss, "ref", bloom_pair["ref_loss"])
    assert abs(loss - bloom_pair["ref_loss"]) < 5e-2, (loss, bloom_pair["ref_loss"])
    ref_grads = bloom_pair["ref_grads"]
    assert grads.keys() == ref_grads.keys() and len(grads) > 0
    for n in grads:
        denom = ref_grads[n].abs().max().clamp_min(1e-4)
        rel = (grads[n] - ref_grads[n]).abs().max() / denom
        print(n, "grad rel max err", rel.item())
        assert rel < 0.12, (n, rel.item())


def test_bloom_materializing_escape_hatch(bloom_pair, monkeypatch):
    """TRLX_AMD_NO_FLASH_PREFILL=1 keeps the [B,H,T,T] path reachable for
    ALiBi models: the dense bias is built lazily there."""
    model, ids, mask = bloom_pair["gpu"], bloom_pair["ids"], bloom_pair["mask"]
    prefill_calls = _spy(monkeypatch, "flash_prefill")
    train_calls = _spy(monkeypatch, "flash_attention")
    monkeypatch.setenv("TRLX_AMD_NO_FLASH_PREFILL", "1")
    with torch.no_grad():
        logits = model(ids, attention_mask=mask).logits
    loss, grads = _ce_step(model, ids, mask)
    model.zero_grad(set_to_none=True)
    assert not prefill_calls and not train_calls
    assert logits.shape == (4, 130, 1024) and torch.isfinite(logits.float()).all()
    assert math.isfinite(loss) and grads
    # same model and the same limits as the flash path: the lazily built bias
    # is the right one (its bf16 rounding, at most 2^-9 relative per element,
    # is of the order of the bf16 score rounding itself at T = 130)
    ref_logits = bloom_pair["ref_logits"]
    rel = (logits.float().cpu() - ref_logits).abs().max() / ref_logits.abs().max()
    print("materializing logits rel max err", rel.item())
    assert rel < 0.12, rel.item()
    assert abs(loss - bloom_pair["ref_loss"]) < 5e-2
