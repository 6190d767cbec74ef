"""kv_fp8.hip and attn_decode_fp8.hip: the store against the bit-level reference,
the attention against fp64 attention on the dequantized cache, and a tiny
Llama-shaped model generating on the fp8 cache."""
import functools

import pytest
import torch

from trlx_amd import ops
from trlx_amd.ops import reference

pytestmark = pytest.mark.gpu

B, S = 2, 83


# ---- store -------------------------------------------------------------------


def _store_inputs(D, T, layout):
    """k, v [B, Hkv=3, T, D] on the GPU in the given memory layout."""
    Hkv, g = 3, torch.Generator().manual_seed(D + T)
    k, v = (torch.randn(B, Hkv, T, D, generator=g).bfloat16() for _ in range(2))
    k[0, 1, 0] = 0.0                              # all-zero row: scale 0, codes 0
    v[1, 2, T - 1, 3], v[1, 2, T - 1, D - 1] = 9.0, -9.0  # +-absmax in one row
    if layout == "contiguous":
        return k.cuda(), v.cuda()
    if layout == "misaligned":  # base 2 B past a 16 B boundary: the scalar instantiation
        bufs = [torch.empty(x.numel() + 1, dtype=torch.bfloat16, device="cuda") for x in (k, v)]
        views = [b[1:].view(x.shape) for b, x in zip(bufs, (k, v))]
    else:  # "qkv": strided views of one fused [B, T, (Hq + 2 Hkv) D] projection output
        Hq = 5
        qkv = torch.zeros(B, T, (Hq + 2 * Hkv) * D, dtype=torch.bfloat16, device="cuda")
        views = [qkv[..., (Hq + i * Hkv) * D:(Hq + (i + 1) * Hkv) * D].view(B, T, Hkv, D)
                 .transpose(1, 2) for i in range(2)]
    for dst, src in zip(views, (k, v)):
        dst.copy_(src)
    return views


@pytest.mark.parametrize("layout", ["contiguous", "qkv", "misaligned"])
@pytest.mark.parametrize("T,start", [(19, 5), (1, torch.tensor([30])), (2, torch.tensor([0, 81]))],
                         ids=["host", "device", "per_row"])
@pytest.mark.parametrize("D", [64, 128])
def test_store_bit_equal_to_reference(D, T, start, layout):
    k, v = _store_inputs(D, T, layout)
    # sentinels: positions outside the written range must come back untouched
    want = [torch.full((B, 3, S, D), 0x55, dtype=torch.uint8), torch.full((B, 3, S), -1.0),
            torch.full((B, 3, S, D), 0x55, dtype=torch.uint8), torch.full((B, 3, S), -1.0)]
    got = [t.cuda() for t in want]
    ops.kv_store_fp8(k, v, *got, start.cuda() if torch.is_tensor(start) else start)
    reference.kv_store_fp8(k.cpu(), v.cpu(), *want, start)
    for g, w in zip(got, want):
        assert torch.equal(g.cpu(), w)
    assert not ((got[0] & 0x7F) == 0x7F).any() and (got[1] == 0).any()


def test_store_unsupported_raises():
    k, v = _store_inputs(64, 1, "contiguous")
    caches = [torch.zeros(B, 3, S, 64, dtype=torch.uint8, device="cuda"),
              torch.zeros(B, 3, S, device="cuda")] * 2
    with pytest.raises(ValueError, match="must be bf16"):
        ops.kv_store_fp8(k.float(), v.float(), *caches, 0)
    with pytest.raises(RuntimeError, match="do not fit"):
        ops.kv_store_fp8(k, v, *caches, S)
    with pytest.raises(RuntimeError, match="head dim must be 64 or 128"):
        ops.kv_store_fp8(k[..., :32], v[..., :32], caches[0][..., :32].contiguous(), caches[1],
                         caches[0][..., :32].contiguous(), caches[1], 0)


# ---- attention ------------------------------------------------------------------

# visible keys [start, len) per batch row.  "edge": one visible key / none.
WINDOWS = {"full": (None, [83, 37]), "tail": ([5, 33], [83, 70]), "edge": ([40, 50], [41, 50])}


def _reference(q, k, v, lens, starts, scale, slopes):
    """fp64 masked softmax attention; a row with no visible key gives zeros."""
    G = q.shape[1] // k.shape[1]
    kf, vf = (t.double().repeat_interleave(G, dim=1) for t in (k, v))
    pos = torch.arange(k.shape[2], device=q.device).view(1, 1, 1, -1)
    lo, hi = starts.view(-1, 1, 1, 1), lens.view(-1, 1, 1, 1)
    s = q.double() @ kf.transpose(-1, -2) * scale
    if slopes is not None:
        s = s + slopes.double().view(1, -1, 1, 1) * (pos - lo)
    p = torch.softmax(s.masked_fill((pos < lo) | (pos >= hi), float("-inf")), dim=-1)
    return p.nan_to_num(0.0) @ vf


@functools.lru_cache(maxsize=None)
def _case(D, Hq, Hkv, window, alibi):
    g = torch.Generator().manual_seed(D + 7 * Hq + Hkv)
    q = torch.randn(B, Hq, 1, D, generator=g).bfloat16().cuda()
    k = torch.randn(B, Hkv, S, D, generator=g).bfloat16()
    v = torch.randn(B, Hkv, S, D, generator=g).bfloat16()
    k[:, :, 10] = 0.0  # a visible key ("full", and row 0 of "tail") with scale 0
    starts, lens = WINDOWS[window]
    for b, n in enumerate(lens):  # a masked key that leaks shows up
        k[b, :, n:] = 1e4
        v[b, :, n:] = 1e4
    (k8, ks), (v8, vs) = ([t.cuda() for t in reference.kv_quantize_fp8(x)] for x in (k, v))
    lens = torch.tensor(lens, dtype=torch.int32, device="cuda")
    starts = None if starts is None else torch.tensor(starts, dtype=torch.int32, device="cuda")
    slopes = None
    if alibi:
        slopes = torch.pow(2.0, -8.0 * torch.arange(1, Hq + 1) / Hq).float().cuda()
    ref = _reference(q, reference.kv_dequantize_fp8(k8, ks), reference.kv_dequantize_fp8(v8, vs),
                     lens, torch.zeros_like(lens) if starts is None else starts, D ** -0.5, slopes)
    return q, k8, ks, v8, vs, lens, starts, slopes, ref


@pytest.mark.parametrize("alibi", [False, True])
@pytest.mark.parametrize("num_splits", [0, 3])  # 3: [64, 83) holds no visible key of a short row
@pytest.mark.parametrize("window", list(WINDOWS))
@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (8, 2), (17, 1)])  # 17 crosses the 16-head chunk
@pytest.mark.parametrize("D", [64, 128])
def test_attention_matches_fp64_on_dequantized_cache(D, Hq, Hkv, window, num_splits, alibi):
    q, k8, ks, v8, vs, lens, starts, slopes, ref = _case(D, Hq, Hkv, window, alibi)
    out = ops.attention_decode(q, k8, v8, lens, D ** -0.5, seq_starts=starts, alibi_slopes=slopes,
                               num_splits=num_splits, k_scale=ks, v_scale=vs)
    assert out.shape == q.shape and out.dtype == torch.bfloat16
    if window == "edge":
        assert torch.count_nonzero(out[1]) == 0
    print("max abs err", (out.double() - ref).abs().max().item())
    # the bound of tests/test_gqa_decode_gpu.py: after the dequantize the arithmetic is that kernel's
    torch.testing.assert_close(out.double(), ref, atol=3e-2, rtol=1e-3)


def test_attention_unsupported_raises():
    q, k8, ks, v8, vs, lens, _, _, _ = _case(64, 4, 4, "full", False)
    with pytest.raises(ValueError, match="k_scale and v_scale"):
        ops.attention_decode(q, k8, v8, lens, 0.125)
    with pytest.raises(ValueError, match="needs bf16 q"):
        ops.attention_decode(q.float(), k8, v8, lens, 0.125, k_scale=ks, v_scale=vs)
    with pytest.raises(RuntimeError, match="head dim must be 64 or 128"):
        ops.attention_decode(q[..., :32].contiguous(), k8[..., :32].contiguous(),
                             v8[..., :32].contiguous(), lens, 0.125, k_scale=ks, v_scale=vs)


# ---- model ------------------------------------------------------------------------


def _llama(Hq, Hkv):
    from trlx_amd.models.nn.config import preset
    from trlx_amd.models.nn.transformer import CausalTransformer

    torch.manual_seed(Hq + Hkv)
    cfg = preset("llama2-7b", vocab_size=480, hidden_size=64 * Hq, num_layers=2, num_heads=Hq,
                 num_kv_heads=Hkv, intermediate_size=256, max_position_embeddings=64)
    model = CausalTransformer(cfg).cuda().bfloat16().eval()
    model.rope_cos, model.rope_sin = model.rope_cos.float(), model.rope_sin.float()
    ids = torch.randint(3, 480, (3, 17), device="cuda")
    mask = torch.ones_like(ids)
    mask[0, :5] = 0
    mask[2, :2] = 0
    return model, ids, mask


@pytest.mark.parametrize("Hq,Hkv", [(4, 2), (2, 2)])
@torch.no_grad()
def test_model_steps_match_bf16_cache_of_dequantized_contents(Hq, Hkv, monkeypatch):
    monkeypatch.setenv("TRLX_AMD_FP8_KV", "1")
    monkeypatch.delenv("TRLX_AMD_FUSED_DECODE", raising=False)
    model, ids, mask = _llama(Hq, Hkv)
    T = ids.shape[1]
    kv8 = model.new_kv_cache(3, T + 3, kv_dtype=model.generation_kv_dtype())
    assert kv8.k[0].dtype == kv8.v[1].dtype == torch.uint8 and kv8.k_scale[0].dtype == torch.float32
    prefill = model(ids, attention_mask=mask, kv_cache=kv8, start_pos=0).logits
    torch.testing.assert_close(prefill.float(), model(ids, attention_mask=mask).logits.float(),
                               atol=8e-2, rtol=8e-2)
    key_starts = (T - mask.sum(-1)).to(torch.int32)
    for pos in range(T, T + 3):
        bf = model.new_kv_cache(3, T + 3)
        for l in range(2):
            bf.k[l].copy_(reference.kv_dequantize_fp8(kv8.k[l], kv8.k_scale[l]))
            bf.v[l].copy_(reference.kv_dequantize_fp8(kv8.v[l], kv8.v_scale[l]))
        step = dict(start_pos=pos, position_ids=(pos - key_starts).unsqueeze(1),
                    seq_lens=torch.full((3,), pos + 1, dtype=torch.int32, device="cuda"),
                    key_starts=key_starts, cache_idx=torch.tensor([pos], device="cuda"))
        tok = torch.randint(3, 480, (3, 1), device="cuda")
        want = model(tok, kv_cache=bf, **step).logits
        got = model(tok, kv_cache=kv8, **step).logits
        # the tolerance of the model-level tests in tests/test_headdim_gpu.py
        torch.testing.assert_close(got.float(), want.float(), atol=8e-2, rtol=8e-2)
    with pytest.raises(NotImplementedError, match="bf16 KVCache"):
        model(ids, attention_mask=mask, kv_cache=kv8, start_pos=4)


def test_decode_engine_captures_and_matches_uncaptured_steps(monkeypatch):
    from trlx_amd.models.nn.generation import GenerateConfig, generate

    monkeypatch.setenv("TRLX_AMD_FP8_KV", "1")
    monkeypatch.delenv("TRLX_AMD_FUSED_DECODE", raising=False)
    model, ids, mask = _llama(4, 2)
    gen = dict(max_new_tokens=6, do_sample=False, eos_token_id=None)
    eager = generate(model, ids, mask, gen=GenerateConfig(use_graph=False, **gen))
    graph = generate(model, ids, mask, gen=GenerateConfig(use_graph=True, **gen))
    engine = getattr(model, "_decode_engine", None)
    assert engine is not None and engine.graph is not None and engine.kv.fp8
    assert torch.equal(eager, graph), (eager != graph).nonzero()
    assert torch.equal(generate(model, ids, mask, gen=GenerateConfig(use_graph=True, **gen)), graph)
    monkeypatch.setenv("TRLX_AMD_FUSED_DECODE", "1")  # the stage kernels read a bf16 cache
    with pytest.raises(NotImplementedError, match="FUSED_DECODE"):
        model.generation_kv_dtype()
