"""ALiBi (Bloom) position bias through the attention paths, CPU side: the
KV-cache decode step carries the bias, the fp32 references take per-head
slopes, and greedy generation agrees with the full forward."""

import pytest
import torch

from trlx_amd import ops
from trlx_amd.models.nn.generation import GenerateConfig, generate
from trlx_amd.models.nn.transformer import CausalTransformer, alibi_slopes
from trlx_amd.ops import reference

from conftest import tiny_config


def _tiny_bloom(**overrides):
    return tiny_config(position_encoding="alibi", arch_name="bloom", **overrides)


def test_alibi_kv_cache_decode_matches_full_forward():
    """Incremental decode with the KV cache must reproduce the full forward
    for an ALiBi model too (the decode attention used to drop the bias, so
    sampling and scoring saw different distributions)."""
    torch.manual_seed(0)
    cfg = _tiny_bloom()
    m = CausalTransformer(cfg).eval()
    B, T = 2, 10
    ids = torch.randint(3, 300, (B, T))
    mask = torch.ones_like(ids)
    mask[0, :3] = 0
    with torch.no_grad():
        full = m(ids, attention_mask=mask).logits

        kv = m.new_kv_cache(B, T)
        pre = m(ids[:, :5], attention_mask=mask[:, :5], kv_cache=kv, start_pos=0).logits
        key_starts = (5 - mask[:, :5].sum(-1)).to(torch.int32)
        step_logits = [pre[:, -1]]
        for t in range(5, T):
            pos = (t - key_starts).to(torch.int32).unsqueeze(1)
            seq_lens = torch.full((B,), t + 1, dtype=torch.int32)
            out = m(ids[:, t : t + 1], kv_cache=kv, start_pos=t, position_ids=pos,
                    seq_lens=seq_lens, key_starts=key_starts)
            step_logits.append(out.logits[:, -1])
    inc = torch.stack(step_logits, dim=1)  # logits at positions 4..T-1
    want = full[:, 4:]
    assert torch.allclose(inc, want, atol=1e-4), (inc - want).abs().max()


def _explicit_attention(q, k, v, scale, slopes, key_starts, visible):
    """softmax(Q K^T * scale + bias + mask) V written out: q [B,Hq,Tq,D],
    k/v [B,Hkv,Tk,D], visible [B,1,Tq,Tk] bool."""
    B, Hq, Tq, D = q.shape
    Hkv, Tk = k.shape[1], k.shape[2]
    out = torch.zeros(B, Hq, Tq, D)
    for b in range(B):
        for h in range(Hq):
            kk, vv = k[b, h // (Hq // Hkv)], v[b, h // (Hq // Hkv)]
            s = (q[b, h] @ kk.T) * scale  # [Tq, Tk]
            bias = slopes[h] * (torch.arange(Tk) - int(key_starts[b])).clamp(min=0).float()
            s = s + bias.unsqueeze(0)
            s = s.masked_fill(~visible[b, 0], float("-inf"))
            out[b, h] = torch.softmax(s, dim=-1) @ vv
    return out


@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (8, 2)])
def test_reference_flash_prefill_alibi_matches_explicit(Hq, Hkv):
    torch.manual_seed(1)
    B, T, D = 2, 12, 16
    q = torch.randn(B, Hq, T, D)
    k = torch.randn(B, Hkv, T, D)
    v = torch.randn(B, Hkv, T, D)
    key_starts = torch.tensor([0, 3], dtype=torch.int32)
    slopes = alibi_slopes(Hq)
    scale = D ** -0.5
    i = torch.arange(T).view(1, 1, T, 1)
    j = torch.arange(T).view(1, 1, 1, T)
    visible = (j <= i) & (j >= key_starts.view(B, 1, 1, 1))
    want = _explicit_attention(q, k, v, scale, slopes, key_starts, visible)
    got = reference.flash_prefill(q, k, v, key_starts, 0, scale, alibi_slopes=slopes)
    # left-pad query rows see no key at all: the reference zeroes them
    rows = (torch.arange(T).view(1, T) >= key_starts.view(B, 1)).view(B, 1, T, 1)
    assert torch.allclose(got * rows, torch.nan_to_num(want) * rows, atol=1e-5), \
        (got - want).abs().max()
    # the argument is not ignored
    plain = reference.flash_prefill(q, k, v, key_starts, 0, scale)
    assert (got - plain).abs().max() > 1e-3
    # ops-level CPU entry points forward it
    assert torch.equal(ops.flash_prefill(q, k, v, key_starts, 0, scale, alibi_slopes=slopes), got)
    assert torch.equal(ops.flash_attention(q, k, v, key_starts, scale, alibi_slopes=slopes), got)


@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (8, 2)])
def test_cpu_attention_decode_alibi_matches_explicit(Hq, Hkv):
    torch.manual_seed(2)
    B, S, D = 2, 11, 16
    q = torch.randn(B, Hq, 1, D)
    kc = torch.randn(B, Hkv, S, D)
    vc = torch.randn(B, Hkv, S, D)
    seq_lens = torch.tensor([11, 7], dtype=torch.int32)
    key_starts = torch.tensor([0, 3], dtype=torch.int32)
    slopes = alibi_slopes(Hq)
    scale = D ** -0.5
    j = torch.arange(S).view(1, 1, 1, S)
    visible = (j < seq_lens.view(B, 1, 1, 1)) & (j >= key_starts.view(B, 1, 1, 1))
    want = _explicit_attention(q, kc, vc, scale, slopes, key_starts, visible)
    got = ops.attention_decode(q, kc, vc, seq_lens, scale, seq_starts=key_starts,
                               alibi_slopes=slopes)
    assert torch.allclose(got, want, atol=1e-5), (got - want).abs().max()
    plain = ops.attention_decode(q, kc, vc, seq_lens, scale, seq_starts=key_starts)
    assert (got - plain).abs().max() > 1e-3
    if Hq != Hkv:
        # slopes are per QUERY head: heads sharing a KV head differ by more
        # than their q alone explains -> compare against slopes indexed by hkv
        wrong = ops.attention_decode(q, kc, vc, seq_lens, scale, seq_starts=key_starts,
                                     alibi_slopes=slopes[torch.arange(Hq) // (Hq // Hkv)])
        assert (got - wrong).abs().max() > 1e-3


def test_alibi_greedy_generate_matches_full_forward_argmax():
    """Every greedily generated token is the argmax of a full (cache-less)
    forward over the sequence generated so far."""
    torch.manual_seed(3)
    cfg = _tiny_bloom()
    m = CausalTransformer(cfg).eval()
    B, T, N = 2, 6, 6
    ids = torch.randint(3, 300, (B, T))
    mask = torch.ones_like(ids)
    mask[0, :2] = 0
    out = generate(m, ids, attention_mask=mask,
                   gen=GenerateConfig(max_new_tokens=N, do_sample=False, eos_token_id=None))
    assert out.shape == (B, T + N)
    full_mask = torch.cat([mask, torch.ones(B, N, dtype=mask.dtype)], dim=1)
    with torch.no_grad():
        logits = m(out, attention_mask=full_mask).logits
    assert torch.equal(logits[:, T - 1 : -1].argmax(-1), out[:, T:])


def test_alibi_hydra_frozen_branch_matches_base_at_init():
    """The hydra branches build their own attention context: it must carry
    the slopes too, or the frozen reference scores a bias-free model."""
    from trlx_amd.models.modeling_ppo import AutoModelForCausalLMWithHydraValueHead

    torch.manual_seed(0)
    model = AutoModelForCausalLMWithHydraValueHead.from_config(_tiny_bloom(),
                                                               num_layers_unfrozen=1)
    model.eval()
    ids = torch.randint(3, 300, (2, 8))
    mask = torch.ones_like(ids)
    mask[0, :2] = 0
    with torch.no_grad():
        out = model(ids, attention_mask=mask, return_ref_logits=True)
        hydra_only = model.forward_hydra(ids, attention_mask=mask)
    assert torch.allclose(out.ref_logits, out.logits, atol=1e-4)
    assert torch.allclose(hydra_only.logits, out.logits, atol=1e-4)


def test_fused_stage_decode_still_refuses_alibi():
    """The opt-in stage-kernel decode step passes no slopes: it must keep
    turning ALiBi models away (the engine then uses the module path)."""
    from trlx_amd.models.nn.generation import FusedStageRefs

    shape = dict(hidden_size=128, num_heads=2)  # head dim 64: otherwise eligible
    ok = CausalTransformer(tiny_config(**shape)).to(torch.bfloat16).eval()
    FusedStageRefs(ok, 2, torch.device("cpu"))
    m = CausalTransformer(_tiny_bloom(**shape)).to(torch.bfloat16).eval()
    with pytest.raises(ValueError):
        FusedStageRefs(m, 2, torch.device("cpu"))


def test_alibi_slopes_buffer_stays_fp32_and_out_of_checkpoints():
    cfg = _tiny_bloom()
    m = CausalTransformer(cfg)
    assert "alibi_slopes" not in m.state_dict()
    want = alibi_slopes(cfg.num_heads)
    m = m.to(torch.bfloat16)
    assert m.alibi_slopes.dtype == torch.float32
    assert torch.equal(m.alibi_slopes, want)
    assert CausalTransformer(tiny_config()).alibi_slopes is None
