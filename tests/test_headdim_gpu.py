"""Head dims 96 (GPT-NeoX-20B) and 256 (GPT-J) through the gfx950 attention
kernels: flash prefill, flash forward+backward, flash-decode and the fused MHA
decode step at the op level against the fp32 reference, and two tiny models
(NeoX-shaped, GPT-J-shaped) that must take the flash and hipGraph paths.

Tolerances are the project's own for the same kernels at D=64/128
(test_flash_prefill.py, test_flash_backward.py, test_ops.py): forward
atol = rtol = 3e-2, gradients 8e-2, decode atol = 3e-2.  Inputs are scaled as
in those files."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from trlx_amd import ops
    from trlx_amd.models.nn.config import preset
    from trlx_amd.models.nn.transformer import CausalTransformer, alibi_slopes
    from trlx_amd.ops import reference

    EXT = ops._load_ext()

DEV = "cuda"
HEAD_DIMS = [96, 256]


def _rand(*shape):
    return (torch.randn(*shape, device=DEV) * 0.5).bfloat16()


# --------------------------------------------------------------------------
# flash prefill (forward only)
# --------------------------------------------------------------------------


@pytest.mark.parametrize("D", HEAD_DIMS)
# 17: one partial tile; 33/97: partial edges of a 32-wide staged tile; 64: exact
# tile; 200: several 64-query blocks with a tail
@pytest.mark.parametrize("T", [17, 33, 64, 97, 200])
def test_flash_prefill_vs_reference(D, T):
    torch.manual_seed(0)
    B, Hq = 3, 4
    q, k = _rand(B, Hq, T, D), _rand(B, Hq, T, D)
    v = torch.randn(B, Hq, T, D, device=DEV).bfloat16()
    key_starts = torch.tensor([0, 3, 7], device=DEV, dtype=torch.int32)
    scale = 1.0 / D ** 0.5

    out = ops.flash_prefill(q, k, v, key_starts, 0, scale)
    ref = reference.flash_prefill(q.float(), k.float(), v.float(), key_starts, 0, scale)
    torch.testing.assert_close(out.float(), ref.float(), atol=3e-2, rtol=3e-2)


@pytest.mark.parametrize("D", HEAD_DIMS)
def test_flash_prefill_gqa_and_cache_stride(D):
    torch.manual_seed(1)
    B, Hq, Hkv, T, Sk = 2, 8, 2, 40, 96
    q = _rand(B, Hq, T, D)
    kc = torch.zeros(B, Hkv, Sk, D, device=DEV).bfloat16()
    vc = torch.zeros(B, Hkv, Sk, D, device=DEV).bfloat16()
    kc[:, :, :T] = _rand(B, Hkv, T, D)
    vc[:, :, :T] = torch.randn(B, Hkv, T, D, device=DEV).bfloat16()
    ks = torch.tensor([0, 5], device=DEV, dtype=torch.int32)
    scale = 1.0 / D ** 0.5
    out = ops.flash_prefill(q, kc, vc, ks, 0, scale, tk=T)
    ref = reference.flash_prefill(q.float(), kc.float(), vc.float(), ks, 0, scale, tk=T)
    torch.testing.assert_close(out.float(), ref.float(), atol=3e-2, rtol=3e-2)


@pytest.mark.parametrize("D", HEAD_DIMS)
def test_flash_prefill_start_pos_chunk(D):
    """Queries 64..95 as a start_pos=64 chunk against 96 valid keys of a cache
    with allocated stride 160."""
    torch.manual_seed(2)
    B, H, Sk, tk, sp = 2, 4, 160, 96, 64
    kc = torch.zeros(B, H, Sk, D, device=DEV).bfloat16()
    vc = torch.zeros(B, H, Sk, D, device=DEV).bfloat16()
    kc[:, :, :tk] = _rand(B, H, tk, D)
    vc[:, :, :tk] = torch.randn(B, H, tk, D, device=DEV).bfloat16()
    qc = _rand(B, H, tk - sp, D)
    ks = torch.tensor([0, 5], device=DEV, dtype=torch.int32)
    scale = 1.0 / D ** 0.5
    out = ops.flash_prefill(qc, kc, vc, ks, sp, scale, tk=tk)
    ref = reference.flash_prefill(qc.float(), kc.float(), vc.float(), ks, sp, scale, tk=tk)
    torch.testing.assert_close(out.float(), ref.float(), atol=3e-2, rtol=3e-2)


def _ref_lse(q, k, key_starts, scale, slopes):
    """Row logsumexp of the reference's scaled, biased, masked scores."""
    B, Hq, T, _ = q.shape
    scores = torch.matmul(q.float() * scale, k.float().transpose(-1, -2))
    i = torch.arange(T, device=q.device).view(1, 1, T, 1)
    j = torch.arange(T, device=q.device).view(1, 1, 1, T)
    ks = key_starts.view(B, 1, 1, 1)
    scores = scores + slopes.float().view(1, Hq, 1, 1) * (j - ks).clamp(min=0).float()
    scores = scores.masked_fill(~((j <= i) & (j >= ks)), float("-inf"))
    return torch.logsumexp(scores, dim=-1)


@pytest.mark.parametrize("D", HEAD_DIMS)
def test_flash_prefill_alibi_and_lse(D):
    torch.manual_seed(3)
    B, Hq, T = 3, 4, 97
    q, k, v = _rand(B, Hq, T, D), _rand(B, Hq, T, D), _rand(B, Hq, T, D)
    key_starts = torch.tensor([0, 3, 7], device=DEV, dtype=torch.int32)
    slopes = alibi_slopes(Hq).to(DEV)
    scale = 1.0 / D ** 0.5

    ref = reference.flash_prefill(q.float(), k.float(), v.float(), key_starts, 0, scale,
                                  alibi_slopes=slopes)
    plain = reference.flash_prefill(q.float(), k.float(), v.float(), key_starts, 0, scale)
    # a kernel that ignored the slopes could not pass
    assert (ref - plain).abs().max().item() >= 10 * 3e-2

    out, lse = EXT.flash_prefill_lse(q, k, v, key_starts, 0, scale, 0, True, slopes)
    torch.testing.assert_close(out.float(), ref, atol=3e-2, rtol=3e-2)
    want = _ref_lse(q, k, key_starts, scale, slopes)
    for b, ks in enumerate(key_starts.tolist()):
        # left-pad query rows see no key: the kernel stores +inf for them
        assert torch.all(lse[b, :, :ks] == float("inf"))
        torch.testing.assert_close(lse[b, :, ks:], want[b, :, ks:], atol=3e-2, rtol=3e-2)


# --------------------------------------------------------------------------
# flash attention forward + backward
# --------------------------------------------------------------------------


def _ref_grads(q, k, v, key_starts, scale, dout, slopes=None):
    qf = q.float().detach().requires_grad_(True)
    kf = k.float().detach().requires_grad_(True)
    vf = v.float().detach().requires_grad_(True)
    out = reference.flash_prefill(qf, kf, vf, key_starts, 0, scale, alibi_slopes=slopes)
    out.backward(dout.float())
    return out.detach(), qf.grad, kf.grad, vf.grad


def _flash_grads(q, k, v, key_starts, scale, dout, slopes=None):
    qg = q.detach().requires_grad_(True)
    kg = k.detach().requires_grad_(True)
    vg = v.detach().requires_grad_(True)
    out = ops.flash_attention(qg, kg, vg, key_starts, scale, alibi_slopes=slopes)
    out.backward(dout)
    return out.detach(), qg.grad, kg.grad, vg.grad


def _assert_grads_close(got, want):
    out, dq, dk, dv = got
    ref_out, rdq, rdk, rdv = want
    torch.testing.assert_close(out.float(), ref_out, atol=3e-2, rtol=3e-2)
    torch.testing.assert_close(dv.float(), rdv, atol=8e-2, rtol=8e-2)
    torch.testing.assert_close(dk.float(), rdk, atol=8e-2, rtol=8e-2)
    torch.testing.assert_close(dq.float(), rdq, atol=8e-2, rtol=8e-2)


@pytest.mark.parametrize("D", HEAD_DIMS)
@pytest.mark.parametrize("T", [33, 64, 97, 200])
def test_flash_attention_fwd_bwd_vs_autograd(D, T):
    torch.manual_seed(0)
    B, Hq = 3, 4
    q, k, v, dout = (_rand(B, Hq, T, D) for _ in range(4))
    key_starts = torch.tensor([0, 3, 7], device=DEV, dtype=torch.int32)
    scale = 1.0 / D ** 0.5

    got = _flash_grads(q, k, v, key_starts, scale, dout)
    _assert_grads_close(got, _ref_grads(q, k, v, key_starts, scale, dout))
    # left-pad positions carry exactly zero grad
    for b, ks in enumerate(key_starts.tolist()):
        for g in got[1:]:
            assert torch.all(g[b, :, :ks] == 0)
    assert got[2][1].abs().sum() > 0
    # deterministic: no atomics, fixed summation order
    again = _flash_grads(q, k, v, key_starts, scale, dout)
    for a, b_ in zip(got, again):
        assert torch.equal(a, b_)


@pytest.mark.parametrize("D", HEAD_DIMS)
def test_flash_attention_gqa_fwd_bwd(D):
    torch.manual_seed(1)
    B, Hq, Hkv, T = 2, 8, 2, 97
    q, dout = _rand(B, Hq, T, D), _rand(B, Hq, T, D)
    k, v = _rand(B, Hkv, T, D), _rand(B, Hkv, T, D)
    ks = torch.tensor([0, 5], device=DEV, dtype=torch.int32)
    scale = 1.0 / D ** 0.5
    got = _flash_grads(q, k, v, ks, scale, dout)
    _assert_grads_close(got, _ref_grads(q, k, v, ks, scale, dout))
    assert torch.all(got[2][1, :, :5] == 0) and torch.all(got[1][1, :, :5] == 0)


@pytest.mark.parametrize("D", HEAD_DIMS)
def test_flash_attention_alibi_fwd_bwd(D):
    torch.manual_seed(4)
    B, Hq, T = 3, 4, 97
    q, k, v, dout = (_rand(B, Hq, T, D) for _ in range(4))
    key_starts = torch.tensor([0, 3, 7], device=DEV, dtype=torch.int32)
    slopes = alibi_slopes(Hq).to(DEV)
    scale = 1.0 / D ** 0.5
    want = _ref_grads(q, k, v, key_starts, scale, dout, slopes)
    plain = reference.flash_prefill(q.float(), k.float(), v.float(), key_starts, 0, scale)
    assert (want[0] - plain).abs().max().item() >= 10 * 3e-2
    _assert_grads_close(_flash_grads(q, k, v, key_starts, scale, dout, slopes), want)


# --------------------------------------------------------------------------
# decode attention at D=96
# --------------------------------------------------------------------------


@pytest.mark.parametrize("gqa,alibi", [(1, False), (4, False), (4, True)])
def test_attention_decode_d96(gqa, alibi):
    """Lengths 1/31/100/257 leave every remainder of a 4-key lane group."""
    torch.manual_seed(6)
    B, Hq, S, D = 4, 8, 257, 96
    Hkv = Hq // gqa
    if alibi:  # scaled like test_alibi_gpu.py so the bias moves the output
        q, k, v = _rand(B, Hq, 1, D), _rand(B, Hkv, S, D), _rand(B, Hkv, S, D)
    else:
        q = torch.randn(B, Hq, 1, D).bfloat16().cuda()
        k = torch.randn(B, Hkv, S, D).bfloat16().cuda()
        v = torch.randn(B, Hkv, S, D).bfloat16().cuda()
    seq_lens = torch.tensor([S, 100, 31, 1], dtype=torch.int32, device=DEV)
    starts = torch.tensor([0, 7, 0, 0], dtype=torch.int32, device=DEV)
    slopes = alibi_slopes(Hq).to(DEV) if alibi else None
    scale = 1.0 / math.sqrt(D)

    cpu = (q.float().cpu(), k.float().cpu(), v.float().cpu(), seq_lens.cpu(), scale)
    want = ops.attention_decode(*cpu, seq_starts=starts.cpu(),
                                alibi_slopes=slopes.cpu() if alibi else None)
    if alibi:
        plain = ops.attention_decode(*cpu, seq_starts=starts.cpu())
        assert (want - plain).abs().max().item() >= 10 * 3e-2
    out = ops.attention_decode(q, k, v, seq_lens, scale, seq_starts=starts, alibi_slopes=slopes)
    torch.testing.assert_close(out.float().cpu(), want, atol=3e-2, rtol=0)


def test_fused_decode_attention_d96_rope():
    """NeoX-20B head: D=96, rot=24, non-interleaved.  One kernel must equal the
    eager split + reference RoPE at position idx - key_start + cache append +
    the CPU attention_decode reference."""
    torch.manual_seed(7)
    B, H, S, D, rot, idx = 3, 4, 40, 96, 24, 17
    qkv = _rand(B, 1, 3 * H * D)
    kc = torch.zeros(B, H, S, D, device=DEV).bfloat16()
    vc = torch.zeros(B, H, S, D, device=DEV).bfloat16()
    kc[:, :, :idx] = _rand(B, H, idx, D)
    vc[:, :, :idx] = _rand(B, H, idx, D)
    seq_lens = torch.full((B,), idx + 1, dtype=torch.int32, device=DEV)
    key_starts = torch.tensor([0, 2, 5], dtype=torch.int32, device=DEV)
    cache_idx = torch.tensor([idx], dtype=torch.long, device=DEV)
    cos, sin = reference.rope_cos_sin(S, rot, device=DEV)
    scale = 1.0 / math.sqrt(D)

    parts = qkv.view(B, 3, H, 1, D)
    qr, knew = parts[:, 0].clone(), parts[:, 1].clone()  # [B, H, 1, D]
    for b in range(B):
        p = idx - int(key_starts[b])
        qb, kb = reference.apply_rope(qr[b:b + 1, ..., :rot], knew[b:b + 1, ..., :rot],
                                      cos[p:p + 1], sin[p:p + 1], interleaved=False)
        qr[b:b + 1, ..., :rot], knew[b:b + 1, ..., :rot] = qb, kb
    kr, vr = kc.clone(), vc.clone()
    kr[:, :, idx] = knew[:, :, 0]
    vr[:, :, idx] = parts[:, 2, :, 0]
    want = ops.attention_decode(qr.float().cpu(), kr.float().cpu(), vr.float().cpu(),
                                seq_lens.cpu(), scale, seq_starts=key_starts.cpu())

    out = ops.fused_decode_attention(qkv, kc, vc, seq_lens, key_starts, cos, sin, cache_idx,
                                     rot, False, scale)
    assert out.shape == (B, H, 1, D)
    torch.testing.assert_close(out.float().cpu(), want, atol=3e-2, rtol=0)
    # appended rows: V and the unrotated K dims are copies, bit for bit; the
    # rotated K dims are fp32 math rounded once to bf16 on both sides, so they
    # agree to one bf16 ulp (2^-8 relative) where fma contraction moves a tie
    assert torch.equal(vc, vr)
    assert torch.equal(kc[..., rot:], kr[..., rot:])
    torch.testing.assert_close(kc[:, :, idx, :rot].float(), kr[:, :, idx, :rot].float(),
                               atol=2.0 ** -10, rtol=2.0 ** -8)
    keep = torch.ones(S, dtype=torch.bool, device=DEV)
    keep[idx] = False
    assert torch.equal(kc[:, :, keep], kr[:, :, keep])  # nothing else moved


# --------------------------------------------------------------------------
# decode instantiations no other op-level test launches
# --------------------------------------------------------------------------
# attention_decode: (D, ALiBi) is 5 x 2; test_ops.py has D=64/128 without the
# bias, test_alibi_gpu.py D=32/64/128/256 with it, this file D=96 both ways.
# fused_decode_attention: (D, mode) is 5 x 3; test_alibi_gpu.py has ALiBi at
# D=64/128 and this file non-interleaved RoPE at D=96.  The cases below are the
# rest.  Inputs come from the CPU generator, so the references (and the checks
# that a wrong mode would move them) do not depend on the device.


def _cpu_rand(*shape):
    return (torch.randn(*shape) * 0.5).bfloat16()


@pytest.mark.parametrize("D", [32, 256])
def test_attention_decode_plain_d32_d256(D):
    torch.manual_seed(8)
    B, Hq, Hkv, S = 2, 4, 2, 80
    q, k, v = _cpu_rand(B, Hq, 1, D), _cpu_rand(B, Hkv, S, D), _cpu_rand(B, Hkv, S, D)
    seq_lens = torch.tensor([S, 33], dtype=torch.int32)
    starts = torch.tensor([0, 7], dtype=torch.int32)  # row 1 is left-padded
    scale = 1.0 / math.sqrt(D)
    want = ops.attention_decode(q.float(), k.float(), v.float(), seq_lens, scale,
                                seq_starts=starts)
    out = ops.attention_decode(q.to(DEV), k.to(DEV), v.to(DEV), seq_lens.to(DEV), scale,
                               seq_starts=starts.to(DEV))
    torch.testing.assert_close(out.float().cpu(), want, atol=3e-2, rtol=0)


_FUSED_MODES = ("alibi", "rope_interleaved", "rope")
_FUSED_ELSEWHERE = {(64, "alibi"), (128, "alibi"), (96, "rope")}


def _fused_decode_reference(qkv, kc, vc, seq_lens, key_starts, idx, mode, scale):
    """Eager split + reference RoPE over the first D/2 dims at position
    idx - key_start (ALiBi: no rotation, slopes in the attention) + cache
    append + the CPU attention_decode reference.  All on the CPU."""
    B, H, S, D = kc.shape
    rot = 0 if mode == "alibi" else D // 2
    parts = qkv.view(B, 3, H, 1, D)
    qr, knew = parts[:, 0].clone(), parts[:, 1].clone()  # [B, H, 1, D]
    if rot:
        cos, sin = reference.rope_cos_sin(S, rot)
        for b in range(B):
            p = idx - int(key_starts[b])
            qb, kb = reference.apply_rope(qr[b:b + 1, ..., :rot], knew[b:b + 1, ..., :rot],
                                          cos[p:p + 1], sin[p:p + 1],
                                          interleaved=mode == "rope_interleaved")
            qr[b:b + 1, ..., :rot], knew[b:b + 1, ..., :rot] = qb, kb
    kr, vr = kc.clone(), vc.clone()
    kr[:, :, idx] = knew[:, :, 0]
    vr[:, :, idx] = parts[:, 2, :, 0]
    want = ops.attention_decode(qr.float(), kr.float(), vr.float(), seq_lens, scale,
                                seq_starts=key_starts,
                                alibi_slopes=alibi_slopes(H) if mode == "alibi" else None)
    return want, kr, vr, rot


def _fused_decode_case(D, mode):
    """CPU inputs and reference of one case; shows on the reference alone that
    a kernel of another mode could not pass (each moves it past the tolerance)."""
    torch.manual_seed(9)
    B, H, S, idx = 2, 4, 80, 70
    qkv = _cpu_rand(B, 1, 3 * H * D)
    kc, vc = torch.zeros(B, H, S, D).bfloat16(), torch.zeros(B, H, S, D).bfloat16()
    kc[:, :, :idx], vc[:, :, :idx] = _cpu_rand(B, H, idx, D), _cpu_rand(B, H, idx, D)
    seq_lens = torch.full((B,), idx + 1, dtype=torch.int32)
    key_starts = torch.tensor([0, 5], dtype=torch.int32)  # row 1 is left-padded
    args = (qkv, kc, vc, seq_lens, key_starts, idx)
    scale = 1.0 / math.sqrt(D)
    want, kr, vr, rot = _fused_decode_reference(*args, mode, scale)
    for other in _FUSED_MODES:
        if other != mode:
            moved = (_fused_decode_reference(*args, other, scale)[0] - want).abs().max().item()
            assert moved > 3e-2, f"mode {other} moves the reference by {moved:.3g}"
    return args, scale, rot, want, kr, vr


@pytest.mark.parametrize("D,mode", [(D, m) for D in (32, 64, 96, 128, 256) for m in _FUSED_MODES
                                    if (D, m) not in _FUSED_ELSEWHERE])
def test_fused_decode_attention_every_mode(D, mode):
    (qkv, kc, vc, seq_lens, key_starts, idx), scale, rot, want, kr, vr = _fused_decode_case(D, mode)
    B, H, S, _ = kc.shape
    cos, sin = reference.rope_cos_sin(S, rot, device=DEV) if rot else (None, None)
    kg, vg = kc.to(DEV), vc.to(DEV)
    out = ops.fused_decode_attention(
        qkv.to(DEV), kg, vg, seq_lens.to(DEV), key_starts.to(DEV), cos, sin,
        torch.tensor([idx], dtype=torch.long, device=DEV), rot, mode == "rope_interleaved", scale,
        alibi_slopes=alibi_slopes(H).to(DEV) if mode == "alibi" else None)
    assert out.shape == (B, H, 1, D)
    torch.testing.assert_close(out.float().cpu(), want, atol=3e-2, rtol=0)
    # appended rows: V and the unrotated K dims are copies, bit for bit; the
    # rotated K dims agree to one bf16 ulp (see test_fused_decode_attention_d96_rope)
    assert torch.equal(vg.cpu(), vr)
    assert torch.equal(kg.cpu()[..., rot:], kr[..., rot:])
    torch.testing.assert_close(kg.cpu()[:, :, idx, :rot].float(), kr[:, :, idx, :rot].float(),
                               atol=2.0 ** -10, rtol=2.0 ** -8)


# --------------------------------------------------------------------------
# tiny NeoX-shaped (D=96) and GPT-J-shaped (D=256) models
# --------------------------------------------------------------------------


def _tiny_model(kind, max_pos=256):
    if kind == "neox":  # D=96, rot=24 non-interleaved, parallel residual
        cfg = preset("gpt-neox-20b", vocab_size=480, hidden_size=192, num_layers=3,
                     num_heads=2, max_position_embeddings=max_pos)
    else:  # D=256, rot=64 interleaved, parallel residual
        cfg = preset("gptj-6b", vocab_size=480, hidden_size=512, num_layers=2, num_heads=2,
                     max_position_embeddings=max_pos)
    assert cfg.head_dim == {"neox": 96, "gptj": 256}[kind] and cfg.rope_pct == 0.25
    model = CausalTransformer(cfg).cuda().bfloat16()
    # rope tables must stay fp32 (cast_compute semantics)
    model.rope_cos = model.rope_cos.float()
    model.rope_sin = model.rope_sin.float()
    return model


def _count_calls(monkeypatch, name):
    calls = []
    real = getattr(ops, name)

    def counted(*args, **kwargs):
        calls.append(name)
        return real(*args, **kwargs)

    monkeypatch.setattr(ops, name, counted)
    return calls


def _padded_batch(vocab=480, B=4, T=130):
    ids = torch.randint(3, vocab, (B, T), device=DEV)
    mask = torch.ones_like(ids)
    mask[0, :9] = 0
    return ids, mask


@pytest.mark.parametrize("kind", ["neox", "gptj"])
def test_model_forward_flash_matches_materializing(kind, monkeypatch):
    torch.manual_seed(2)
    model = _tiny_model(kind).eval()
    ids, mask = _padded_batch()
    calls = _count_calls(monkeypatch, "flash_prefill")
    # flash on: the default at D=96; D=256 measured slower than the materializing
    # path, so there the same switch set to 0 turns it on
    if not ops.flash_enabled(model.config.head_dim, train=False):
        monkeypatch.setenv("TRLX_AMD_NO_FLASH_PREFILL", "0")
    with torch.no_grad():
        flash_logits = model(ids, attention_mask=mask).logits
        assert len(calls) == model.config.num_layers, "flash_prefill was not engaged"
        monkeypatch.setenv("TRLX_AMD_NO_FLASH_PREFILL", "1")
        mat_logits = model(ids, attention_mask=mask).logits
        assert len(calls) == model.config.num_layers  # the escape hatch still works
    torch.testing.assert_close(flash_logits.float(), mat_logits.float(), atol=8e-2, rtol=8e-2)


@pytest.mark.parametrize("kind", ["neox", "gptj"])
def test_model_training_grads_flash_vs_materializing(kind, monkeypatch):
    torch.manual_seed(3)
    model = _tiny_model(kind)
    ids, mask = _padded_batch()
    calls = _count_calls(monkeypatch, "flash_attention")
    # the training direction is not the default at either head dim (measured
    # slower than the materializing path): the switch set to 0 turns it on
    monkeypatch.setenv("TRLX_AMD_NO_FLASH_TRAIN", "0")

    def step():
        model.zero_grad(set_to_none=True)
        logits = model(ids, attention_mask=mask).logits
        loss = torch.nn.functional.cross_entropy(
            logits[:, :-1].flatten(0, 1).float(), ids[:, 1:].flatten())
        loss.backward()
        return loss.item(), {n: p.grad.detach().float().clone()
                             for n, p in model.named_parameters() if p.grad is not None}

    loss_f, grads_f = step()
    assert len(calls) == model.config.num_layers, "flash_attention was not engaged"
    monkeypatch.setenv("TRLX_AMD_NO_FLASH_PREFILL", "1")
    loss_m, grads_m = step()
    assert len(calls) == model.config.num_layers

    assert abs(loss_f - loss_m) < 5e-2, (loss_f, loss_m)
    assert grads_f.keys() == grads_m.keys() and len(grads_f) > 0
    for n in grads_f:
        gf, gm = grads_f[n], grads_m[n]
        denom = gm.abs().max().clamp_min(1e-4)
        rel = (gf - gm).abs().max() / denom
        assert rel < 0.12, (n, rel.item())


def test_graph_decode_d96_matches_eager_greedy():
    """NeoX-shaped model: generate() builds the hipGraph DecodeEngine and it
    reproduces the eager loop token for token (greedy)."""
    from trlx_amd.models.nn.generation import GenerateConfig, generate

    torch.manual_seed(0)
    model = _tiny_model("neox").eval()
    ids = torch.randint(3, 480, (4, 12), device=DEV)
    mask = torch.ones_like(ids)
    mask[0, :5] = 0
    mask[2, :2] = 0

    gen_e = GenerateConfig(max_new_tokens=9, do_sample=False, eos_token_id=None, use_graph=False)
    out_eager = generate(model, ids, mask, gen=gen_e)
    assert getattr(model, "_decode_engine", None) is None
    gen_g = GenerateConfig(max_new_tokens=9, do_sample=False, eos_token_id=None, use_graph=True)
    out_graph = generate(model, ids, mask, gen=gen_g)
    assert getattr(model, "_decode_engine", None) is not None, "graph engine was skipped"
    assert torch.equal(out_eager, out_graph), (out_eager != out_graph).nonzero()
    out_graph2 = generate(model, ids, mask, gen=gen_g)  # replays the captured graph
    assert torch.equal(out_graph2, out_graph)


def test_training_peak_memory_d256_flash_below_materializing(monkeypatch):
    """B=2, H=2, T=1024, D=256: one training step with flash attention saves
    O(T) per row (the logsumexp); the materializing path saves the O(T^2)
    probabilities, so its peak must be strictly higher."""
    torch.manual_seed(5)
    model = _tiny_model("gptj", max_pos=1024)
    ids = torch.randint(3, 480, (2, 1024), device=DEV)

    def peak():
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        logits = model(ids).logits
        logits[:, :-1].float().logsumexp(-1).mean().backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated()

    monkeypatch.setenv("TRLX_AMD_NO_FLASH_TRAIN", "0")
    calls = _count_calls(monkeypatch, "flash_attention")
    peak()  # warm-up: workspace and allocator pools exist before either measurement
    flash = peak()
    assert len(calls) == 2 * model.config.num_layers, "flash_attention was not engaged"
    monkeypatch.setenv("TRLX_AMD_NO_FLASH_TRAIN", "1")
    materializing = peak()
    assert flash < materializing, (flash, materializing)
