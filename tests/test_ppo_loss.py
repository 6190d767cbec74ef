"""PPOConfig.loss without the fused kernel: same keys, order and values as the
plain-torch formulas it had before ops.ppo_loss existed (copied below), and
the TRLX_AMD_NO_FUSED_PPO_LOSS switch."""

import types

import torch

from trlx_amd import ops
from trlx_amd.models.modeling_ppo import PPOConfig

EXPECTED_KEYS = [
    "losses/total_loss", "losses/policy_loss", "losses/value_loss",
    "values/mean", "values/min", "values/max", "values/std", "values/values_error", "values/clipfrac",
    "old_values/mean", "old_values/min", "old_values/max", "old_values/std",
    "returns/mean", "returns/min", "returns/max", "returns/std",
    "policy/approx_kl", "policy/clipfrac", "ratio", "padding_percentage",
]


def _tensor_stats(xs, mask, n):
    mean = (xs * mask).sum() / n
    minimum = torch.where(mask.bool(), xs, torch.full_like(xs, float("inf"))).min()
    maximum = torch.where(mask.bool(), xs, torch.full_like(xs, float("-inf"))).max()
    denom = torch.clamp(torch.as_tensor(n, dtype=torch.float32, device=xs.device) - 1, min=1)
    std = torch.sqrt(((xs - mean) * mask).pow(2).sum() / denom)
    return dict(mean=mean, min=minimum, max=maximum, std=std)


def expected_loss(cfg, logprobs, values, old_logprobs, old_values, advantages, returns, mask):
    """The formulas of PPOConfig.loss before the fused kernel, verbatim."""
    values_clipped = torch.clamp(values, old_values - cfg.cliprange_value, old_values + cfg.cliprange_value)
    n = mask.sum()
    vf_loss1 = (values - returns) ** 2
    vf_loss2 = (values_clipped - returns) ** 2
    vf_loss = 0.5 * torch.sum(torch.max(vf_loss1, vf_loss2) * mask) / n
    vf_clipfrac = torch.sum((vf_loss2 > vf_loss1).float() * mask) / n
    log_ratio = (logprobs - old_logprobs) * mask
    ratio = torch.exp(log_ratio)
    with torch.no_grad():
        approx_kl = torch.mean((ratio - 1) - log_ratio)
    pg_loss1 = -advantages * ratio
    pg_loss2 = -advantages * torch.clamp(ratio, 1.0 - cfg.cliprange, 1.0 + cfg.cliprange)
    pg_loss = torch.sum(torch.max(pg_loss1, pg_loss2) * mask) / n
    pg_clipfrac = torch.sum((pg_loss2 > pg_loss1).float() * mask) / n
    loss = pg_loss + cfg.vf_coef * vf_loss
    stats = {
        "losses/total_loss": loss.detach(),
        "losses/policy_loss": pg_loss.detach(),
        "losses/value_loss": vf_loss.detach(),
    }
    for k, v in _tensor_stats(values.detach(), mask, n).items():
        stats[f"values/{k}"] = v
    stats["values/values_error"] = torch.sum(((values.detach() - returns) * mask) ** 2) / n
    stats["values/clipfrac"] = vf_clipfrac
    for name, x in (("old_values", old_values), ("returns", returns)):
        for k, v in _tensor_stats(x, mask, n).items():
            stats[f"{name}/{k}"] = v
    stats["policy/approx_kl"] = approx_kl
    stats["policy/clipfrac"] = pg_clipfrac
    stats["ratio"] = (ratio.detach() * mask).sum() / n
    stats["padding_percentage"] = 1 - n / mask.numel()
    return loss, stats


def _inputs(B=4, R=9):
    g = torch.Generator().manual_seed(3)
    old_logprobs = -2 * torch.rand(B, R, generator=g)
    t = dict(
        logprobs=(old_logprobs + 0.4 * torch.randn(B, R, generator=g)).requires_grad_(True),
        values=torch.randn(B, R, generator=g).requires_grad_(True),
        old_logprobs=old_logprobs,
        old_values=torch.randn(B, R, generator=g),
        advantages=torch.randn(B, R, generator=g),
        returns=torch.randn(B, R, generator=g),
    )
    lengths = torch.tensor([R, 5, 1, 7])[:B]
    t["mask"] = (torch.arange(R)[None, :] < lengths[:, None]).long()
    return t


def _check_matches_expected(cfg):
    t = _inputs()
    loss, stats = cfg.loss(**t)
    dlp, dv = torch.autograd.grad(loss, [t["logprobs"], t["values"]])
    t2 = _inputs()
    eloss, estats = expected_loss(cfg, **t2)
    edlp, edv = torch.autograd.grad(eloss, [t2["logprobs"], t2["values"]])
    assert list(stats) == EXPECTED_KEYS == list(estats) == list(ops.PPO_LOSS_STAT_KEYS)
    assert torch.equal(loss, eloss)
    for k in EXPECTED_KEYS:
        assert torch.equal(stats[k], estats[k]), k
    assert torch.equal(dlp, edlp) and torch.equal(dv, edv)


def test_cpu_loss_is_the_plain_torch_loss(monkeypatch):
    # extension path unavailable
    monkeypatch.setattr(ops, "_EXT", None)
    monkeypatch.setattr(ops, "_EXT_TRIED", True)
    _check_matches_expected(PPOConfig(name="PPOConfig", cliprange=0.2, cliprange_value=0.3, vf_coef=0.8))


def test_switch_keeps_the_plain_torch_loss(monkeypatch):
    monkeypatch.setenv("TRLX_AMD_NO_FUSED_PPO_LOSS", "1")
    _check_matches_expected(PPOConfig(name="PPOConfig"))


def _fake_gpu_tensor(dtype=torch.float32, shape=(4, 9)):
    return types.SimpleNamespace(
        is_cuda=True, dtype=dtype, shape=torch.Size(shape), device=torch.device("cuda", 0),
        requires_grad=False, dim=lambda: len(shape), numel=lambda: shape[0] * shape[1])


def test_switch_turns_the_fused_gate_off(monkeypatch):
    """The gate itself, on stand-ins for GPU tensors (no GPU needed)."""
    monkeypatch.setattr(ops, "_require_ext", lambda name: object())
    monkeypatch.delenv("TRLX_AMD_NO_FUSED_PPO_LOSS", raising=False)
    floats = [_fake_gpu_tensor() for _ in range(6)]
    mask = _fake_gpu_tensor(torch.int64)
    assert ops.ppo_loss_fusable(*floats, mask)
    assert not ops.ppo_loss_fusable(*floats, _fake_gpu_tensor(torch.bool))
    assert not ops.ppo_loss_fusable(_fake_gpu_tensor(torch.bfloat16), *floats[1:], mask)
    monkeypatch.setenv("TRLX_AMD_NO_FUSED_PPO_LOSS", "1")
    assert not ops.ppo_loss_fusable(*floats, mask)


def test_cpu_inputs_never_take_the_fused_gate():
    t = _inputs()
    assert not ops.ppo_loss_fusable(*(t[k].detach() for k in (
        "logprobs", "values", "old_logprobs", "old_values", "advantages", "returns")), t["mask"])
