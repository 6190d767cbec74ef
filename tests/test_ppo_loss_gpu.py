"""Fused PPO loss kernel (csrc/ppo_loss.hip, ops.ppo_loss) against the eager
loss evaluated in fp64 on the same inputs.

Tolerance: for every output, |fused - fp64| <= 4 * |eager_fp32 - fp64| plus a
floor of 16 * 2^-24 * sum|terms| for the reductions (a different but equally
valid summation order) and of 4 ulp for the gradient elements.  min, max, the
two clip fractions and padding_percentage equal the eager fp32 result bit for
bit; min, max and the clip fractions also equal the fp64 result rounded to
fp32 (a single correctly rounded division of two integers-as-floats rounds the
same either way; padding_percentage is several fp32 roundings, 1 - n * fl(1 /
numel) as ATen divides by a host scalar, so its fp64 value may differ in the
last bits and is held to the tolerance).

The std floor follows from the floor on the variance: std = sqrt(var), so a
16 eps relative slack on var is 8 eps relative on std.

Inputs use cliprange_value = 0.25 (dyadic) so that the clip bounds of the
exact-tie element are the same numbers in fp32 and in fp64.
"""

import pytest
import torch

from trlx_amd import ops
from trlx_amd.models.modeling_ppo import PPOConfig

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
DEV = "cuda:0"
METHOD = PPOConfig(name="PPOConfig", cliprange=0.2, cliprange_value=0.25, vf_coef=0.7)

SHAPES = [(1, 1), (2, 3), (3, 70), (5, 411), (32, 40)]
# right-padded response masks with n >= 1: a [1, 1] input has only "ones"
CASES = [(s, m) for s in SHAPES for m in ("ones", "ragged", "zero_row") if s != (1, 1) or m == "ones"]
# enough masked-in elements in row 0 for every branch region (needs >= 18 + 2 specials)
COVERED = [(s, m) for s, m in CASES if s[1] >= 40]

FLOAT_NAMES = ("logprobs", "values", "old_logprobs", "old_values", "advantages", "returns")
EXACT_KEYS = ("values/min", "values/max", "old_values/min", "old_values/max", "returns/min",
              "returns/max", "values/clipfrac", "policy/clipfrac", "padding_percentage")
EXACT_VS_FP64 = tuple(k for k in EXACT_KEYS if k != "padding_percentage")


def make_inputs(shape, mask_kind, seed=0):
    """CPU fp32 inputs + int64 mask.  Element k (flat index) cycles through the
    ratio regions (k % 3), the advantage signs ((k // 3) % 2) and the value
    regions ((k // 6) % 3), so 18 consecutive masked-in elements cover every
    combination; row 0 is never padded."""
    B, R = shape
    g = torch.Generator().manual_seed(seed + 1000 * B + R)
    k = torch.arange(B * R).view(B, R)
    u = torch.rand(B, R, generator=g)
    old_logprobs = -3.0 * torch.rand(B, R, generator=g) - 0.01
    delta = torch.tensor([-0.5, 0.03, 0.5])[k % 3] * (1 + 0.1 * u)
    logprobs = old_logprobs + delta
    sign = torch.tensor([1.0, -1.0])[(k // 3) % 2]
    advantages = sign * (0.1 + torch.randn(B, R, generator=g).abs())
    old_values = torch.randn(B, R, generator=g)
    values = old_values + torch.tensor([-0.5, 0.05, 0.5])[(k // 6) % 3] * (1 + 0.1 * torch.rand(B, R, generator=g))
    returns = old_values + 0.5 * torch.randn(B, R, generator=g)
    if R >= 40:
        # specials in row 0, past the first 18 elements
        advantages[0, 20] = 0.0
        # (values - returns)^2 == (values_clipped - returns)^2 with values != values_clipped:
        # old 1.0 -> upper bound 1.25; values 1.75 clips to 1.25; returns 1.5 is midway
        old_values[0, 21], values[0, 21], returns[0, 21] = 1.0, 1.75, 1.5

    mask = torch.ones(B, R, dtype=torch.int64)
    if mask_kind in ("ragged", "zero_row"):
        lengths = torch.randint(1, R + 1, (B,), generator=g)
        lengths[0] = R
        mask = (torch.arange(R)[None, :] < lengths[:, None]).long()
    if mask_kind == "zero_row":
        mask[-1] = 0
    assert int(mask.sum()) >= 1
    t = dict(logprobs=logprobs, values=values, old_logprobs=old_logprobs, old_values=old_values,
             advantages=advantages, returns=returns)
    return {k_: v.float().contiguous() for k_, v in t.items()}, mask


def run(loss_fn, inputs, mask, dtype=torch.float32):
    """-> (stats dict of python-free device tensors incl. 'loss', dlogprobs, dvalues)"""
    t = {k: v.to(DEV, dtype) for k, v in inputs.items()}
    t["logprobs"].requires_grad_(True)
    t["values"].requires_grad_(True)
    loss, stats = loss_fn(mask=mask.to(DEV), **t)
    dlp, dv = torch.autograd.grad(loss, [t["logprobs"], t["values"]])
    out = {k: v.detach() for k, v in stats.items()}
    out["loss"] = loss.detach()
    return out, dlp, dv


def fused(inputs, mask):
    dev = {k: v.to(DEV) for k, v in inputs.items()}
    assert ops.ppo_loss_fusable(*(dev[n] for n in FLOAT_NAMES), mask.to(DEV))
    return run(METHOD.loss, inputs, mask)


def floors(inputs, mask):
    """16 * 2^-24 * sum|terms| for every reduction, scaled as the statistic is."""
    d = {k: v.double() for k, v in inputs.items()}
    m = mask.double()
    n, N = m.sum(), m.numel()
    cv, cr = METHOD.cliprange_value, METHOD.cliprange
    vc = torch.clamp(d["values"], d["old_values"] - cv, d["old_values"] + cv)
    l = torch.max((d["values"] - d["returns"]) ** 2, (vc - d["returns"]) ** 2)
    lr = (d["logprobs"] - d["old_logprobs"]) * m
    ratio = torch.exp(lr)
    p = torch.max(-d["advantages"] * ratio, -d["advantages"] * torch.clamp(ratio, 1 - cr, 1 + cr))
    f = {
        "losses/policy_loss": (p * m).abs().sum() / n,
        "losses/value_loss": 0.5 * (l * m).abs().sum() / n,
        "values/values_error": (((d["values"] - d["returns"]) * m) ** 2).sum() / n,
        "policy/approx_kl": ((ratio - 1) - lr).abs().sum() / N,
        "ratio": (ratio * m).sum() / n,
        "padding_percentage": torch.tensor(1.0, dtype=torch.float64),
    }
    f["losses/total_loss"] = f["losses/policy_loss"] + METHOD.vf_coef * f["losses/value_loss"]
    f["loss"] = f["losses/total_loss"]
    denom = torch.clamp(n - 1, min=1)
    for name in ("values", "old_values", "returns"):
        x = d[name]
        mean = (x * m).sum() / n
        f[f"{name}/mean"] = (x * m).abs().sum() / n
        f[f"{name}/std"] = 0.5 * torch.sqrt((((x - mean) * m) ** 2).sum() / denom)
    return {k: 16 * EPS * float(v) for k, v in f.items()}


def ulp32(x64):
    """fp32 spacing at |x| (x in fp64): 2^(e - 24) with |x| = m * 2^e, m in [0.5, 1)."""
    _, e = torch.frexp(x64.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x64), e - 24)


_CACHE = {}


def case(shape, mask_kind):
    """inputs and the three evaluations, computed once per case and shared."""
    key = (shape, mask_kind)
    if key not in _CACHE:
        inputs, mask = make_inputs(shape, mask_kind)
        _CACHE[key] = dict(
            inputs=inputs, mask=mask,
            fused=fused(inputs, mask),
            eager=run(METHOD._loss_eager, inputs, mask),
            ref=run(METHOD._loss_eager, inputs, mask, torch.float64),
        )
    return _CACHE[key]


@pytest.mark.parametrize("shape,mask_kind", COVERED)
def test_inputs_cover_every_branch(shape, mask_kind):
    inputs, mask = make_inputs(shape, mask_kind)
    on = mask.bool()
    cr, cv = METHOD.cliprange, METHOD.cliprange_value
    ratio = torch.exp((inputs["logprobs"] - inputs["old_logprobs"]) * mask)
    adv = inputs["advantages"]
    for region in (ratio < 1 - cr, (ratio >= 1 - cr) & (ratio <= 1 + cr), ratio > 1 + cr):
        assert (region & on & (adv > 0)).any() and (region & on & (adv < 0)).any()
    v, ov, ret = inputs["values"], inputs["old_values"], inputs["returns"]
    assert ((v < ov - cv) & on).any() and ((v > ov + cv) & on).any()
    assert ((v >= ov - cv) & (v <= ov + cv) & on).any()
    assert ((adv == 0) & on).any()
    vc = torch.clamp(v, ov - cv, ov + cv)
    assert (((v - ret) ** 2 == (vc - ret) ** 2) & (v != vc) & on).any()


@pytest.mark.parametrize("shape,mask_kind", CASES)
def test_statistics_within_tolerance_of_fp64(shape, mask_kind):
    c = case(shape, mask_kind)
    (fs, _, _), (es, _, _), (rs, _, _) = c["fused"], c["eager"], c["ref"]
    assert list(fs)[:-1] == list(es)[:-1] == list(ops.PPO_LOSS_STAT_KEYS)
    fl = floors(c["inputs"], c["mask"])
    for k in fs:
        assert fs[k].dim() == 0 and fs[k].dtype == torch.float32 and fs[k].is_cuda
        if k in EXACT_VS_FP64:
            continue
        ref = float(rs[k])
        err, yard = abs(float(fs[k]) - ref), abs(float(es[k]) - ref)
        print(f"{shape} {mask_kind} {k}: fused err {err:.3e} eager err {yard:.3e} floor {fl[k]:.3e}")
        assert err <= 4 * yard + fl[k], (k, float(fs[k]), float(es[k]), ref)


@pytest.mark.parametrize("shape,mask_kind", CASES)
def test_exact_statistics(shape, mask_kind):
    c = case(shape, mask_kind)
    (fs, _, _), (es, _, _), (rs, _, _) = c["fused"], c["eager"], c["ref"]
    for k in EXACT_KEYS:
        assert torch.equal(fs[k], es[k].float()), (k, float(fs[k]), float(es[k]))
    for k in EXACT_VS_FP64:
        assert torch.equal(fs[k], rs[k].float()), (k, float(fs[k]), float(rs[k]))


@pytest.mark.parametrize("shape,mask_kind", CASES)
def test_gradients_within_tolerance_of_fp64(shape, mask_kind):
    c = case(shape, mask_kind)
    for name, f, e, r in zip(("dlogprobs", "dvalues"), c["fused"][1:], c["eager"][1:], c["ref"][1:]):
        assert f.shape == r.shape and f.dtype == torch.float32
        err = (f.double() - r).abs()
        bound = 4 * (e.double() - r).abs() + 4 * ulp32(r)
        worst = (err - bound).max()
        print(f"{shape} {mask_kind} {name}: max err {float(err.max()):.3e}, max (err - bound) {float(worst):.3e}, "
              f"elements differing from eager fp32: {int((f != e).sum())}")
        assert bool((err <= bound).all()), (name, float(worst))


def _bits(result):
    stats, dlp, dv = result
    return torch.stack([stats[k] for k in stats]), dlp, dv


@pytest.mark.parametrize("shape", [(3, 70), (32, 40)])
def test_strided_slices_equal_contiguous_bitwise(shape):
    c = case(shape, "ragged")
    B, R = shape
    wide = {}
    for k, v in c["inputs"].items():
        w = torch.full((B, R + 14), float("nan"))
        w[:, 7:7 + R] = v
        wide[k] = w.to(DEV)
    wmask = torch.zeros(B, R + 14, dtype=torch.int64)
    wmask[:, 7:7 + R] = c["mask"]
    wmask = wmask.to(DEV)
    wide["logprobs"].requires_grad_(True)
    wide["values"].requires_grad_(True)
    sl = {k: v[:, 7:7 + R] for k, v in wide.items()}
    assert not sl["logprobs"].is_contiguous()
    assert ops.ppo_loss_fusable(*(sl[n] for n in FLOAT_NAMES), wmask[:, 7:7 + R])
    loss, stats = METHOD.loss(mask=wmask[:, 7:7 + R], **sl)
    dlp, dv = torch.autograd.grad(loss, [wide["logprobs"], wide["values"]])
    ref_vec, ref_dlp, ref_dv = _bits(c["fused"])
    assert torch.equal(torch.stack(list(stats.values()) + [loss.detach()]), ref_vec)
    assert torch.equal(dlp[:, 7:7 + R], ref_dlp) and torch.equal(dv[:, 7:7 + R], ref_dv)
    # nothing leaks into the padding columns of the wide gradients
    assert float(dlp[:, :7].abs().sum() + dlp[:, 7 + R:].abs().sum()) == 0.0


@pytest.mark.parametrize("shape", [(5, 411), (32, 40)])
def test_two_calls_are_bit_identical(shape):
    c = case(shape, "ragged")
    again = fused(c["inputs"], c["mask"])
    for a, b in zip(_bits(c["fused"]), _bits(again)):
        assert torch.equal(a, b)


def test_graph_capture_replays_match_eager_calls_bitwise():
    shape = (32, 40)
    variants = [make_inputs(shape, "ragged", seed=s) for s in (1, 2, 3)]
    static = {k: v.to(DEV).clone() for k, v in variants[0][0].items()}
    smask = variants[0][1].to(DEV).clone()
    static["logprobs"].requires_grad_(True)
    static["values"].requires_grad_(True)

    def step():
        loss, stats = METHOD.loss(mask=smask, **static)
        dlp, dv = torch.autograd.grad(loss, [static["logprobs"], static["values"]])
        return loss, stats, dlp, dv

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, stats, dlp, dv = step()

    for inputs, mask in variants[1:]:
        with torch.no_grad():
            for k, v in inputs.items():
                static[k].copy_(v)
            smask.copy_(mask)
        graph.replay()
        torch.cuda.synchronize()
        ref_vec, ref_dlp, ref_dv = _bits(fused(inputs, mask))
        assert torch.equal(torch.stack(list(stats.values()) + [loss.detach()]), ref_vec)
        assert torch.equal(dlp, ref_dlp) and torch.equal(dv, ref_dv)


def test_switch_restores_the_eager_body(monkeypatch):
    c = case((2, 3), "ones")
    monkeypatch.setenv("TRLX_AMD_NO_FUSED_PPO_LOSS", "1")
    dev = {k: v.to(DEV) for k, v in c["inputs"].items()}
    assert not ops.ppo_loss_fusable(*(dev[n] for n in FLOAT_NAMES), c["mask"].to(DEV))
    stats, dlp, dv = run(METHOD.loss, c["inputs"], c["mask"])
    for a, b in zip(_bits((stats, dlp, dv)), _bits(c["eager"])):
        assert torch.equal(a, b)
