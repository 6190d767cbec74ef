"""ops.gated_act on the CPU is the eager expression, bit for bit, and the
opt-in switch changes nothing there."""
import pytest
import torch
import torch.nn.functional as F
from conftest import tiny_config

from trlx_amd import ops
from trlx_amd.models.nn.seq2seq import Seq2SeqConfig, T5FFN
from trlx_amd.models.nn.transformer import MLP

ACTS = {"silu": F.silu, "gelu_new": lambda x: F.gelu(x, approximate="tanh"), "gelu": F.gelu}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("act", list(ACTS))
def test_cpu_is_the_eager_expression(act, fused, dtype):
    torch.manual_seed(0)
    I = 24
    a, b = (torch.randn(2, 3, 2 * I if fused else I).to(dtype).requires_grad_() for _ in range(2))
    dh = torch.randn(2, 3, I).to(dtype)
    if fused:
        got, want, inputs = ops.gated_act(a, act=act), ACTS[act](a[..., :I]) * a[..., I:], (a,)
    else:
        got, want, inputs = ops.gated_act(a, b, act=act), ACTS[act](a) * b, (a, b)
    assert got.shape == (2, 3, I) and torch.equal(got, want)
    for x, y in zip(torch.autograd.grad(got, inputs, dh), torch.autograd.grad(want, inputs, dh)):
        assert torch.equal(x, y)


def test_switch_changes_nothing_on_cpu(monkeypatch):
    torch.manual_seed(0)
    cfg = tiny_config(hidden_size=32, intermediate_size=40, activation="silu", swiglu=True,
                      mlp_bias=False, arch_name="llama")
    t5 = Seq2SeqConfig(d_model=32, d_ff=40, feed_forward_proj="gated-gelu")
    for module in (MLP(cfg), T5FFN(t5)):
        x = torch.randn(2, 5, 32, requires_grad=True)
        results = []
        for flag in (None, "1"):
            monkeypatch.delenv("TRLX_AMD_FUSED_GATED_ACT", raising=False)
            if flag:
                monkeypatch.setenv("TRLX_AMD_FUSED_GATED_ACT", flag)
            assert ops.gated_act_enabled() == bool(flag)
            out = module(x)
            results.append((out, *torch.autograd.grad(out.sum(), [x, *module.parameters()])))
        for a, b in zip(*results):
            assert torch.equal(a, b)
