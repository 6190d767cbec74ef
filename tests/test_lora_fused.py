"""ops.lora_linear on the CPU is LoRALinear's eager line, and the opt-in switch
routes LoRALinear.forward through it only when the call is fusable."""
import pytest
import torch
import torch.nn as nn

from trlx_amd import ops
from trlx_amd.models.lora import LoRALinear, adapters_disabled


def make_layer(bias=True, dropout=0.0):
    torch.manual_seed(0)
    layer = LoRALinear(nn.Linear(24, 40, bias=bias), r=8, alpha=4.0, dropout=dropout)
    nn.init.normal_(layer.lora_B)
    return layer


@pytest.mark.parametrize("bias", [True, False])
def test_cpu_is_the_eager_line(bias):
    layer = make_layer(bias)
    x = torch.randn(2, 5, 24, requires_grad=True)
    dy = torch.randn(2, 5, 40)
    leaves = (x, layer.lora_A, layer.lora_B)
    want = layer(x)
    got = ops.lora_linear(x, layer.base.weight, layer.base.bias, layer.lora_A, layer.lora_B,
                          layer.scaling)
    assert torch.equal(got, want)
    for a, b in zip(torch.autograd.grad(got, leaves, dy), torch.autograd.grad(want, leaves, dy)):
        assert torch.equal(a, b)


def test_switch_routes_the_module_through_the_op(monkeypatch):
    layer = make_layer(dropout=0.5)
    x = torch.randn(3, 24)
    calls = []

    def spy(x, weight, bias, lora_A, lora_B, scaling, x_lora=None):
        calls.append(x_lora)
        return ops.reference.lora_linear(x, weight, bias, lora_A, lora_B, scaling, x_lora)

    monkeypatch.setattr(ops, "lora_linear", spy)
    monkeypatch.setattr(ops, "lora_fusable", lambda x, base, r: True)
    layer(x)
    assert not calls, "the switch is opt-in"
    monkeypatch.setenv("TRLX_AMD_FUSED_LORA", "1")
    assert ops.lora_enabled()
    layer(x)
    assert len(calls) == 1 and calls[0] is not None, "the dropout output goes in as x_lora"
    layer.eval()
    want = layer.base(x) + layer.scaling * (x @ layer.lora_A.t()) @ layer.lora_B.t()
    torch.testing.assert_close(layer(x), want)
    with adapters_disabled(layer):
        assert torch.equal(layer(x), layer.base(x))
    assert len(calls) == 2, "adapters_disabled bypasses the op"


def test_not_fusable_on_the_cpu(monkeypatch):
    monkeypatch.setenv("TRLX_AMD_FUSED_LORA", "1")
    layer = make_layer()
    assert not ops.lora_fusable(torch.randn(3, 24), layer.base, layer.r)
