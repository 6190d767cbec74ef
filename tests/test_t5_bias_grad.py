"""``ops.seq2seq_attention(..., bias_grad=True)`` on the CPU: the relative-
position bias vector is a differentiable input, and the default still rejects
a bias that requires grad."""

import pytest
import torch

from trlx_amd import ops
from trlx_amd.ops import reference


@pytest.mark.parametrize("causal", [False, True])
def test_bias_grad_is_the_reference_gradient_and_stays_opt_in(causal):
    torch.manual_seed(0)
    B, H, T, D = 2, 3, 9, 16
    q, k, v = (torch.randn(B, H, T, D) for _ in range(3))
    dout = torch.randn(B, H, T, D)
    key_mask = torch.ones(B, T, dtype=torch.uint8)
    key_mask[1, 5:] = 0
    vec0, zero = ops.t5_rel_bias(torch.randn(32, H) * 2.0, T, T, 0, not causal)

    want = vec0.clone().requires_grad_()
    reference.seq2seq_attention(q, k, v, want, zero, key_mask, causal).backward(dout)
    assert want.grad.abs().max() > 0.1

    vec = vec0.clone().requires_grad_()
    ops.seq2seq_attention(q, k, v, vec, zero, key_mask, causal, bias_grad=True).backward(dout)
    torch.testing.assert_close(vec.grad, want.grad, atol=1e-6, rtol=1e-6)

    with pytest.raises(RuntimeError, match="rel_bias"):
        ops.seq2seq_attention(q, k, v, vec, zero, key_mask, causal)
