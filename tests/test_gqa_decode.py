"""Grouped-query decode attention: the public interface on CPU (the kernel
itself is checked in test_gqa_decode_gpu.py)."""
import pytest
import torch

from trlx_amd import ops


@pytest.mark.parametrize("alibi", [False, True])
def test_grouped_arguments_run_the_reference_on_cpu(alibi):
    torch.manual_seed(0)
    B, Hq, Hkv, S, D = 3, 8, 2, 24, 64
    q = torch.randn(B, Hq, 1, D)
    k, v = torch.randn(B, Hkv, S, D), torch.randn(B, Hkv, S, D)
    lens = torch.tensor([1, 24, 9], dtype=torch.int32)
    starts = torch.tensor([0, 3, 4], dtype=torch.int32)
    slopes = torch.linspace(0.5, 0.01, Hq) if alibi else None
    want = ops.attention_decode(q, k, v, lens, D ** -0.5, seq_starts=starts, alibi_slopes=slopes)
    for grouped in (None, False, True):
        got = ops.attention_decode(q, k, v, lens, D ** -0.5, seq_starts=starts,
                                   alibi_slopes=slopes, grouped=grouped, num_splits=3)
        assert torch.equal(got, want)


@pytest.mark.parametrize("env,head_dim,group", [(None, 128, 8), ("0", 128, 8), ("1", 128, 1),
                                                ("1", 96, 4)])
def test_gate_is_off(monkeypatch, env, head_dim, group):
    if env is None:
        monkeypatch.delenv("TRLX_AMD_GQA_DECODE", raising=False)
    else:
        monkeypatch.setenv("TRLX_AMD_GQA_DECODE", env)
    assert ops.gqa_decode_enabled(head_dim, group) is False


def test_gate_follows_the_extension(monkeypatch):
    monkeypatch.setenv("TRLX_AMD_GQA_DECODE", "1")
    assert ops.GQA_DECODE_HEAD_DIMS == (64, 128)
    for head_dim in ops.GQA_DECODE_HEAD_DIMS:
        assert ops.gqa_decode_enabled(head_dim, 2) is ops.extension_available()
