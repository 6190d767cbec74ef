"""Head-dim gating has one source of truth (ops.FLASH_HEAD_DIMS /
ops.DECODE_HEAD_DIMS) and the two largest causal presets are inside it."""

import pytest

from trlx_amd import ops
from trlx_amd.models.nn.config import preset


@pytest.mark.parametrize("name,head_dim", [("gptj-6b", 256), ("gpt-neox-20b", 96)])
def test_large_presets_have_flash_and_decode_head_dims(name, head_dim):
    cfg = preset(name)
    assert cfg.head_dim == head_dim
    assert cfg.head_dim in ops.FLASH_HEAD_DIMS
    assert cfg.head_dim in ops.DECODE_HEAD_DIMS


def test_head_dim_sets():
    assert ops.FLASH_HEAD_DIMS == (64, 96, 128, 256)
    assert ops.DECODE_HEAD_DIMS == (32, 64, 96, 128, 256)
    # every flash head dim can also decode (generate() after a flash prefill)
    assert set(ops.FLASH_HEAD_DIMS) <= set(ops.DECODE_HEAD_DIMS)


def test_flash_defaults_follow_the_measured_ab(monkeypatch):
    monkeypatch.delenv("TRLX_AMD_NO_FLASH_PREFILL", raising=False)
    monkeypatch.delenv("TRLX_AMD_NO_FLASH_TRAIN", raising=False)
    # unchanged head dims: both directions on
    for d in (64, 128):
        assert ops.flash_enabled(d, train=False) and ops.flash_enabled(d, train=True)
    # D=96 wins the no_grad forward only; D=256 neither (profiles/headdim_notes.md)
    assert ops.flash_enabled(96, train=False) and not ops.flash_enabled(96, train=True)
    assert not ops.flash_enabled(256, train=False) and not ops.flash_enabled(256, train=True)
    assert not ops.flash_enabled(80, train=False)  # no such instantiation


def test_flash_switches(monkeypatch):
    dims = ops.FLASH_HEAD_DIMS
    # 0 turns a direction on for every instantiated head dim, and for no other
    monkeypatch.setenv("TRLX_AMD_NO_FLASH_PREFILL", "0")
    monkeypatch.setenv("TRLX_AMD_NO_FLASH_TRAIN", "0")
    assert all(ops.flash_enabled(d, train=False) and ops.flash_enabled(d, train=True) for d in dims)
    assert not ops.flash_enabled(80, train=False) and not ops.flash_enabled(80, train=True)
    # the escape hatches: NO_FLASH_TRAIN=1 stops training only, NO_FLASH_PREFILL=1 both
    monkeypatch.setenv("TRLX_AMD_NO_FLASH_TRAIN", "1")
    assert all(ops.flash_enabled(d, train=False) and not ops.flash_enabled(d, train=True) for d in dims)
    monkeypatch.setenv("TRLX_AMD_NO_FLASH_TRAIN", "0")
    monkeypatch.setenv("TRLX_AMD_NO_FLASH_PREFILL", "1")
    assert not any(ops.flash_enabled(d, train=False) or ops.flash_enabled(d, train=True) for d in dims)
