"""The fp8 KV-cache format (ops/reference.py) and its CPU paths."""
import pytest
import torch

from trlx_amd import ops
from trlx_amd.ops import reference


def _rows(D=64):
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(2, 3, 11, D, generator=g) * 3.0).bfloat16()
    x[0, 1, 4] = 0.0                      # an all-zero row
    x[1, 2, 7, 5], x[1, 2, 7, 9] = 32.0, -32.0  # +-absmax
    return x


def test_roundtrip_within_half_a_step():
    x = _rows()
    codes, scale = reference.kv_quantize_fp8(x)
    assert codes.dtype == torch.uint8 and codes.shape == x.shape and scale.shape == x.shape[:-1]
    back = reference.kv_dequantize_fp8(codes, scale)
    amax = x.float().abs().amax(-1, keepdim=True)
    # e4m3's widest step below 448 is 32: half of it, relative to absmax, is 16/448
    assert ((back - x.float()).abs() <= amax * (16.0 / 448.0) * (1 + 1e-6)).all()
    assert scale[0, 1, 4] == 0 and codes[0, 1, 4].count_nonzero() == 0
    assert codes[1, 2, 7, 5] == 0x7E and codes[1, 2, 7, 9] == 0xFE  # +-448


@pytest.mark.parametrize("amax", [448.0, 1.0, 3.0e-3, 7.0, 1.0e30])
def test_absmax_never_encodes_nan(amax):
    x = torch.zeros(1, 64).bfloat16()
    x[0, 0], x[0, 1], x[0, 2] = amax, -amax, amax / 2
    codes, _ = reference.kv_quantize_fp8(x)
    assert codes[0, 0] == 0x7E and codes[0, 1] == 0xFE  # +-448, one below the NaN codes
    assert not ((codes & 0x7F) == 0x7F).any()


@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (6, 2)])
def test_attention_decode_fp8_cpu_equals_bf16_reference_on_dequantized_cache(Hq, Hkv):
    g = torch.Generator().manual_seed(Hq)
    B, S, D = 2, 13, 64
    q = torch.randn(B, Hq, 1, D, generator=g).bfloat16()
    k8, v8 = (torch.zeros(B, Hkv, S, D, dtype=torch.uint8) for _ in range(2))
    ks, vs = (torch.zeros(B, Hkv, S) for _ in range(2))
    k, v = (torch.randn(B, Hkv, 9, D, generator=g).bfloat16() for _ in range(2))
    ops.kv_store_fp8(k, v, k8, ks, v8, vs, torch.tensor([2, 4]))
    assert k8[0, :, :2].count_nonzero() == 0 and k8[1, :, :4].count_nonzero() == 0
    assert torch.equal(k8[1, :, 4:13], reference.kv_quantize_fp8(k[1])[0])
    lens = torch.tensor([11, 13], dtype=torch.int32)
    starts = torch.tensor([2, 4], dtype=torch.int32)
    out = ops.attention_decode(q, k8, v8, lens, 0.125, seq_starts=starts, k_scale=ks, v_scale=vs)
    ref = ops.attention_decode(q, reference.kv_dequantize_fp8(k8, ks),
                               reference.kv_dequantize_fp8(v8, vs), lens, 0.125, seq_starts=starts)
    assert torch.equal(out, ref)
    with pytest.raises(ValueError, match="k_scale and v_scale"):
        ops.attention_decode(q, k8, v8, lens, 0.125)


def test_kv_fp8_is_opt_in(monkeypatch):
    monkeypatch.delenv("TRLX_AMD_FP8_KV", raising=False)
    assert ops.KV_FP8_HEAD_DIMS == (64, 128)
    assert not ops.kv_fp8_enabled(64)
    monkeypatch.setenv("TRLX_AMD_FP8_KV", "1")
    assert not ops.kv_fp8_enabled(96)
