"""CPU tests of the T5 per-token generation step: the two decode-attention
reference ops against dense fp32 math, ``Seq2SeqTransformer.decode_step`` over a
preallocated state against the ``decode(..., past=)`` loop, the head-dim list
mirror, and the routing that keeps CPU and small-head models on the old loop."""

import re
from pathlib import Path

import pytest
import torch

from trlx_amd import ops
from trlx_amd.models.nn.seq2seq import Seq2SeqConfig, Seq2SeqTransformer
from trlx_amd.ops import reference

B, H, S, D = 3, 2, 12, 16


def _dense_self(q, kc, vc, pos, table, bidirectional_bias_of):
    """Dense fp32 math for one query at ``pos`` over keys 0..pos: an explicit
    [H, pos+1] bias row from the model-side bucket function, no Toeplitz vector."""
    scores = torch.einsum("bhd,bhsd->bhs", q.float(), kc[:, :, : pos + 1].float())
    if table is not None:
        scores = scores + bidirectional_bias_of(pos)[None]
    probs = torch.softmax(scores, dim=-1)
    return torch.einsum("bhs,bhsd->bhd", probs, vc[:, :, : pos + 1].float()).unsqueeze(2)


@pytest.mark.parametrize("pos", [0, 5, S - 1])
@pytest.mark.parametrize("bias", [False, True])
def test_self_step_reference_matches_dense(pos, bias):
    g = torch.Generator().manual_seed(pos * 2 + bias)
    q, kn, vn = (torch.randn(B, H, D, generator=g) for _ in range(3))
    kc, vc = (torch.randn(B, H, S, D, generator=g) for _ in range(2))
    kc0, vc0 = kc.clone(), vc.clone()
    table = torch.randn(8, H, generator=g)  # [num_buckets, H]
    vec = zero = None
    if bias:
        vec, zero = ops.t5_rel_bias(table, 1, 1, S - 1, False, 8, 20)
        assert vec.shape == (H, S) and zero == S - 1

    def bias_row(p):
        rel = torch.arange(p + 1) - p
        buckets = reference.relative_position_bucket(rel, False, 8, 20)
        return table[buckets].t()  # [H, p+1]

    out = ops.seq2seq_decode_attention(q, kn, vn, kc, vc, torch.tensor([pos]), rel_bias=vec,
                                       bias_zero=zero or 0, scale=1.0)
    assert out.shape == (B, H, 1, D)
    # the append happened in place, at row pos only
    assert torch.equal(kc[:, :, pos], kn) and torch.equal(vc[:, :, pos], vn)
    keep = torch.arange(S) != pos
    assert torch.equal(kc[:, :, keep], kc0[:, :, keep])
    assert torch.equal(vc[:, :, keep], vc0[:, :, keep])
    want = _dense_self(q, kc, vc, pos, table if bias else None, bias_row)
    assert torch.allclose(out, want, atol=1e-5), (out - want).abs().max()


def test_self_step_reference_scale_and_out_of_range_index():
    g = torch.Generator().manual_seed(0)
    q, kn, vn = (torch.randn(B, H, D, generator=g) for _ in range(3))
    kc, vc = (torch.randn(B, H, S, D, generator=g) for _ in range(2))
    out = ops.seq2seq_decode_attention(q, kn, vn, kc, vc, torch.tensor([4]), scale=0.25)
    want = _dense_self(q * 0.25, kc, vc, 4, None, None)
    assert torch.allclose(out, want, atol=1e-5)
    kc0, vc0 = kc.clone(), vc.clone()
    for bad in (-1, S):  # the kernel's guard: nothing written, zeros returned
        out = ops.seq2seq_decode_attention(q, kn, vn, kc, vc, torch.tensor([bad]))
        assert torch.equal(out, torch.zeros(B, H, 1, D))
        assert torch.equal(kc, kc0) and torch.equal(vc, vc0)


def _masks(Tk):
    none = None
    right = torch.ones(B, Tk, dtype=torch.uint8)
    right[1, Tk // 2:] = 0
    left = torch.ones(B, Tk, dtype=torch.uint8)
    left[0, : Tk // 3] = 0
    holes = (torch.arange(Tk)[None, :] % 3 != 1).to(torch.uint8).repeat(B, 1)
    holes[2, 0] = 1
    dead = torch.ones(B, Tk, dtype=torch.uint8)
    dead[1] = 0  # one all-masked row
    return {"none": none, "right": right, "left": left, "holes": holes, "dead": dead}


@pytest.mark.parametrize("kind", ["none", "right", "left", "holes", "dead"])
def test_cross_step_reference_matches_dense(kind):
    Tk = 11
    g = torch.Generator().manual_seed(3)
    q = torch.randn(B, H, 1, D, generator=g)
    k, v = (torch.randn(B, H, Tk, D, generator=g) for _ in range(2))
    mask = _masks(Tk)[kind]
    if mask is not None:  # whatever lies behind the mask must not leak
        hidden = (mask == 0)[:, None, :, None].expand_as(k)
        k = torch.where(hidden, torch.full_like(k, float("nan")), k)
        v = torch.where(hidden, torch.full_like(v, float("inf")), v)
    out = ops.seq2seq_cross_decode_attention(q, k, v, key_mask=mask, scale=0.5)
    assert out.shape == (B, H, 1, D) and torch.isfinite(out).all()
    for b in range(B):  # dense math over the visible keys of each row
        vis = torch.ones(Tk, dtype=torch.bool) if mask is None else mask[b] != 0
        if not vis.any():
            assert torch.equal(out[b], torch.zeros(H, 1, D))
            continue
        scores = torch.einsum("hqd,hsd->hqs", q[b] * 0.5, k[b][:, vis])
        want = torch.einsum("hqs,hsd->hqd", torch.softmax(scores, -1), v[b][:, vis])
        assert torch.allclose(out[b], want, atol=1e-5), (kind, b)


def _tiny(d_kv=16):
    torch.manual_seed(0)
    cfg = Seq2SeqConfig(vocab_size=120, d_model=64, d_kv=d_kv, num_heads=4, d_ff=128,
                        num_layers=2, decoder_start_token_id=2, pad_token_id=2, eos_token_id=1)
    m = Seq2SeqTransformer(cfg).eval()
    m.shared.weight.data.normal_(0.0, 1.0)
    m.decoder_blocks[0].self_attn.relative_attention_bias.weight.data.normal_(0.0, 1.0)
    return m, cfg


def test_decode_step_matches_past_loop():
    m, cfg = _tiny()
    ids = torch.randint(3, cfg.vocab_size, (3, 9))
    mask = torch.ones_like(ids)
    mask[0, :3] = 0  # left pad
    mask[1, 6:] = 0  # right pad
    steps = 7
    with torch.no_grad():
        enc = m.encode(ids, mask)
        # capacity beyond the prompt and beyond the steps taken
        state = m.new_decode_state(3, enc_capacity=12, max_positions=10)
        state.begin(m, enc, mask)
        cur_old = cur_new = torch.full((3, 1), cfg.decoder_start_token_id)
        past = None
        for t in range(steps):
            h_old, past, _ = m.decode(cur_old, enc, mask, past=past)
            h_new = m.decode_step(cur_new, state)
            assert int(state.cache_idx) == t  # the step itself does not advance
            state.cache_idx += 1
            assert h_new.shape == h_old.shape
            assert torch.allclose(h_new, h_old, atol=1e-4), (t, (h_new - h_old).abs().max())
            cur_old = m.project(h_old)[:, 0].argmax(-1, keepdim=True)
            cur_new = m.project(h_new)[:, 0].argmax(-1, keepdim=True)
            assert torch.equal(cur_old, cur_new), t
        # a second, shorter prompt reuses the same buffers
        ids2, mask2 = ids[:, :5].contiguous(), torch.ones(3, 5, dtype=torch.long)
        enc2 = m.encode(ids2, mask2)
        ptrs = [t.data_ptr() for t in state.cross_k + state.self_k] + [state.rel_bias.data_ptr()]
        state.begin(m, enc2, mask2)
        assert ptrs == [t.data_ptr() for t in state.cross_k + state.self_k] + [
            state.rel_bias.data_ptr()]
        assert int(state.cache_idx) == 0 and int(state.key_mask[:, 5:].sum()) == 0
        start = torch.full((3, 1), cfg.decoder_start_token_id)
        h_old, _, _ = m.decode(start, enc2, mask2)
        assert torch.allclose(m.decode_step(start, state), h_old, atol=1e-4)


def test_decode_state_bias_follows_the_table():
    m, cfg = _tiny()
    ids = torch.randint(3, cfg.vocab_size, (2, 4))
    with torch.no_grad():
        enc = m.encode(ids)
        state = m.new_decode_state(2, 4, 6)
        state.begin(m, enc)
        before = state.rel_bias.clone()
        m.decoder_blocks[0].self_attn.relative_attention_bias.weight.add_(1.0)
        state.begin(m, enc)
    assert torch.allclose(state.rel_bias, before + 1.0)


def test_decode_head_dims_mirror_the_header():
    header = Path(ops.__file__).parent.parent / "csrc" / "attn_host.h"
    found = re.search(r"HeadDims<([\d,\s]+)>\s*kSeq2SeqDecodeHeadDims", header.read_text())
    assert found, "kSeq2SeqDecodeHeadDims not found in attn_host.h"
    dims = tuple(int(x) for x in found.group(1).split(","))
    assert dims == ops.SEQ2SEQ_DECODE_HEAD_DIMS == (64, 128)


@pytest.mark.parametrize("d_kv", [16, 64])
def test_generate_on_cpu_keeps_the_old_loop(d_kv, monkeypatch):
    m, cfg = _tiny(d_kv)

    def boom(*a, **k):
        raise AssertionError("decode_step must not run here")

    monkeypatch.setattr(m, "decode_step", boom)
    ids = torch.randint(3, cfg.vocab_size, (2, 5))
    out = m.generate(ids, max_new_tokens=4, do_sample=False)
    assert out.shape[0] == 2 and 2 <= out.shape[1] <= 5
    assert (out[:, 0] == cfg.decoder_start_token_id).all()
    assert getattr(m, "_decode_engine", None) is None
