"""attn_decode_gqa.hip against fp64 attention on the same bf16 inputs."""
import functools

import pytest
import torch

from trlx_amd import ops

pytestmark = pytest.mark.gpu

B, S = 5, 160
SEQ_LENS = [1, 17, 33, 160, 40]
SEQ_STARTS = [0, 5, 16, 31, 40]  # the last row has no visible key


def _reference(q, k, v, lens, starts, scale, slopes):
    """fp64 masked softmax attention; a row with no visible key gives zeros."""
    G = q.shape[1] // k.shape[1]
    kf, vf = (t.double().repeat_interleave(G, dim=1) for t in (k, v))
    pos = torch.arange(k.shape[2], device=q.device).view(1, 1, 1, -1)
    lo, hi = starts.view(-1, 1, 1, 1), lens.view(-1, 1, 1, 1)
    s = q.double() @ kf.transpose(-1, -2) * scale
    if slopes is not None:
        s = s + slopes.double().view(1, -1, 1, 1) * (pos - lo)
    p = torch.softmax(s.masked_fill((pos < lo) | (pos >= hi), float("-inf")), dim=-1)
    return p.nan_to_num(0.0) @ vf


@functools.lru_cache(maxsize=None)
def _case(D, Hq, Hkv, alibi, S=S):
    g = torch.Generator().manual_seed(D + 7 * Hq + Hkv)
    q = torch.randn(B, Hq, 1, D, generator=g).bfloat16().cuda()
    k = torch.randn(B, Hkv, S, D, generator=g).bfloat16().cuda()
    v = torch.randn(B, Hkv, S, D, generator=g).bfloat16().cuda()
    lens = torch.tensor(SEQ_LENS, dtype=torch.int32, device="cuda")
    starts = torch.tensor(SEQ_STARTS, dtype=torch.int32, device="cuda")
    for b, n in enumerate(SEQ_LENS):  # a masked key that leaks shows up
        k[b, :, n:] = 1e4
        v[b, :, n:] = 1e4
    slopes = None
    if alibi:
        slopes = torch.pow(2.0, -8.0 * torch.arange(1, Hq + 1) / Hq).float().cuda()
    ref = _reference(q, k, v, lens, starts, D ** -0.5, slopes)
    return q, k, v, lens, starts, slopes, ref


@pytest.mark.parametrize("alibi", [False, True])
@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("Hq,Hkv", [(4, 2), (16, 2), (16, 1), (24, 1)])
@pytest.mark.parametrize("D", [64, 128])
def test_gqa_decode_matches_fp64(D, Hq, Hkv, num_splits, alibi):
    q, k, v, lens, starts, slopes, ref = _case(D, Hq, Hkv, alibi)
    out = ops.attention_decode(q, k, v, lens, D ** -0.5, seq_starts=starts, alibi_slopes=slopes,
                               grouped=True, num_splits=num_splits)
    assert out.shape == q.shape and out.dtype == torch.bfloat16
    assert torch.count_nonzero(out[-1]) == 0
    torch.testing.assert_close(out.double(), ref, atol=3e-2, rtol=1e-3)


def test_gqa_decode_unsupported_shape_raises():
    q, k, v, lens, starts, _, _ = _case(64, 4, 2, False)
    with pytest.raises(RuntimeError, match="at least 2 query heads"):
        ops.attention_decode(q[:, :2].contiguous(), k, v, lens, 0.125, grouped=True)
    with pytest.raises(RuntimeError, match="head dim must be 64 or 128"):
        ops.attention_decode(q[..., :32].contiguous(), k[..., :32].contiguous(),
                             v[..., :32].contiguous(), lens, 0.125, grouped=True)


def test_gqa_decode_graph_replay_follows_seq_lens():
    # S = 1024 makes the heuristic split the keys, so the graph holds both launches
    D, Hq, Hkv = 128, 16, 2
    q, k, v, _, _, _, _ = _case(D, Hq, Hkv, False, S=1024)
    lens = torch.tensor([1, 300, 513, 1024, 40], dtype=torch.int32, device="cuda")
    starts = torch.tensor(SEQ_STARTS, dtype=torch.int32, device="cuda")

    def call():
        return ops.attention_decode(q, k, v, lens, D ** -0.5, seq_starts=starts, grouped=True,
                                    num_splits=0)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for new_lens in ([1, 300, 513, 1024, 40], [700, 41, 1024, 32, 41], [64, 1024, 17, 257, 999]):
        lens.copy_(torch.tensor(new_lens, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        eager = call()
        assert torch.equal(out, eager)
        ref = _reference(q, k, v, lens, starts, D ** -0.5, None)
        torch.testing.assert_close(out.double(), ref, atol=3e-2, rtol=1e-3)
