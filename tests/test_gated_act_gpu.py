"""gated_act.hip against an fp64 evaluation of act(g) * u and its autograd
gradients on the same (already rounded) inputs.

Tolerances, elementwise, for h, dg and du: |y - ref| <= RTOL |ref| + 1e-5.
bf16: RTOL = 1.5 * 2^-8 (one bf16 rounding of a correctly computed value, half
as much again for fp32 evaluation with the device's exp / erf); the 1e-5 covers
the cancelling tails of 1 + erf at |g| <= 8.  fp32: RTOL = 2 * 4.64e-7, twice
the largest relative error of the eager fp32 expression (forward and autograd
gradients, on the CPU) against the same fp64 reference over exactly the cases
below, measured with the same floor: the smallest r for which |eager - ref| <=
r |ref| + 1e-5 holds everywhere.  The 4.64e-7 is dg of gelu_new at (2, 4104);
every other output stays under 5e-8 (profiles/gated_act_notes.md section 3)."""
import functools

import pytest
import torch
import torch.nn.functional as F
from conftest import tiny_config

from trlx_amd import ops
from trlx_amd.models.nn.seq2seq import Seq2SeqConfig, T5FFN
from trlx_amd.models.nn.transformer import MLP

pytestmark = pytest.mark.gpu

ATOL = 1e-5
RTOL = {torch.bfloat16: 1.5 * 2.0 ** -8, torch.float32: 2 * 4.64e-7}
ACTS = {"silu": F.silu, "gelu_new": lambda x: F.gelu(x, approximate="tanh"), "gelu": F.gelu}
SPECIALS = [0.0, 1e-3, -1e-3, 20.0, -20.0, 88.0, -88.0, 1e4, -1e4]
# one vector; vector path with a partly empty last chunk; odd I (the fused up
# half misaligned: scalar instantiation); one full chunk plus a one-vector tail
SHAPES = [(1, 8), (5, 1000), (3, 1001), (2, ops.GATED_ACT_CHUNK + 8)]


@functools.lru_cache(maxsize=None)
def case(act, dtype, N, I):
    """CPU tensors g, u, dh in ``dtype`` and the fp64 (h, dg, du) of them."""
    gen = torch.Generator().manual_seed(1000 * N + I)
    g, u, dh = ((2 * torch.randn(N, I, generator=gen)).clamp(-8, 8).to(dtype) for _ in range(3))
    k = min(I, len(SPECIALS))
    g[0, :k] = torch.tensor(SPECIALS[:k]).to(dtype)
    gd, ud = g.double().requires_grad_(), u.double().requires_grad_()
    h = ACTS[act](gd) * ud
    dg, du = torch.autograd.grad(h, (gd, ud), dh.double())
    return g, u, dh, (h.detach(), dg, du)


def check(names, got, want, rtol):
    for name, y, r in zip(names, got, want):
        y, r = y.double().cpu(), r.double().cpu()
        assert y.shape == r.shape and torch.isfinite(y).all(), name
        err, bound = (y - r).abs(), rtol * r.abs() + ATOL
        print(f"{name}: max err / bound = {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), name


@pytest.mark.parametrize("N,I", SHAPES)
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("act", list(ACTS))
def test_gated_act_matches_fp64(act, dtype, fused, N, I):
    g, u, dh, ref = case(act, dtype, N, I)
    dh = dh.cuda()
    if fused:
        gu = torch.cat([g, u], dim=-1).cuda().requires_grad_()
        h = ops.gated_act(gu, act=act)
        (dgu,) = torch.autograd.grad(h, gu, dh)
        assert dgu.shape == gu.shape
        dg, du = dgu[:, :I], dgu[:, I:]
    else:
        gg, uu = g.cuda().requires_grad_(), u.cuda().requires_grad_()
        h = ops.gated_act(gg, uu, act=act)
        dg, du = torch.autograd.grad(h, (gg, uu), dh)
    assert h.dtype == dg.dtype == du.dtype == dtype
    check(("h", "dg", "du"), (h, dg, du), ref, RTOL[dtype])


def test_gated_mlps_take_the_kernels(monkeypatch):
    """The swiglu MLP and the gated T5FFN with the switch on against their eager
    line, fp32: output, input gradient and every weight gradient; then forward
    and backward captured into a graph and replayed on a new input."""
    torch.manual_seed(0)
    cfg = tiny_config(hidden_size=64, intermediate_size=104, activation="silu", swiglu=True,
                      mlp_bias=False, arch_name="llama")
    t5 = Seq2SeqConfig(d_model=64, d_ff=104, feed_forward_proj="gated-gelu")
    for module in (MLP(cfg).cuda(), T5FFN(t5).cuda()):
        params = list(module.parameters())
        x = torch.randn(2, 5, 64, device="cuda", requires_grad=True)
        x2, dy = torch.randn(2, 2, 5, 64, device="cuda")

        def run():
            # out is returned detached: a result that kept its autograd graph
            # alive would keep the leaves' gradient accumulators, made on this
            # stream, for the capture on another one, where the engine would
            # then synchronise the two streams inside the capture
            out = module(x)
            return (out.detach(), *torch.autograd.grad(out, [x, *params], dy))

        monkeypatch.delenv("TRLX_AMD_FUSED_GATED_ACT", raising=False)
        eager = run()
        monkeypatch.setenv("TRLX_AMD_FUSED_GATED_ACT", "1")
        seen, real = [], ops.gated_act
        monkeypatch.setattr(ops, "gated_act", lambda *a, **k: (seen.append(1), real(*a, **k))[1])
        fused = run()
        assert seen, "the module did not call ops.gated_act"
        names = ["out", "dx"] + [n for n, _ in module.named_parameters()]
        check(names, fused, eager, RTOL[torch.float32])

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = run()
        with torch.no_grad():
            x.copy_(x2)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(captured, run()):
            assert torch.equal(a, b)
        monkeypatch.undo()
