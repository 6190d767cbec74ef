"""csrc/lora.hip through ops.lora_linear against an fp64 evaluation on the same
rounded bf16 inputs: y, dx, dA, dB.

The tolerance is derived.  u = 2^-8 (one bf16 rounding, doubled), e = 2^-24.  A
product P = L @ R over inner length n whose left factor carries the elementwise
error bound bL is bounded by  u |P_ref| + bL @ |R| + n e (|L| @ |R|)  (product()
below; bR is the same with the bound on the right factor).  T = x A^T and
dT = s dY B are such products with bL = 0; the adapter terms of y, dx, dA and dB
are products of T or dT and take bT / bdT (dB on the right).  The base GEMM is
rounded to bf16 before the kernel adds to it: y and dx get one more
u |base_ref| + n e (|L| @ |R|).

y and dx are rounded twice, each by up to 2^-8 in the worst case, so the bound
is tight for them by construction.  A CPU emulation of the kernels (fp32
accumulate, T / dT / outputs rounded once) on exactly these inputs has its worst
element at 0.98 (y), 0.86 (dx), 0.90 (dA), 0.65 (dB) of the bound, and at 90 or
more with one row of T dropped.  Measured on an MI355X: 0.98, 0.86, 0.90, 0.67
(profiles/lora_notes.md section 3)."""
import functools

import pytest
import torch
from conftest import tiny_config

from trlx_amd import ops
from trlx_amd.models.lora import LoRALinear, apply_lora
from trlx_amd.models.nn.transformer import Block

pytestmark = pytest.mark.gpu

U, E = 2.0 ** -8, 2.0 ** -24
# (N, K, O, r): one vector; N off the 16-row group; K, O multiples of 8 but not
# of 16 / 32; rank below, across a 16-tile and across the 32-wide k-step; K past
# one round of the four waves' chunks; a K that lora_shrink splits across blocks
SHAPES = [(1, 8, 8, 1), (17, 40, 24, 8), (33, 72, 136, 16), (70, 264, 40, 40), (5, 520, 72, 64),
          (3, 3 * ops.LORA_SPLIT_COLS + 40, 24, 24)]


def product(L, R, n, bL=None, bR=None, add=0.0):
    P = L @ R + add
    bound = U * P.abs() + n * E * (L.abs() @ R.abs())
    if bL is not None:
        bound = bound + bL @ R.abs()
    if bR is not None:
        bound = bound + L.abs() @ bR
    return P, bound


def reference(x, W, bias, A, B, dy, s):
    """{name: (fp64 value, bound, adapter term of the value)} from bf16 inputs."""
    x, W, A, B, dy = (t.detach().double().cpu() for t in (x, W, A, B, dy))
    bias = 0.0 if bias is None else bias.detach().double().cpu()
    x, dy = x.reshape(-1, x.shape[-1]), dy.reshape(-1, dy.shape[-1])
    N, K, O, r = x.shape[0], x.shape[1], W.shape[0], A.shape[0]
    T, bT = product(x, A.t(), K)
    dT, bdT = product(s * dy, B, O)
    (base, bbase), (lora, blora) = product(x, W.t(), K, add=bias), product(T, s * B.t(), r, bL=bT)
    out = {"y": (base + lora, bbase + blora, lora)}
    (base, bbase), (lora, blora) = product(dy, W, O), product(dT, A, r, bL=bdT)
    out["dx"] = (base + lora, bbase + blora, lora)
    for name, (P, bound) in (("dA", product(dT.t(), x, N, bL=bdT.t())),
                             ("dB", product(s * dy.t(), T, N, bR=bT))):
        out[name] = (P, bound, P)
    return out


@functools.lru_cache(maxsize=None)
def case(N, K, O, r, s):
    gen = torch.Generator().manual_seed(0)

    def rand(*shape, scale=1.0):
        return (torch.randn(*shape, generator=gen) * scale).bfloat16()

    x, dy = rand(N, K), rand(N, O)
    # base and adapter terms of y and of dx get the same magnitude, so that an
    # error in either one shows
    W, A = rand(O, K, scale=K ** -0.5), rand(r, K, scale=K ** -0.5)
    B = rand(O, r, scale=r ** -0.5 / s)
    return (x, W, A, B, dy), reference(x, W, None, A, B, dy, s)


def check(got, ref, slack=lambda bound, ref, lora: bound):
    for (name, (want, bound, lora)), y in zip(ref.items(), got):
        y = y.double().cpu().reshape(want.shape)
        assert torch.isfinite(y).all(), name
        err, tol = (y - want).abs(), slack(bound, want, lora)
        print(f"{name}: max err / bound = {float((err / tol).max()):.3f}")
        assert bool((err <= tol).all()), name


@pytest.mark.parametrize("s", [2.0, 0.25])
@pytest.mark.parametrize("N,K,O,r", SHAPES)
def test_lora_linear_matches_fp64(N, K, O, r, s):
    inputs, ref = case(N, K, O, r, s)
    x, W, A, B, dy = (t.cuda() for t in inputs)
    leaves = [t.requires_grad_() for t in (x, A, B)]
    y = ops.lora_linear(x, W, None, A, B, s)
    grads = torch.autograd.grad(y, leaves, dy)
    assert all(t.dtype == torch.bfloat16 for t in (y, *grads))
    check((y, *grads), ref)


def test_lora_layers_take_the_kernels(monkeypatch):
    """qkv_proj and down_proj of a bf16 Llama-style block under LoRA, switch on:
    within the bound of the fp64 reference, and against the eager lines.  Those
    round three more times (the adapter product, its scaled value, the sum), each
    by 2^-9 of the adapter term or of the result, so eager and fused differ by at
    most 2 bound + u (|adapter term| + |result|).  Two runs are bit-equal, and
    forward + backward replayed from a graph on a new input equal a direct run."""
    torch.manual_seed(0)
    cfg = tiny_config(hidden_size=64, intermediate_size=104, activation="silu", swiglu=True,
                      mlp_bias=False, arch_name="llama")
    block = apply_lora(Block(cfg, 0).cuda().bfloat16(),
                       {"r": 8, "lora_alpha": 16, "target_modules": ["qkv_proj", "down_proj"]})
    for layer in (block.attn.qkv_proj, block.mlp.down_proj):
        assert type(layer) is LoRALinear
        torch.nn.init.normal_(layer.lora_B)
        K, O = layer.base.weight.shape[1], layer.base.weight.shape[0]
        x = torch.randn(2, 5, K, device="cuda").bfloat16().requires_grad_()
        x2 = torch.randn(2, 5, K, device="cuda").bfloat16()
        dy = torch.randn(2, 5, O, device="cuda").bfloat16()
        leaves = [x, layer.lora_A, layer.lora_B]

        def run():
            # detached: see test_gated_mlps_take_the_kernels
            out = layer(x)
            return (out.detach(), *torch.autograd.grad(out, leaves, dy))

        monkeypatch.delenv("TRLX_AMD_FUSED_LORA", raising=False)
        eager = run()
        monkeypatch.setenv("TRLX_AMD_FUSED_LORA", "1")
        seen, real = [], ops.lora_linear
        monkeypatch.setattr(ops, "lora_linear", lambda *a, **k: (seen.append(1), real(*a, **k))[1])
        fused = run()
        assert seen, "the layer did not call ops.lora_linear"
        ref = reference(x, layer.base.weight, layer.base.bias, layer.lora_A, layer.lora_B, dy,
                        layer.scaling)
        check(fused, ref)
        against_eager = {k: (e.double().cpu().reshape(v[0].shape), *v[1:])
                         for (k, v), e in zip(ref.items(), eager)}
        check(fused, against_eager, lambda bound, want, lora: 2 * bound + U * (lora.abs() + want.abs()))
        for a, b in zip(fused, run()):
            assert torch.equal(a, b)

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
