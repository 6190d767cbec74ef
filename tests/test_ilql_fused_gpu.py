"""The fused ILQL path on the GPU: the linear_gather_lse kernels against fp32
torch on the same bf16-rounded operands, the untouched lm_head / CE entry
points against them, the model-level fused loss against the unfused one, and
one hipGraph-captured loss + backward.

Bounds (measured on an MI355X, recorded in profiles/ilql_heads_notes.md):
both sides of the kernel comparison accumulate in fp32, so they differ by
summation order and ``__expf``; the bound is 4x the measured maximum,
rounded up to one digit.  The model-level bounds are 4x the measured
difference between the bf16-operand fused path and the fp32 unfused heads.
"""

import pytest
import torch
import torch.nn.functional as F

from trlx_amd import ops
from trlx_amd.models.modeling_ilql import ILQLConfig, ilql_actions

from test_ilql_fused import loss_and_grads, ragged_ilql_batch, tiny_ilql_model

pytestmark = pytest.mark.gpu

# max |val - ref|, |lse - ref| over CASES measured 7.63e-6 (lse, case
# (257, 1000, 192); case (257, 1281, 64) measured 1.91e-6 and leaves the
# maximum where it was); bound = 4x = 3.05e-5, rounded up to one digit
FWD_BOUND = 4e-5
BF16_ULP = 2.0 ** -7
# tiny model, fused vs unfused: measured loss difference 5.91e-5 and worst
# per-parameter relative gradient error 8.50e-3 (layers.0.ln_1.bias; worst
# cosine 0.999965); bounds = 4x, rounded up to one digit
MODEL_LOSS_BOUND = 3e-4
MODEL_GRAD_REL_BOUND = 4e-2
MODEL_GRAD_COSINE = 0.99

# (257, 1281, 64): 2 x 6 = 12 workgroups, the smallest grid in which the XCD
# remap of csrc/lm_tile.h takes both of its branches with a non-zero quotient
# (q8 = 1, r8 = 4); one K-tile, ragged last row tile and last column tile
CASES = [(1, 256, 64), (255, 257, 64), (257, 1000, 192), (300, 513, 128), (257, 1281, 64)]
_cache = {}


def _ext():
    ext = ops._require_ext("linear_gather_lse")
    assert ext is not None and hasattr(ext, "linear_gather_lse_fwd")
    return ext


def _case(N, V, K):
    """Operands, kernel outputs and the fp32 reference of one case, computed
    once and shared (never modified) by the tests below."""
    key = (N, V, K)
    if key in _cache:
        return _cache[key]
    g = torch.Generator().manual_seed(N * 7 + V)
    x = torch.randn(N, K, generator=g).cuda().bfloat16()
    w = (torch.randn(V, K, generator=g) * 0.5).cuda().bfloat16()
    bias = torch.randn(V, generator=g).cuda()
    idx = torch.randint(0, V, (N,), generator=g)
    # both sides of the 256-column tile edge and the last valid column
    special = [c for c in (V - 1, 255, 256, 0) if c < V]
    for i, c in enumerate(dict.fromkeys(special)):
        if i < N:
            idx[i] = c
    idx = idx.cuda()
    z = x.float() @ w.float().t() + bias
    ref_val = z.gather(-1, idx.unsqueeze(-1)).squeeze(-1)
    ref_lse = torch.logsumexp(z, -1)
    val, lse = _ext().linear_gather_lse_fwd(x, w, bias, idx)
    _cache[key] = dict(x=x, w=w, bias=bias, idx=idx, z=z, ref_val=ref_val, ref_lse=ref_lse,
                       val=val, lse=lse,
                       g_val=torch.randn(N, generator=g).cuda(),
                       g_lse=torch.randn(N, generator=g).cuda())
    return _cache[key]


def _ref_dz(c, g_val, g_lse):
    dz = g_lse[:, None] * torch.exp(c["z"] - c["ref_lse"][:, None])
    return dz.scatter_add(1, c["idx"][:, None], g_val[:, None])


def _assert_dz(dz, ref, gmax, what):
    assert dz.dtype == torch.bfloat16 and dz.shape == ref.shape
    err = (dz.float() - ref).abs()
    tol = FWD_BOUND * gmax + BF16_ULP * ref.abs()
    worst = (err - tol).max().item()
    print(f"{what}: max err {err.max().item():.3e}, max (err - tol) {worst:.3e}")
    assert worst <= 0, what


@pytest.mark.parametrize("N,V,K", CASES)
def test_forward_against_fp32_torch(N, V, K):
    c = _case(N, V, K)
    assert c["val"].dtype == torch.float32 and c["val"].shape == (N,)
    assert c["lse"].dtype == torch.float32 and c["lse"].shape == (N,)
    e_val = (c["val"] - c["ref_val"]).abs().max().item()
    e_lse = (c["lse"] - c["ref_lse"]).abs().max().item()
    # dropping the bias cannot pass: it moves every value by O(1)
    no_bias = c["bias"][c["idx"]].abs().max().item()
    print(f"fwd ({N},{V},{K}): max|val err| {e_val:.3e}  max|lse err| {e_lse:.3e}")
    assert no_bias > 100 * FWD_BOUND
    assert e_val <= FWD_BOUND and e_lse <= FWD_BOUND


@pytest.mark.parametrize("N,V,K", CASES)
def test_backward_against_fp32_torch(N, V, K):
    c = _case(N, V, K)
    ext = _ext()
    zero = torch.zeros_like(c["g_val"])
    # each coefficient alone, so a swapped pair cannot hide, then both
    for what, gv, gl in (("g_lse=0", c["g_val"], zero), ("g_val=0", zero, c["g_lse"]),
                         ("both", c["g_val"], c["g_lse"])):
        dz = ext.linear_gather_lse_bwd(c["x"], c["w"], c["bias"], c["idx"], c["lse"], gv, gl)
        gmax = max(gv.abs().max().item(), gl.abs().max().item())
        _assert_dz(dz, _ref_dz(c, gv, gl), gmax, f"dz ({N},{V},{K}) {what}")
    # rows with both gradients zero come out exactly zero
    rows = torch.arange(N, device="cuda") % 3 == 0
    gv = torch.where(rows, zero, c["g_val"])
    gl = torch.where(rows, zero, c["g_lse"])
    dz = ext.linear_gather_lse_bwd(c["x"], c["w"], c["bias"], c["idx"], c["lse"], gv, gl)
    assert (dz[rows] == 0).all()
    assert (dz[~rows] != 0).any() or N == 1


def test_autograd_op_grads():
    """ops.linear_gather_lse end to end on fp32 inputs (the head parameters'
    dtype): gradients come back in the input dtypes and match fp32 torch on
    the bf16-rounded operands."""
    N, V, K = 257, 1000, 192
    c = _case(N, V, K)
    x = c["x"].float().requires_grad_()
    w = c["w"].float().requires_grad_()
    b = c["bias"].clone().requires_grad_()
    val, lse = ops.linear_gather_lse(x, w, b, c["idx"])
    ((val * c["g_val"]).sum() + (lse * c["g_lse"]).sum()).backward()
    dz = _ref_dz(c, c["g_val"], c["g_lse"])
    for name, got, want in (("dx", x.grad, dz @ c["w"].float()),
                            ("dw", w.grad, dz.t() @ c["x"].float()),
                            ("db", b.grad, dz.sum(0))):
        assert got.dtype == torch.float32
        rel = ((got - want).norm() / want.norm()).item()
        print(f"{name}: relative error {rel:.3e}")
        # dz and the contraction outputs are bf16: 2^-8 relative per element
        assert rel <= BF16_ULP, name


@pytest.mark.parametrize("N,V,K", CASES)
def test_old_entry_points_unchanged(N, V, K):
    c = _case(N, V, K)
    ext = _ext()
    zb = torch.zeros_like(c["bias"])
    out, lse = ext.lm_logprobs_v2_with_lse(c["x"], c["w"], c["idx"], True)
    val0, lse0 = ext.linear_gather_lse_fwd(c["x"], c["w"], zb, c["idx"])
    assert (lse - lse0).abs().max().item() <= FWD_BOUND
    assert (out - (val0 - lse0)).abs().max().item() <= FWD_BOUND
    assert torch.equal(out, ext.lm_logprobs_v2(c["x"], c["w"], c["idx"]))
    z = c["x"].float() @ c["w"].float().t()
    ref = z.gather(-1, c["idx"][:, None]).squeeze(-1) - torch.logsumexp(z, -1)
    assert (out - ref).abs().max().item() <= FWD_BOUND

    g = c["g_val"]
    old = ext.ce_dlogits(c["x"], c["w"], c["idx"], lse, g)
    new = ext.linear_gather_lse_bwd(c["x"], c["w"], zb, c["idx"], lse, g, -g)
    err = (old.float() - new.float()).abs()
    tol = FWD_BOUND * g.abs().max().item() + BF16_ULP * new.float().abs()
    assert (err <= tol).all()


def test_empty_input():
    """N = 0: every entry point of the two files returns the right shape and
    dtype without a launch."""
    ext = _ext()
    V, K = 300, 64
    x = torch.empty(0, K, device="cuda", dtype=torch.bfloat16)
    w = torch.zeros(V, K, device="cuda", dtype=torch.bfloat16)
    bias = torch.zeros(V, device="cuda")
    idx = torch.empty(0, device="cuda", dtype=torch.long)
    f = torch.empty(0, device="cuda")
    outs = [ext.lm_logprobs_v2(x, w, idx), *ext.lm_logprobs_v2_with_lse(x, w, idx, True),
            *ext.linear_gather_lse_fwd(x, w, bias, idx)]
    for o in outs:
        assert o.shape == (0,) and o.dtype == torch.float32
    for dz in (ext.ce_dlogits(x, w, idx, f, f),
               ext.linear_gather_lse_bwd(x, w, bias, idx, f, f, f)):
        assert dz.shape == (0, V) and dz.dtype == torch.bfloat16


def test_rejected_input():
    ext = _ext()
    N, V, K = 255, 257, 64
    c = _case(N, V, K)
    x, w, idx, lse, g = c["x"], c["w"], c["idx"], c["lse"], c["g_val"]
    x96 = torch.zeros(N, 96, device="cuda", dtype=torch.bfloat16)
    w96 = torch.zeros(V, 96, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        ext.lm_logprobs_v2(x96, w96, idx)
    with pytest.raises(RuntimeError):
        ext.ce_dlogits(x96, w96, idx, lse, g)
    with pytest.raises(RuntimeError):
        ext.ce_dlogits(x, w, idx.int(), lse, g)
    with pytest.raises(RuntimeError):
        ext.ce_dlogits(x, w, idx, lse[:-1].contiguous(), g)
    with pytest.raises(RuntimeError):
        ext.ce_dlogits(x, w, idx, lse, g.bfloat16())
    lse2 = torch.stack([lse, lse], 1)[:, 0]
    assert not lse2.is_contiguous() and torch.equal(lse2, lse)
    with pytest.raises(RuntimeError):
        ext.ce_dlogits(x, w, idx, lse2, g)
    # the same operands, well-formed, are accepted
    assert ext.ce_dlogits(x, w, idx, lse, g).shape == (N, V)


def test_strided_dlp():
    ext = _ext()
    N, V, K = 255, 257, 64
    c = _case(N, V, K)
    long = torch.randn(2 * N, generator=torch.Generator().manual_seed(3)).cuda()
    g = long[::2]
    assert not g.is_contiguous() and g.dtype == torch.float32
    got = ext.ce_dlogits(c["x"], c["w"], c["idx"], c["lse"], g)
    want = ext.ce_dlogits(c["x"], c["w"], c["idx"], c["lse"], g.contiguous())
    assert (want != 0).any()
    assert torch.equal(got, want)


def _gpu_model(two_qs=True):
    # bf16 trunk, fp32 heads
    model = tiny_ilql_model(two_qs).cuda()
    model.base_model.to(torch.bfloat16)
    return model


def _to_cuda(batch):
    return type(batch)(*(getattr(batch, f).cuda() for f in batch.__dataclass_fields__))


def test_model_fused_against_unfused():
    model = _gpu_model()
    method = ILQLConfig(beta=0.5)
    batch = _to_cuda(ragged_ilql_batch())
    ref_loss, ref_stats, ref_grads = loss_and_grads(model, method, batch, fused=False)
    loss, stats, grads = loss_and_grads(model, method, batch, fused=True)
    dl = (loss - ref_loss).abs().item()
    print(f"model: loss {loss.item():.6f} vs {ref_loss.item():.6f}, |diff| {dl:.3e}")
    assert stats.keys() == ref_stats.keys()
    worst_rel, worst_cos = 0.0, 1.0
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        g, r = grads[name].float(), ref_grads[name].float()
        rel = ((g - r).norm() / r.norm()).item()
        cos = F.cosine_similarity(g.flatten(), r.flatten(), dim=0).item()
        print(f"model grad {name}: rel {rel:.3e} cos {cos:.6f}")
        worst_rel, worst_cos = max(worst_rel, rel), min(worst_cos, cos)
    print(f"model: worst rel {worst_rel:.3e}, worst cos {worst_cos:.6f}")
    assert dl <= MODEL_LOSS_BOUND
    assert worst_rel <= MODEL_GRAD_REL_BOUND
    assert worst_cos >= MODEL_GRAD_COSINE


def test_captured_fused_step_reproduces_eager_grads():
    model = _gpu_model()
    method = ILQLConfig(beta=0.5)
    batch = _to_cuda(ragged_ilql_batch())
    actions = ilql_actions(batch)

    def step():
        out = model(input_ids=batch.input_ids, attention_mask=batch.attention_mask,
                    actions_ixs=batch.actions_ixs, states_ixs=batch.states_ixs,
                    fused_actions=actions)
        loss, _ = method.loss(out.action_values, batch)
        loss.backward()
        return loss

    params = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    model.zero_grad(set_to_none=True)
    eager_loss = step().detach().clone()
    eager = {n: p.grad.detach().clone() for n, p in params}

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            model.zero_grad(set_to_none=True)
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    model.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_out = step()
    for _ in range(2):
        for _, p in params:
            p.grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss_out, eager_loss)
        for n, p in params:
            assert torch.equal(p.grad, eager[n]), n
    del graph
