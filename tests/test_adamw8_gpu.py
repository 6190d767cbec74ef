"""adamw8.hip against ``reference.adamw8_step``, one step from an uploaded
reference state (2 warm-up steps on the CPU), so a rare code flip cannot compound.

Master and p are held to an fp64 evaluation of the step (the kernel's fp32
hyper-parameters, every operation in fp64) from the same decoded state:
|w - ref| <= RTOL |ref| + ATOL.  ATOL = 2e-8 is a floor for weights near zero:
an update is at most about 2 lr = 2e-2 here and carries a dozen fp32 roundings
of itself, 12 * 2^-24 * 2e-2 = 1.4e-8.  RTOL = 2 * 1.073e-7, twice the smallest
r for which the CPU fp32 reference meets |w32 - w64| <= r |w64| + 2e-8 on
exactly the cases below (the worst is the second-trip case at 256 CUs; the other
cases of more than one element lie between 7.5e-8 and 9.7e-8).  A bf16 p gets one more
bf16 rounding, 2^-8.  Scales: within 2 fp32 ulp.  Codes: equal, but for at most
0.1 % of a case's elements (none below 1000 elements), each of which decodes to
a neighbouring e4m3 value."""
import copy
import functools

import pytest
import torch
from conftest import tiny_config

from trlx_amd import ops
from trlx_amd.models.modeling_ppo import AutoModelForCausalLMWithHydraValueHead
from trlx_amd.ops import reference
from trlx_amd.parallel.optim import FusedAdamW8bit

pytestmark = pytest.mark.gpu

ATOL, RTOL = 2e-8, 2 * 1.073e-7
HYPER = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, grad_scale=0.5,
             seed=11)
BF16, FP32 = torch.bfloat16, torch.float32
SECOND_TRIP = -1  # n that fills every block of the grid once, then one tile and 3 elements
CASES = [(pt, gt, n, 0, False) for pt, gt in ((BF16, BF16), (FP32, FP32), (BF16, FP32))
         for n in (1, 255, 257, 8 * 256 + 3)]
CASES += [(BF16, BF16, SECOND_TRIP, 0, False), (BF16, BF16, 8 * 256 + 3, 12345, True)]


def second_trip_n(cus):
    return cus * ops.ADAMW8_BLOCKS_PER_CU * ops.ADAMW8_TILE + ops.ADAMW8_TILE + 3


@functools.lru_cache(maxsize=None)
def case(pt, gt, n, index_base):
    """(state before the step, gradient, state after reference.adamw8_step, fp64
    master of the same step); a state is p, master, m8, m_scale, u8, u_scale."""
    gen = torch.Generator().manual_seed(n + index_base)
    nb = -(-n // 256)
    mag = (2.0 ** torch.linspace(-12, 4, nb)).repeat_interleave(256)[:n]
    if nb >= 4:
        mag[256:512] = 0  # a block of zeros
        mag[513:768] = 0  # a block with one non-zero element
    master = torch.randn(n, generator=gen)
    p = master if pt == FP32 else master.to(pt)
    state = [p, master, torch.zeros(n, dtype=torch.uint8), torch.zeros(nb),
             torch.zeros(n, dtype=torch.uint8), torch.zeros(nb)]
    for step in (1, 2, 3):
        g = (torch.randn(n, generator=gen) * mag).to(gt)
        if step == 3:
            before = [t.clone() for t in state]
            m = reference.adamw8_dequant(state[2], state[3]).double()
            u = reference.adamw8_dequant(state[4], state[5]).double()
            # the kernel's fp32 hyper-parameters, then every operation in fp64
            f32 = reference._f32
            lr, b1, b2, eps = f32(1e-2), f32(0.9), f32(0.999), f32(1e-8)
            gd = g.double() * HYPER["grad_scale"]
            m = b1 * m + f32(1 - b1) * gd
            v = b2 * u * u + f32(1 - b2) * gd * gd
            w64 = state[1].double()
            w64 = w64 - f32(lr * f32(0.01)) * w64
            w64 = w64 - lr * (m / f32(1 - 0.9 ** 3)) / ((v / f32(1 - 0.999 ** 3)).sqrt() + eps)
        reference.adamw8_step(state[0], state[1], g, *state[2:], step,
                              **dict(HYPER, index_base=index_base))
    return before, g, state, w64


def shifted(t, misalign):
    """``t`` on the GPU; with ``misalign`` at a base that is 4 B past a 16 B one."""
    if not misalign:
        return t.cuda()
    off = 4 // t.element_size()
    buf = torch.zeros(t.numel() + off, dtype=t.dtype, device="cuda")
    buf[off:].copy_(t)
    return buf[off:]


def code_order(c):
    """e4m3 bytes as integers in value order (sign-magnitude to signed)."""
    c = c.to(torch.int32)
    return (c & 0x7F) * (1 - 2 * (c >> 7))


def check(got, want, w64, n):
    p, master, m8, m_scale, u8, u_scale = (t.cpu() for t in got)
    for name, w, extra in (("master", master, 0.0), ("p", p, 2.0 ** -8 if p.dtype == BF16 else 0.0)):
        err = (w.double() - w64).abs()
        bound = (RTOL + extra) * w64.abs() + ATOL
        print(f"{name}: max err / bound = {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), name
    for name, s, r in (("m_scale", m_scale, want[3]), ("u_scale", u_scale, want[5])):
        ulps = (s.view(torch.int32) - r.view(torch.int32)).abs().max()
        print(f"{name}: max ulp = {int(ulps)}")
        assert ulps <= 2, name
    for name, c, r in (("m8", m8, want[2]), ("u8", u8, want[4])):
        differ = c != r
        print(f"{name}: {int(differ.sum())} of {n} codes differ")
        assert int(differ.sum()) <= (n // 1000 if n >= 1000 else 0), name
        assert bool(((code_order(c) - code_order(r)).abs() <= 1).all()), name


@pytest.mark.parametrize("pt,gt,n,index_base,misalign", CASES)
def test_kernel_matches_reference(pt, gt, n, index_base, misalign):
    if n == SECOND_TRIP:
        n = second_trip_n(torch.cuda.get_device_properties(0).multi_processor_count)
    before, g, want, w64 = case(pt, gt, n, index_base)
    state = [shifted(t, misalign) for t in before]
    if pt == FP32:
        state[0] = state[1]  # fp32 params are their own master
    ops.adamw8_step(state[0], state[1], shifted(g, misalign), *state[2:], 3,
                    **dict(HYPER, index_base=index_base))
    check(state, want, w64, n)


@pytest.mark.parametrize("dtype", [FP32, BF16], ids=["fp32", "bf16"])
def test_optimizer_gpu_matches_cpu(dtype):
    torch.manual_seed(0)
    cpu = AutoModelForCausalLMWithHydraValueHead.from_config(tiny_config(), num_layers_unfrozen=1)
    cpu = cpu.to(dtype)
    gpu = copy.deepcopy(cpu).cuda()
    opts = [FusedAdamW8bit([p for p in m.parameters() if p.requires_grad], lr=1e-2,
                           weight_decay=0.01, seed=3) for m in (cpu, gpu)]
    gen = torch.Generator().manual_seed(1)
    steps = 3
    for _ in range(steps):
        for (fg_c, _), (fg_g, _) in zip(*(o.grad_arenas() for o in opts)):
            fg_c.copy_(torch.randn(fg_c.numel(), generator=gen).to(dtype))
            fg_g.copy_(fg_c)
        for o in opts:
            o.step()
    for a_c, a_g in zip(opts[0]._arenas[0], opts[1]._arenas[0]):
        assert "m8" in a_g and a_g["m8"].is_cuda
        ref = a_c["master"].double()
        err = (a_g["master"].cpu().double() - ref).abs()
        bound = steps * (RTOL * ref.abs() + ATOL)
        print(f"master: max err / bound = {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())


def test_block_absmax_never_rounds_past_the_range():
    """tests/test_adamw8.py's case of the same name through the kernel: the draw
    that carries y = 448 to 480 must store 0x7E, as the reference does."""
    idx, lane = 5494511, 5
    g = torch.zeros(256)
    g[lane] = 1.0
    want = [torch.ones(256), torch.zeros(256, dtype=torch.uint8), torch.zeros(1),
            torch.zeros(256, dtype=torch.uint8), torch.zeros(1)]
    got = [t.cuda() for t in want]
    for state, grad in ((want, g), (got, g.cuda())):
        ops.adamw8_step(state[0], state[0], grad, *state[1:], 1, 1e-3, 0.9, 0.999, 1e-8, 0.0,
                        seed=0, index_base=idx - lane)
    assert want[3][lane] == 0x7E
    torch.testing.assert_close(got[0].cpu(), want[0], rtol=RTOL, atol=ATOL)
    for a, b in zip(got[1:], want[1:]):
        assert torch.equal(a.cpu(), b)
