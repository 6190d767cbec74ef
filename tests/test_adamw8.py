"""8-bit AdamW on the CPU: names, state format, unbiased rounding, trajectory and
checkpoint round trip of ``FusedAdamW8bit`` / ``reference.adamw8_step``."""
import math

import pytest
import torch
from conftest import tiny_config

from trlx_amd.models.modeling_ppo import AutoModelForCausalLMWithHydraValueHead
from trlx_amd.ops import reference
from trlx_amd.parallel.optim import FusedAdamW, FusedAdamW8bit, build_optimizer
from trlx_amd.utils import get_optimizer_class

NAMES = ["adamw_8bit", "adamw_8bit_bnb", "adam_8bit_bnb"]


def tiny_model():
    torch.manual_seed(0)
    return AutoModelForCausalLMWithHydraValueHead.from_config(tiny_config(), num_layers_unfrozen=1)


@pytest.mark.parametrize("name", NAMES)
def test_names_build_the_8bit_optimizer(name):
    opt = build_optimizer(tiny_model(), name, dict(lr=1e-3, weight_decay=0.0))
    assert isinstance(opt, FusedAdamW8bit) and isinstance(opt, FusedAdamW)
    assert all("m8" in a and "m" not in a for group in opt._arenas for a in group)
    assert get_optimizer_class(name) is torch.optim.AdamW


def test_adam_8bit_bnb_refuses_weight_decay():
    with pytest.raises(ValueError, match="weight_decay"):
        build_optimizer(tiny_model(), "adam_8bit_bnb", dict(lr=1e-3, weight_decay=0.01))


def test_small_arena_keeps_fp32_moments():
    opt = build_optimizer(tiny_model(), "adamw_8bit", dict(lr=1e-3, min_8bit_size=10 ** 9))
    assert all("m" in a and "m8" not in a for group in opt._arenas for a in group)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_format_after_one_step(n):
    gen = torch.Generator().manual_seed(n)
    g = torch.randn(n, generator=gen)
    p = torch.randn(n, generator=gen)
    m8, u8 = torch.zeros(n, dtype=torch.uint8), torch.zeros(n, dtype=torch.uint8)
    nb = -(-n // 256)
    ms, us = torch.zeros(nb), torch.zeros(nb)
    reference.adamw8_step(p, p.clone(), g, m8, ms, u8, us, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0)
    # from zero state, in the step's own fp32 operations
    want = {"m": (0.9 * torch.zeros(n) + reference._f32(1 - reference._f32(0.9)) * g, m8, ms),
            "u": (reference._sqrt32(0.999 * torch.zeros(n)
                                   + reference._f32(1 - reference._f32(0.999)) * (g * g)),
                  u8, us)}
    for name, (x, codes, scales) in want.items():
        assert not bool(((codes & 0x7F) == 0x7F).any()), name  # the e4m3 NaN byte
        deq = reference.adamw8_dequant(codes, scales)
        for b in range(nb):
            blk = x[b * 256:(b + 1) * 256]
            top = blk.abs().argmax()
            assert scales[b] == blk.abs().max() * torch.tensor(1 / 448, dtype=torch.float32), name
            # 448 * (absmax / 448): two fp32 roundings, one to compare within
            torch.testing.assert_close(deq[b * 256 + top], blk[top], rtol=2.0 ** -23, atol=0)


def test_stochastic_rounding_is_unbiased():
    """y = 1.3 lies between the grid points 1.25 and 1.375 (step 2^-3).  The mean
    of 2^16 roundings is within 5 standard errors of a uniform draw's spread,
    5 step / sqrt(12 * 2^16); round-to-nearest is off by 0.05 = 113 of them."""
    count, step = 2 ** 16, 0.125
    y = torch.full((count,), 1.3)
    q = reference.adamw8_stochastic_round(y, torch.arange(count), seed=0, step=7)
    assert set(q.tolist()) == {1.25, 1.375}
    assert (q.to(torch.float8_e4m3fn).float() == q).all()  # the hardware convert is exact
    bound = 5 * step / math.sqrt(12 * count)
    err = abs(float(q.double().mean()) - float(y[0].double()))
    print(f"mean error {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def least_squares(cls, seed, steps=200):
    gen = torch.Generator().manual_seed(seed)
    a, x = torch.randn(256, 64, generator=gen), torch.randn(64, 64, generator=gen)
    b = a @ x
    w = torch.nn.Parameter(torch.zeros(64, 64))
    opt = cls([w], lr=1e-2)
    for _ in range(steps):
        ((a @ w - b) ** 2).mean().backward()
        opt.step()
        opt.zero_grad()
    return float(((a @ w - b) ** 2).mean().detach())


def test_trajectory_tracks_fp32_adamw():
    """4096 parameters, 200 steps, lr 1e-2 (the loss falls from about 64 to about
    2.5): final loss of the 8-bit run over the fp32 run's.  Measured on the CPU
    over seeds 0..4: 0.7915, 0.8297, 0.8213, 0.7483, 0.8638; the bound is twice
    the worst of them."""
    ratio = least_squares(FusedAdamW8bit, 0) / least_squares(FusedAdamW, 0)
    print(f"loss ratio 8-bit / fp32: {ratio:.4f}")
    assert ratio <= TRAJECTORY_BOUND


TRAJECTORY_BOUND = 2 * 0.8638


def test_state_dict_round_trip_is_bit_exact():
    def fresh():
        torch.manual_seed(3)
        return torch.nn.Parameter(torch.randn(5000))

    gen = torch.Generator().manual_seed(4)
    grads = [torch.randn(5000, generator=gen) for _ in range(3)]

    def run(opt, w, some):
        for g in some:
            w.grad.copy_(g)
            opt.step()

    w1 = fresh()
    straight = FusedAdamW8bit([w1], lr=1e-2, weight_decay=0.01, seed=5)
    run(straight, w1, grads)
    w2 = fresh()
    first = FusedAdamW8bit([w2], lr=1e-2, weight_decay=0.01, seed=5)
    run(first, w2, grads[:2])
    state = first.state_dict()
    assert state["state_bits"] == 8 and state["step"] == 2
    w3 = fresh()
    resumed = FusedAdamW8bit([w3], lr=1e-2, weight_decay=0.01, seed=5)
    resumed.load_state_dict(state)
    run(resumed, w3, grads[2:])
    for k in ("master", "m8", "m_scale", "u8", "u_scale"):
        assert torch.equal(resumed._arenas[0][0][k], straight._arenas[0][0][k]), k
    with pytest.raises(ValueError, match="8-bit"):
        FusedAdamW([fresh()], lr=1e-2).load_state_dict(state)
    with pytest.raises(ValueError, match="32-bit"):
        resumed.load_state_dict(FusedAdamW([fresh()], lr=1e-2).state_dict())


def test_config_name_trains_ppo(tmp_path, tiny_cfg):
    import trlx_amd
    from trlx_amd.data.default_configs import default_ppo_config

    cfg = default_ppo_config()
    cfg.model.model_path = "tiny"
    cfg.model.model_extra_configs = {"config": tiny_cfg.to_dict()}
    cfg.tokenizer.tokenizer_path = "byte"
    cfg.optimizer.name = "adamw_8bit_bnb"
    cfg.train.seq_length, cfg.train.batch_size, cfg.train.total_steps = 32, 4, 2
    cfg.train.eval_interval, cfg.train.checkpoint_interval = 2, 100
    cfg.train.tracker, cfg.train.save_best = None, False
    cfg.train.checkpoint_dir = str(tmp_path / "ck")
    cfg.method.num_rollouts, cfg.method.chunk_size, cfg.method.ppo_epochs = 4, 4, 1
    cfg.method.gen_kwargs = dict(max_new_tokens=4, top_k=0, top_p=1.0, do_sample=True)
    trainer = trlx_amd.train(reward_fn=lambda samples, **kw: [1.0] * len(samples),
                             prompts=["aa", "bb", "cc", "dd"], eval_prompts=["aa"] * 4, config=cfg)
    assert trainer.iter_count == 2 and isinstance(trainer.opt, FusedAdamW8bit)
    assert trainer.opt._step == 2 and any("m8" in a for g in trainer.opt._arenas for a in g)


def test_block_absmax_never_rounds_past_the_range():
    """The absmax of a block is y = 448 = 14 * 32.  Seed 0, step 1, index 5494511
    draw r = 1 - 6 * 2^-24, and the fp32 sum 14 + r rounds to 15: unclamped that
    is 480, the e4m3 NaN byte 0x7F, and a NaN weight one step later."""
    idx, lane = 5494511, 5
    q = reference.adamw8_stochastic_round(torch.tensor([448.0]), torch.tensor([idx]), 0, 1)
    assert float(q) == 448.0
    g = torch.zeros(256)
    g[lane] = 1.0
    p = torch.ones(256)
    state = [torch.zeros(256, dtype=torch.uint8), torch.zeros(1),
             torch.zeros(256, dtype=torch.uint8), torch.zeros(1)]
    for step in (1, 2):
        reference.adamw8_step(p, p, g, *state, step, 1e-3, 0.9, 0.999, 1e-8, 0.0,
                              seed=0, index_base=idx - lane)
        assert state[2][lane] == 0x7E or step == 2
    assert torch.isfinite(p).all() and torch.isfinite(state[3]).all()
