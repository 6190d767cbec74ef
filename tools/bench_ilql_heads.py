"""ILQL heads alone, forward + backward: vocabulary-wide (``ILQLHeads.forward``
+ gather + cross-entropy, what ``ILQLConfig.loss`` does with the full tensors)
against the fused ``ILQLHeads.forward_actions``, at the ILQL bench shape
(gpt2: batch 128, 63 actions per row, hidden 768, vocab 50257).

Prints ms per forward+backward and torch.cuda.max_memory_allocated for each.
One process, a fixed number of iterations, no retries.

    python tools/bench_ilql_heads.py [--head-dtype fp32|bf16] [--iters 10]
"""

import argparse
import json
import os
import sys
from functools import reduce

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from trlx_amd.models.modeling_ilql import ILQLHeads  # noqa: E402


def head_terms_unfused(heads, hs, states_ixs, actions_ixs, actions):
    qs, target_qs, vs = heads(hs, states_ixs=states_ixs, actions_ixs=actions_ixs)
    a = actions.unsqueeze(-1)
    q = [x.gather(-1, a).squeeze(-1) for x in qs]
    tq = [x.gather(-1, a).squeeze(-1).detach() for x in target_qs]
    ce = [F.cross_entropy(x.reshape(-1, x.shape[-1]), actions.reshape(-1), reduction="none")
          .reshape(actions.shape) for x in qs]
    return q, ce, tq, vs


def head_terms_fused(heads, hs, states_ixs, actions_ixs, actions):
    q, q_lse, tq, vs = heads.forward_actions(hs, states_ixs, actions_ixs, actions)
    return list(q), [lse - x for lse, x in zip(q_lse, q)], list(tq), vs


def head_loss(terms):
    q, ce, tq, vs = terms
    target = reduce(torch.minimum, tq).float()
    v = vs[:, :-1, 0].float()
    return (sum((x.float() - target).pow(2).mean() for x in q) + (target - v).pow(2).mean()
            + sum(x.float().mean() for x in ce))


def measure(fn, heads, hs, args4, iters, warmup):
    def step():
        hs.grad = None
        heads.zero_grad(set_to_none=True)
        loss = head_loss(fn(heads, hs, *args4))
        loss.backward()
        return loss

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        loss = step()
    end.record()
    torch.cuda.synchronize()
    return dict(ms=round(start.elapsed_time(end) / iters, 3), loss=round(float(loss), 6),
                peak_gb=round(torch.cuda.max_memory_allocated() / 2**30, 3),
                resident_gb=round(base / 2**30, 3))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=128)
    p.add_argument("--actions", type=int, default=63)
    p.add_argument("--hidden", type=int, default=768)
    p.add_argument("--vocab", type=int, default=50257)
    p.add_argument("--head-dtype", choices=["fp32", "bf16"], default="fp32")
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    args = p.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"

    torch.manual_seed(0)
    dtype = torch.float32 if args.head_dtype == "fp32" else torch.bfloat16
    heads = ILQLHeads(args.hidden, args.vocab, two_qs=True, alpha=0.5).cuda().to(dtype)
    B, na = args.batch, args.actions
    hs = torch.randn(B, na + 1, args.hidden, device="cuda").bfloat16().requires_grad_()
    actions_ixs = torch.arange(na, device="cuda").expand(B, na).contiguous()
    states_ixs = torch.arange(na + 1, device="cuda").expand(B, na + 1).contiguous()
    actions = torch.randint(0, args.vocab, (B, na), device="cuda")
    args4 = (states_ixs, actions_ixs, actions)

    out = dict(shape=dict(N=B * na, V=args.vocab, K=2 * args.hidden), head_dtype=args.head_dtype)
    for name, fn in (("unfused", head_terms_unfused), ("fused", head_terms_fused)):
        out[name] = measure(fn, heads, hs, args4, args.iters, args.warmup)
    out["speedup"] = round(out["unfused"]["ms"] / out["fused"]["ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
