"""A/B of T5 attention: the flash kernels' seq2seq modes (ops.seq2seq_attention)
against the eager sequence T5Attention ran before them
(matmul -> .float() -> + position_bias -> + mask -> softmax -> cast -> matmul).

Both sides run in this one process on the same inputs, alternating window by
window (eager, flash, eager, flash, ...), so drift of the box hits both alike;
the range over the windows is printed next to the median, and a difference
inside the eager side's own range is not a difference.  Times are device
events around a window of calls after ``--warm`` warm calls; the number of
calls is chosen per measurement so that a window lasts at least ``--window-ms``
(100 ms by default: a window of a few milliseconds measures the clock and the
scheduler as much as the kernels), and never fewer than ``--calls``.

After the op shapes, one ``ppo_sentiments_t5``-shaped experience pass (hydra
forward under no_grad: policy + value + frozen reference branch) and one train
step (forward + backward, top decoder blocks unfrozen) of a t5-small-sized
model are timed with the kernels off / on through the two switches.

    python tools/bench_t5_attention.py [--out profiles/t5_attention.json]

Needs a GPU: there is no CPU fallback for a timing."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from trlx_amd import ops  # noqa: E402
from trlx_amd.models.nn.seq2seq import AttnMask  # noqa: E402

DEV = "cuda"

# (name, B, H, D, Tq, Tk, causal, with_bias)
SHAPES = [
    ("enc self  t5-small-ish", 32, 8, 64, 128, 128, False, True),
    ("enc self  t5-large-ish", 8, 16, 64, 512, 512, False, True),
    ("enc self  t5-11b-ish  ", 8, 32, 128, 512, 512, False, True),
    ("dec self  T=32        ", 32, 8, 64, 32, 32, True, True),
    ("dec self  T=128       ", 32, 8, 64, 128, 128, True, True),
    ("cross     Tq=64 Tk=512", 8, 16, 64, 64, 512, False, False),
]


def eager_attention(q, k, v, dense_bias, additive_mask):
    scores = torch.matmul(q, k.transpose(-1, -2)).float()
    if dense_bias is not None:
        scores = scores + dense_bias.float()
    if additive_mask is not None:
        scores = scores + additive_mask.float()
    probs = torch.softmax(scores, dim=-1).to(v.dtype)
    return torch.matmul(probs, v)


def time_calls(fn, calls, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / calls


def alternate(sides, windows, calls, warm, window_ms=0.0):
    """sides: {name: fn}; returns {name: [ms per call, one per window]} plus
    the number of calls per window under "calls".  Both
    sides get the same number of calls: enough for the FASTER side's window to
    last ``window_ms`` (probed with one short window each), at least ``calls``."""
    if window_ms > 0:
        fastest = min(time_calls(fn, calls, warm) for fn in sides.values())
        calls = max(calls, int(window_ms / fastest) + 1)
    out = {name: [] for name in sides}
    for _ in range(windows):
        for name, fn in sides.items():
            out[name].append(time_calls(fn, calls, warm))
    out["calls"] = calls
    return out


def summarize(ms):
    return dict(median=statistics.median(ms), lo=min(ms), hi=max(ms))


def bench_shape(name, B, H, D, Tq, Tk, causal, with_bias, args):
    torch.manual_seed(0)
    q, k, v = (torch.randn(B, H, T, D, device=DEV).mul_(0.5).bfloat16() for T in (Tq, Tk, Tk))
    dout = torch.randn(B, H, Tq, D, device=DEV).mul_(0.5).bfloat16()
    key_mask = torch.ones(B, Tk, dtype=torch.uint8, device=DEV)
    # every other row padded by an eighth: encoder keys on the left, decoder
    # tokens on the right (so every causal row keeps a visible key)
    if causal:
        key_mask[::2, Tk - Tk // 8:] = 0
    else:
        key_mask[::2, : Tk // 8] = 0
    vec = zero = dense = None
    if with_bias:
        table = torch.randn(32, H, device=DEV).bfloat16()
        vec, zero = ops.t5_rel_bias(table, Tq, Tk, 0, not causal)
        dense = ops.reference.gather_rel_bias(vec, zero, Tq, Tk)[None].to(torch.bfloat16)
    additive = AttnMask(key_mask, causal=causal, q_len=Tq, device=DEV).additive()
    rows = []
    for direction in ("forward", "forward+backward"):
        if direction == "forward":
            def eager():
                with torch.no_grad():
                    return eager_attention(q, k, v, dense, additive)

            def flash():
                with torch.no_grad():
                    return ops.seq2seq_attention(q, k, v, vec, zero or 0, key_mask, causal)
        else:
            qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))

            def eager():
                eager_attention(qg, kg, vg, dense, additive).backward(dout)
                qg.grad = kg.grad = vg.grad = None

            def flash():
                ops.seq2seq_attention(qg, kg, vg, vec, zero or 0, key_mask, causal).backward(dout)
                qg.grad = kg.grad = vg.grad = None
        with torch.no_grad():
            a = eager_attention(q, k, v, dense, additive).float()
            b = ops.seq2seq_attention(q, k, v, vec, zero or 0, key_mask, causal).float()
        res = alternate({"eager": eager, "flash": flash}, args.windows, args.calls, args.warm,
                        args.window_ms)
        row = dict(kind="op", shape=name.strip(), B=B, H=H, D=D, Tq=Tq, Tk=Tk, causal=causal,
                   bias=with_bias, direction=direction, eager_ms=summarize(res["eager"]),
                   flash_ms=summarize(res["flash"]), calls_per_window=res["calls"],
                   max_abs_diff=(a - b).abs().max().item())
        row["flash_over_eager"] = row["flash_ms"]["median"] / row["eager_ms"]["median"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def bench_bias_cost(name, B, H, D, Tq, Tk, causal, with_bias, args):
    """What the Toeplitz-vector loads cost: the flash forward with the bias
    read through L1 against the same call without a bias (decides whether a
    per-tile LDS window for the vector is worth building)."""
    torch.manual_seed(0)
    q, k, v = (torch.randn(B, H, T, D, device=DEV).mul_(0.5).bfloat16() for T in (Tq, Tk, Tk))
    vec, zero = ops.t5_rel_bias(torch.randn(32, H, device=DEV), Tq, Tk, 0, not causal)
    key_mask = torch.ones(B, Tk, dtype=torch.uint8, device=DEV)

    def with_b():
        with torch.no_grad():
            return ops.seq2seq_attention(q, k, v, vec, zero, key_mask, causal)

    def without():
        with torch.no_grad():
            return ops.seq2seq_attention(q, k, v, None, 0, key_mask, causal)

    res = alternate({"bias": with_b, "no_bias": without}, args.windows, args.calls, args.warm,
                    args.window_ms)
    row = dict(kind="bias_cost", shape=name.strip(), D=D, Tq=Tq, Tk=Tk,
               bias_ms=summarize(res["bias"]), no_bias_ms=summarize(res["no_bias"]),
               calls_per_window=res["calls"])
    row["bias_over_no_bias"] = row["bias_ms"]["median"] / row["no_bias_ms"]["median"]
    print(json.dumps(row), flush=True)
    return [row]


def bench_model(args):
    """ppo_sentiments_t5 shape: t5-small-sized model, prompts 128, 25
    decoder tokens (start token + 24 new), chunk 16 for the experience pass,
    batch 8 for the train step, num_layers_unfrozen=2."""
    from trlx_amd.models.modeling_seq2seq import AutoModelForSeq2SeqLMWithHydraValueHead
    from trlx_amd.models.nn.seq2seq import Seq2SeqConfig, Seq2SeqTransformer
    from trlx_amd.utils.modeling import freeze_bottom_seq2seq_layers, logprobs_of_labels

    torch.manual_seed(0)
    cfg = Seq2SeqConfig()  # t5-small: d_model 512, 8 heads x 64, 6 + 6 layers
    model = AutoModelForSeq2SeqLMWithHydraValueHead(Seq2SeqTransformer(cfg), num_layers_unfrozen=2)
    freeze_bottom_seq2seq_layers(model.base_model, 2)
    model = model.to(DEV)
    model.cast_compute(torch.bfloat16)

    def batch(n):
        ids = torch.randint(2, cfg.vocab_size, (n, 128), device=DEV)
        mask = torch.ones_like(ids)
        mask[::2, :16] = 0
        dec = torch.randint(2, cfg.vocab_size, (n, 25), device=DEV)
        return ids, mask, dec, torch.ones_like(dec)

    exp_batch, train_batch = batch(16), batch(8)

    def experience():
        with torch.no_grad():
            model(*exp_batch, return_ref_logits=True)

    def train():
        ids, mask, dec, dmask = train_batch
        out = model(ids, mask, dec, dmask)
        lp = logprobs_of_labels(out.logits[:, :-1], dec[:, 1:])
        (lp.mean() + out.values.pow(2).mean()).backward()
        model.zero_grad(set_to_none=True)

    def switched(fn, on):
        def run():
            os.environ["TRLX_AMD_NO_FLASH_PREFILL"] = "0" if on else "1"
            os.environ["TRLX_AMD_NO_FLASH_TRAIN"] = "0" if on else "1"
            fn()
        return run

    rows = []
    for name, fn in (("experience pass (chunk 16)", experience), ("train step (batch 8)", train)):
        res = alternate({"eager": switched(fn, False), "flash": switched(fn, True)},
                        args.windows, max(args.calls // 4, 5), args.warm, args.window_ms)
        row = dict(kind="model", shape=name, eager_ms=summarize(res["eager"]),
                   flash_ms=summarize(res["flash"]), calls_per_window=res["calls"])
        row["flash_over_eager"] = row["flash_ms"]["median"] / row["eager_ms"]["median"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--windows", type=int, default=5, help="alternating windows per side")
    ap.add_argument("--calls", type=int, default=50, help="least timed calls per window")
    ap.add_argument("--window-ms", type=float, default=100.0,
                    help="least duration of a timed window; 0 times exactly --calls calls")
    ap.add_argument("--warm", type=int, default=5, help="warm calls before each window")
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--out", default=None, help="also write all rows to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_t5_attention: needs a GPU (no timing without one)")
    rows = []
    for shape in SHAPES:
        rows += bench_shape(*shape, args)
    for shape in SHAPES[:3]:
        rows += bench_bias_cost(*shape, args)
    if not args.skip_model:
        rows += bench_model(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
