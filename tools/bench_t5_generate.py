"""Three-way A/B of T5 generation (Seq2SeqTransformer.generate) and the price of
the self-attention decode kernel against the causal one.

Sides, all in this one process on the same prompts, alternating window by
window so drift of the box hits them alike:

    (a) eager   today's ``past`` loop                (TRLX_AMD_NO_S2S_DECODE=1)
    (b) kernel  decode_step in a plain Python loop   (TRLX_AMD_NO_GRAPHS=1)
    (c) graph   Seq2SeqDecodeEngine, one replay per token

The model is the t5-small-sized random model of profiles/t5_attention_notes.md
§3 in bf16, prompts of 128 tokens with every other row left-padded by 16.
``eos_token_id`` is an id outside the vocabulary (``None`` would mean the
config's), so every side runs all ``max_new_tokens`` steps.  Times are device
events around a window of generate calls after ``--warm`` warm calls; a window
lasts at least ``--window-ms``; the median and the range over ``--windows``
windows are printed, and a difference inside a side's own range is not one.

Then ``ops.seq2seq_decode_attention`` (in-kernel append, optional bias) against
``ops.attention_decode`` at the same (B, H, S, D): the ratio is the price of
the append and of the bias.

    python tools/bench_t5_generate.py [--out profiles/t5_generate.json]

Needs a GPU: there is no CPU fallback for a timing."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from trlx_amd import ops  # noqa: E402

DEV = "cuda"
SIDES = {
    "eager": {"TRLX_AMD_NO_S2S_DECODE": "1"},
    "kernel": {"TRLX_AMD_NO_GRAPHS": "1"},
    "graph": {},
}
SWITCHES = ("TRLX_AMD_NO_S2S_DECODE", "TRLX_AMD_NO_GRAPHS")


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


def alternate(sides, windows, calls, warm, window_ms):
    """sides: {name: fn}; {name: [ms per call, one per window]} and the calls
    per window: enough for the FASTEST side's window to last ``window_ms``."""
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


def bench_generate(model, cfg, B, new_tokens, args):
    torch.manual_seed(B + new_tokens)
    ids = torch.randint(2, cfg.vocab_size, (B, 128), device=DEV)
    mask = torch.ones_like(ids)
    mask[::2, :16] = 0
    kw = dict(max_new_tokens=new_tokens, do_sample=True, seed=0, eos_token_id=cfg.vocab_size)

    def side(env):
        def run():
            for name in SWITCHES:
                os.environ.pop(name, None)
            os.environ.update(env)
            out = model.generate(ids, mask, **kw)
            assert out.shape == (B, 1 + new_tokens), out.shape
        return run

    fns = {name: side(env) for name, env in SIDES.items()}
    res = alternate(fns, args.windows, 1, args.warm, args.window_ms)
    for name in SWITCHES:
        os.environ.pop(name, None)
    row = dict(kind="generate", B=B, new_tokens=new_tokens, calls_per_window=res["calls"])
    for name in SIDES:
        row[f"{name}_ms"] = summarize(res[name])
    for name in ("kernel", "graph"):
        row[f"{name}_over_eager"] = row[f"{name}_ms"]["median"] / row["eager_ms"]["median"]
    print(json.dumps(row), flush=True)
    return [row]


def bench_self_step(B, H, S, D, args):
    """The self step at the last cache slot against attention_decode over the
    same S keys, without and with the bias."""
    torch.manual_seed(0)
    q, kn, vn = (torch.randn(B, H, D, device=DEV).mul_(0.5).bfloat16() for _ in range(3))
    kc, vc = (torch.randn(B, H, S, D, device=DEV).mul_(0.5).bfloat16() for _ in range(2))
    q4 = q.view(B, H, 1, D)
    idx = torch.full((1,), S - 1, dtype=torch.long, device=DEV)
    lens = torch.full((B,), S, dtype=torch.int32, device=DEV)
    vec, zero = ops.t5_rel_bias(torch.randn(32, H, device=DEV), 1, 1, S - 1, False)
    sides = {
        "attention_decode": lambda: ops.attention_decode(q4, kc, vc, lens, 1.0),
        "s2s_append": lambda: ops.seq2seq_decode_attention(q, kn, vn, kc, vc, idx),
        "s2s_append_bias": lambda: ops.seq2seq_decode_attention(q, kn, vn, kc, vc, idx, vec, zero),
    }
    res = alternate(sides, args.windows, 200, args.warm, args.window_ms)
    row = dict(kind="self_step", B=B, H=H, S=S, D=D, calls_per_window=res["calls"])
    for name in sides:
        row[f"{name}_us"] = {k: v * 1e3 for k, v in summarize(res[name]).items()}
    base = row["attention_decode_us"]["median"]
    row["append_over_decode"] = row["s2s_append_us"]["median"] / base
    row["append_bias_over_decode"] = row["s2s_append_bias_us"]["median"] / base
    print(json.dumps(row), flush=True)
    return [row]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--windows", type=int, default=5, help="alternating windows per side")
    ap.add_argument("--window-ms", type=float, default=100.0,
                    help="least duration of a timed window")
    ap.add_argument("--warm", type=int, default=5, help="warm calls before each window")
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--new-tokens", type=int, nargs="+", default=[25, 50])
    ap.add_argument("--out", default=None, help="also write all rows to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_t5_generate: needs a GPU (no timing without one)")
    from trlx_amd.models.nn.generation import release_graphs
    from trlx_amd.models.nn.seq2seq import Seq2SeqConfig, Seq2SeqTransformer

    torch.manual_seed(0)
    cfg = Seq2SeqConfig()  # t5-small: d_model 512, 8 heads x 64, 6 + 6 layers
    model = Seq2SeqTransformer(cfg).to(DEV).bfloat16().eval()
    rows = []
    for B in args.batches:
        for new_tokens in args.new_tokens:
            rows += bench_generate(model, cfg, B, new_tokens, args)
            release_graphs()
    for B in args.batches:
        for D in (64, 128):
            rows += bench_self_step(B, 8, 50, D, args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
