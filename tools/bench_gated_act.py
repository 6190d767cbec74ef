"""A/B of the gated MLP activation ``act(g) * u``: the eager lines of ``MLP`` /
``T5FFN`` (``reference.gated_act``: slice views, activation, multiply, and
autograd's backward of them) against ``ops.gated_act`` (csrc/gated_act.hip), at
the shapes of Llama-2-7B and Flan-T5-large, bf16.

Old, new and a plain ``copy_`` of the same byte count alternate window by window
in this one process, so drift of the box hits all alike; the range over the
windows is printed next to the median.  A window is as many calls between two
device events as fill ``--window-s`` seconds (calibrated per variant after the
warm-up), and successive calls walk over as many distinct inputs as it takes to
exceed ``--footprint-mb``, so a call finds its input neither in L2 nor in the
memory-side cache.  Bytes are the algorithm's: 3 N I elements forward, 5 N I
backward; the copy moves the same count (half read, half written) and is the
yardstick the kernel is judged against.  Calls are plain launches, not graph
replays: at the decode shape (N=128) the host's launch cost is inside every
figure, the eager ones (two forward kernels) as well as the new one.

The last column block is ``torch.cuda.max_memory_allocated`` over one forward +
backward of a whole MLP module with ``TRLX_AMD_FUSED_GATED_ACT`` off and on.

    python tools/bench_gated_act.py [--out profiles/gated_act.json]

Needs a GPU: there is no CPU fallback for a timing."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from trlx_amd import ops  # noqa: E402
from trlx_amd.models.nn.config import TransformerConfig  # noqa: E402
from trlx_amd.models.nn.seq2seq import Seq2SeqConfig, T5FFN  # noqa: E402
from trlx_amd.models.nn.transformer import MLP  # noqa: E402
from trlx_amd.ops import reference  # noqa: E402

# (name, N tokens, I, hidden size, act, fused layout)
SHAPES = [
    ("llama2-7b N=8192", 8192, 11008, 4096, "silu", True),
    ("llama2-7b decode N=128", 128, 11008, 4096, "silu", True),
    ("llama2-7b TP=2 shard N=8192", 8192, 5504, 4096, "silu", True),
    ("flan-t5-large N=32*512", 32 * 512, 2816, 1024, "gelu_new", False),
]
ELT = 2  # bf16


def timed_windows(variants, args):
    """{name: [seconds per call, one per window]} for callables taking the call
    index; the variants alternate window by window."""
    calls = {}
    for name, fn in variants.items():
        for i in range(args.warm):
            fn(i)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for i in range(args.warm):
            fn(i)
        stop.record()
        stop.synchronize()
        per_call = start.elapsed_time(stop) * 1e-3 / args.warm
        calls[name] = max(args.warm, int(args.window_s / per_call) + 1)
    times = {name: [] for name in variants}
    for _ in range(args.windows):
        for name, fn in variants.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for i in range(calls[name]):
                fn(i)
            stop.record()
            stop.synchronize()
            times[name].append(start.elapsed_time(stop) * 1e-3 / calls[name])
    return times


def module_peak_mb(name, N, I, hidden, fused, flag):
    """Peak allocation above the resident weights and input over one forward +
    backward of the model's MLP module, switch off or on."""
    os.environ.pop("TRLX_AMD_FUSED_GATED_ACT", None)
    if flag:
        os.environ["TRLX_AMD_FUSED_GATED_ACT"] = "1"
    torch.manual_seed(0)
    if fused:
        module = MLP(TransformerConfig(vocab_size=8, hidden_size=hidden, num_layers=1,
                                       num_heads=1, intermediate_size=I, activation="silu",
                                       swiglu=True, mlp_bias=False, arch_name="llama"))
    else:
        module = T5FFN(Seq2SeqConfig(d_model=hidden, d_ff=I, feed_forward_proj="gated-gelu"))
    module = module.cuda().bfloat16()
    x = torch.randn(N, hidden, device="cuda").bfloat16().requires_grad_()
    dy = torch.randn(N, hidden, device="cuda").bfloat16()
    for _ in range(2):
        module(x).backward(dy)
    module.zero_grad(set_to_none=False)
    x.grad.zero_()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    module(x).backward(dy)
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 2**20
    os.environ.pop("TRLX_AMD_FUSED_GATED_ACT", None)
    return peak


def bench_shape(name, N, I, hidden, act, fused, args):
    gen = torch.Generator(device="cuda").manual_seed(0)
    width = 2 * I if fused else I
    per_input = N * 2 * I * ELT
    copies = max(2, -(-args.footprint_mb * 2**20 // per_input))

    def rand(*shape):
        return torch.randn(*shape, device="cuda", generator=gen).bfloat16()

    inputs = [tuple(rand(N, width).requires_grad_() for _ in range(1 if fused else 2))
              for _ in range(copies)]
    dh = rand(N, I)
    # the copies that move 3 N I (forward) and 8 N I (forward + backward) elements
    src = [rand(N, 4 * I) for _ in range(max(2, copies // 2))]
    dst = torch.empty_like(src[0])

    def old(i):
        return reference.gated_act(*inputs[i % copies], act=act)

    def new(i):
        return ops.gated_act(*inputs[i % copies], act=act)

    def with_bwd(fn):
        def call(i):
            return torch.autograd.grad(fn(i), inputs[i % copies], dh)
        return call

    def no_grad(fn):
        def call(i):
            with torch.no_grad():
                return fn(i)
        return call

    def copy(elements):  # moves 2 * elements: one read, one write, both contiguous
        def call(i):
            dst.view(-1)[:elements].copy_(src[i % len(src)].view(-1)[:elements])
        return call

    with torch.no_grad():
        diff = float((new(0).float() - old(0).float()).abs().max())
    fwd = timed_windows({"old": no_grad(old), "new": no_grad(new), "copy": copy(3 * N * I // 2)},
                        args)
    both = timed_windows({"old": with_bwd(old), "new": with_bwd(new), "copy": copy(4 * N * I)},
                         args)
    del inputs, src, dst
    torch.cuda.empty_cache()
    row = {"shape": name, "N": N, "I": I, "act": act, "fused": fused, "inputs": copies,
           "max_abs_diff_new_vs_old": diff, "fwd": {}, "fwd_bwd": {},
           "module_peak_mb": {"old": module_peak_mb(name, N, I, hidden, fused, False),
                              "new": module_peak_mb(name, N, I, hidden, fused, True)}}
    for key, times, elements in (("fwd", fwd, 3), ("fwd_bwd", both, 8)):
        for variant, t in times.items():
            med = statistics.median(t)
            row[key][variant] = {"us": med * 1e6, "min_us": min(t) * 1e6, "max_us": max(t) * 1e6,
                                 "gb_per_s": elements * N * I * ELT / med / 1e9}
    print(f"{name}: " + "  ".join(
        f"{key} old {row[key]['old']['us']:.1f} new {row[key]['new']['us']:.1f} "
        f"copy {row[key]['copy']['us']:.1f} us" for key in ("fwd", "fwd_bwd"))
        + f"  peak MB old {row['module_peak_mb']['old']:.0f} new {row['module_peak_mb']['new']:.0f}",
        flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.4)
    ap.add_argument("--footprint-mb", type=int, default=768)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_gated_act needs a GPU")
    ops._require_ext("bench_gated_act")
    rows = [bench_shape(*shape, args) for shape in SHAPES]
    result = {"windows": args.windows, "window_s": args.window_s,
              "footprint_mb": args.footprint_mb, "device": torch.cuda.get_device_name(0),
              "shapes": rows}
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
