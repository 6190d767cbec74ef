"""A/B of the LoRA linear: the eager lines of ``LoRALinear`` (base GEMM, two
rank-r GEMMs, scalar multiply, add, and autograd's backward of them) against
``ops.lora_linear`` (csrc/lora.hip), bf16, at the four projections of Llama-2-7B
with N = 8192 tokens and ranks 8, 16 and 64, and at the decode batch N = 128.

Both variants contain the same library base GEMM (and, backward, the same
``dY @ W``), so ``old - new`` is what the adapter path saves and ``old / new`` is
the whole projection.  The adapter alone is also timed: ``new`` minus a bare
``F.linear`` (forward) is set against a plain ``copy_`` that moves the bytes the
kernels must move (forward: X once, Y read and written).

Old, new, the bare base and the copy alternate window by window in one process;
the range over the windows is printed next to the median.  A window is as many
calls between two device events as fill ``--window-s`` seconds, and successive
calls walk over as many distinct inputs as it takes to exceed
``--footprint-mb``.  Calls are plain launches, not graph replays: at N = 128 the
host's launch cost is inside every figure.

    python tools/bench_lora.py [--out profiles/lora.json] [--ranks 8 16 64]

Needs a GPU: there is no CPU fallback for a timing."""

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from trlx_amd import ops  # noqa: E402
from trlx_amd.ops import reference  # noqa: E402

# Llama-2-7B: (projection, in features K, out features O)
PROJECTIONS = [("qkv_proj", 4096, 12288), ("o_proj", 4096, 4096),
               ("gate_up_proj", 4096, 22016), ("down_proj", 11008, 4096)]
TOKENS = [8192, 128]
ELT = 2  # bf16


def timed_windows(variants, args):
    """{name: [seconds per call, one per window]}; the variants alternate."""
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


def bench_shape(proj, K, O, N, r, args):
    gen = torch.Generator(device="cuda").manual_seed(0)

    def rand(*shape, scale=1.0):
        return (torch.randn(*shape, device="cuda", generator=gen) * scale).bfloat16()

    copies = max(2, -(-args.footprint_mb * 2**20 // (N * (K + O) * ELT)))
    xs = [rand(N, K).requires_grad_() for _ in range(copies)]
    dy = rand(N, O)
    W = rand(O, K, scale=K ** -0.5)
    A = rand(r, K, scale=K ** -0.5).requires_grad_()
    B = rand(O, r, scale=r ** -0.5).requires_grad_()
    scaling = 2.0
    # the bytes the adapter kernels must move: forward X + 2 Y; backward dY + 2 dX
    fwd_elems, bwd_elems = N * (K + 2 * O), N * (O + 2 * K)
    src = [rand((fwd_elems + bwd_elems) // 2 + 8) for _ in range(2)]
    dst = torch.empty_like(src[0])

    def old(i):
        return reference.lora_linear(xs[i % copies], W, None, A, B, scaling)

    def new(i):
        return ops.lora_linear(xs[i % copies], W, None, A, B, scaling)

    def base(i):
        return F.linear(xs[i % copies], W)

    def with_bwd(fn, leaves):
        def call(i):
            return torch.autograd.grad(fn(i), [xs[i % copies], *leaves], dy)
        return call

    def no_grad(fn):
        def call(i):
            with torch.no_grad():
                return fn(i)
        return call

    def copy(elements):  # moves `elements`: half read, half written
        def call(i):
            dst[:elements // 2].copy_(src[i % 2][:elements // 2])
        return call

    with torch.no_grad():
        diff = float((new(0).float() - old(0).float()).abs().max())
    fwd = timed_windows({"old": no_grad(old), "new": no_grad(new), "base": no_grad(base),
                         "copy": copy(fwd_elems)}, args)
    both = timed_windows({"old": with_bwd(old, [A, B]), "new": with_bwd(new, [A, B]),
                          "base": with_bwd(base, []), "copy": copy(fwd_elems + bwd_elems)}, args)
    row = {"proj": proj, "N": N, "K": K, "O": O, "r": r, "inputs": copies,
           "max_abs_diff_new_vs_old": diff, "fwd": {}, "fwd_bwd": {}}
    for key, times, elements in (("fwd", fwd, fwd_elems), ("fwd_bwd", both, fwd_elems + bwd_elems)):
        for variant, t in times.items():
            med = statistics.median(t)
            row[key][variant] = {"us": med * 1e6, "min_us": min(t) * 1e6, "max_us": max(t) * 1e6}
        adapter = {v: row[key][v]["us"] - row[key]["base"]["us"] for v in ("old", "new")}
        row[key]["adapter_us"] = adapter
        row[key]["adapter_gb_per_s"] = {v: elements * ELT / max(adapter[v], 1e-3) / 1e3
                                        for v in adapter}
        row[key]["copy_gb_per_s"] = elements * ELT / row[key]["copy"]["us"] / 1e3
        row[key]["old_over_new"] = row[key]["old"]["us"] / row[key]["new"]["us"]
    print(f"{proj} N={N} r={r}: " + "  ".join(
        f"{key} old {row[key]['old']['us']:.1f} new {row[key]['new']['us']:.1f} base "
        f"{row[key]['base']['us']:.1f} copy {row[key]['copy']['us']:.1f} us "
        f"({row[key]['old_over_new']:.2f}x)" for key in ("fwd", "fwd_bwd")), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--footprint-mb", type=int, default=768)
    ap.add_argument("--ranks", type=int, nargs="+", default=[8, 16, 64])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_lora needs a GPU")
    ops._require_ext("bench_lora")
    rows = []
    for N in TOKENS:
        for proj, K, O in PROJECTIONS:
            for r in args.ranks:
                rows.append(bench_shape(proj, K, O, N, r, args))
                torch.cuda.empty_cache()
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
