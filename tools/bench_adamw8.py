"""A/B of the optimizer step kernels: ``fused_adamw8`` (csrc/adamw8.hip, e4m3
moment codes) against ``fused_adamw`` (csrc/adamw.hip, fp32 moments), and each
against a plain ``copy_`` that moves the same byte count, on one flat arena of
bf16 params and grads: gpt2 (124 M), gpt2-xl (1.5 B) and the shard one of 8
ZeRO ranks holds of a 6 B model (756 M).

The variants alternate window by window in this one process, so drift of the
box hits all alike; the range over the windows is printed next to the median.
A window is as many calls between two device events as fill ``--window-s``
seconds (calibrated per variant after the warm-up).  Every arena is far larger
than L2 and the memory-side cache (the smallest moves 2 GB per call), so a call
finds nothing of the previous one cached.  Bytes are the algorithm's, per
parameter: 28 for fused_adamw (g 2, m 4+4, v 4+4, master 4+4, p 2), 16 + 1/16
for fused_adamw8 (g 2, m8 1+1, u8 1+1, master 4+4, p 2, two scales per 256 read
and written); a copy moves half of its count in and half out.

    python tools/bench_adamw8.py [--out profiles/adamw8.json]

Needs a GPU: there is no CPU fallback for a timing."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from trlx_amd import ops  # noqa: E402

ARENAS = [("gpt2 124M", 124_439_808), ("gpt2-xl 1.5B", 1_557_611_200),
          ("6B / 8 ZeRO ranks", 756_000_000)]
BYTES = {"adamw": 28.0, "adamw8": 16.0 + 1.0 / 16}
HYPER = (1e-5, 0.9, 0.95, 1e-8, 1e-6, 1.0)  # lr, betas, eps, weight decay, grad scale


def timed_windows(variants, args):
    """{name: [seconds per call, one per window]}; the variants alternate window
    by window."""
    def window(fn, calls):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(calls):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e-3 / calls

    calls = {}
    for name, fn in variants.items():
        window(fn, args.warm)
        calls[name] = max(args.warm, int(args.window_s / window(fn, args.warm)) + 1)
    times = {name: [] for name in variants}
    for _ in range(args.windows):
        for name, fn in variants.items():
            times[name].append(window(fn, calls[name]))
    return times


def bench_arena(name, n, args, ext):
    gen = torch.Generator(device="cuda").manual_seed(0)
    p = torch.randn(n, device="cuda", generator=gen, dtype=torch.bfloat16)
    g = torch.randn(n, device="cuda", generator=gen, dtype=torch.bfloat16) * 1e-2
    master = p.float()
    m, v = torch.zeros_like(master), torch.zeros_like(master)
    nb = -(-n // ops.ADAMW8_QB)
    m8, u8 = (torch.zeros(n, device="cuda", dtype=torch.uint8) for _ in range(2))
    m_scale, u_scale = (torch.zeros(nb, device="cuda") for _ in range(2))
    # as large as the larger copy needs: half of fused_adamw's bytes each
    src, dst = (torch.zeros(int(max(BYTES.values()) * n / 2), device="cuda", dtype=torch.uint8)
                for _ in range(2))
    step = [0]

    def adamw():
        step[0] += 1
        ext.fused_adamw(p, master, g, m, v, step[0], *HYPER)

    def adamw8():
        step[0] += 1
        ext.fused_adamw8(p, master, g, m8, m_scale, u8, u_scale, step[0], *HYPER, 0, 0)

    def copy(total_bytes):  # half read, half written, both contiguous
        half = int(total_bytes * n / 2)
        assert half <= src.numel()
        return lambda: dst[:half].copy_(src[:half])

    variants = {"adamw": adamw, "adamw8": adamw8}
    variants.update({f"copy_{k}": copy(b) for k, b in BYTES.items()})
    times = timed_windows(variants, args)
    row = {"arena": name, "n": n}
    for variant, t in times.items():
        med = statistics.median(t)
        per_param = BYTES[variant.replace("copy_", "")]
        row[variant] = {"us": med * 1e6, "min_us": min(t) * 1e6, "max_us": max(t) * 1e6,
                        "gb_per_s": per_param * n / med / 1e9}
    print(f"{name}: " + "  ".join(
        f"{k} {row[k]['us']:.0f} us ({row[k]['gb_per_s']:.0f} GB/s)" for k in variants),
        flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_adamw8 needs a GPU")
    ext = ops._require_ext("bench_adamw8")
    rows = []
    for name, n in ARENAS:
        rows.append(bench_arena(name, n, args, ext))
        torch.cuda.empty_cache()
    result = {"windows": args.windows, "window_s": args.window_s,
              "device": torch.cuda.get_device_name(0), "arenas": rows}
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
