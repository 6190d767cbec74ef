"""A/B of decode attention on the fp8 KV cache (csrc/attn_decode_fp8.hip) against
the bf16 kernels that serve the same shape today: the block-per-query-head
kernel (``grouped=False``) and, where Hq > Hkv, the grouped-query kernel
(``grouped=True``).  Also times ``kv_store_fp8`` alone and a plain device copy
of the fp8 cache's bytes, the yardstick for its effective GB/s.

All variants run in this one process on caches of the same values, alternating
window by window, so drift of the box hits all alike; the range over the windows
is printed next to the median.  Successive calls walk over as many distinct
caches ("layers") as it takes to exceed ``--footprint-mb``, so a call finds its
K/V neither in L2 nor in the memory-side cache.  One pass over the layers is
captured into a graph per variant, as the decode engine captures its step.

    python tools/bench_kv_fp8.py [--out profiles/kv_fp8.json]

Needs a GPU: there is no CPU fallback for a timing."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from trlx_amd import ops  # noqa: E402
from trlx_amd.ops import reference  # noqa: E402

# (name, B, Hq, Hkv, D, S): S keys allocated and visible in every row
SHAPES = [
    ("llama2-7b S=256 ", 128, 32, 32, 128, 256),
    ("llama2-7b S=1024", 128, 32, 32, 128, 1024),
    ("llama G=4 S=1024", 128, 32, 8, 128, 1024),
    ("llama G=8 S=1024", 128, 32, 4, 128, 1024),
]
# kv_store_fp8 alone: (name, B, Hkv, D, T new tokens, S)
STORE_SHAPES = [("prefill T=512", 128, 32, 128, 512, 1024), ("decode T=1", 128, 32, 128, 1, 1024)]


def timed(variants, layers, args):
    """{variant: [us per call, one per window]}: ``variants`` maps a name to
    run(i), graphs of one pass over the layers replayed alternately."""
    graphs = {}
    side = torch.cuda.Stream()
    for name, run in variants.items():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for i in range(layers):
                run(i)
        torch.cuda.current_stream().wait_stream(side)
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            keep = [run(i) for i in range(layers)]  # noqa: F841 - the graph owns them
        for _ in range(args.warm):
            graphs[name].replay()
    torch.cuda.synchronize()
    replays = -(-args.calls // layers)
    times = {name: [] for name in variants}
    for _ in range(args.windows):
        for name in variants:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(replays):
                graphs[name].replay()
            stop.record()
            stop.synchronize()
            times[name].append(start.elapsed_time(stop) * 1e3 / (replays * layers))
    return {n: {"median": statistics.median(t), "min": min(t), "max": max(t)}
            for n, t in times.items()}


def bench_attention(name, B, Hq, Hkv, D, S, args):
    g = torch.Generator(device="cuda").manual_seed(0)
    fp8_bytes = 2 * B * Hkv * S * (D + 4)
    layers = max(2, -(-args.footprint_mb * 2**20 // fp8_bytes))
    q = torch.randn(B, Hq, 1, D, device="cuda", generator=g).bfloat16()
    bf, f8 = [], []
    for _ in range(layers):
        k, v = (torch.randn(B, Hkv, S, D, device="cuda", generator=g).bfloat16() for _ in range(2))
        bf.append((k, v))
        f8.append(reference.kv_quantize_fp8(k) + reference.kv_quantize_fp8(v))
    dst = [torch.empty(fp8_bytes, dtype=torch.uint8, device="cuda") for _ in range(layers)]
    src = [torch.empty(fp8_bytes, dtype=torch.uint8, device="cuda") for _ in range(layers)]
    lens = torch.full((B,), S, dtype=torch.int32, device="cuda")
    scale = D ** -0.5

    def fp8(i):
        k8, ks, v8, vs = f8[i % layers]
        return ops.attention_decode(q, k8, v8, lens, scale, k_scale=ks, v_scale=vs)

    variants = {
        "fp8": fp8,
        "bf16": lambda i: ops.attention_decode(q, *bf[i % layers], lens, scale, grouped=False),
        "copy": lambda i: dst[i % layers].copy_(src[i % layers]),
    }
    if Hq > Hkv:
        variants["bf16_gqa"] = lambda i: ops.attention_decode(q, *bf[i % layers], lens, scale,
                                                              grouped=True)
    diff = float((fp8(0).float() - variants["bf16"](0).float()).abs().max())
    us = timed(variants, layers, args)
    row = {"shape": name.strip(), "B": B, "Hq": Hq, "Hkv": Hkv, "D": D, "S": S, "layers": layers,
           "fp8_mb_per_call": fp8_bytes / 2**20, "max_abs_diff_vs_bf16": diff, "us": us,
           "fp8_gbps": fp8_bytes / us["fp8"]["median"] / 1e3,
           "copy_gbps": fp8_bytes / us["copy"]["median"] / 1e3}
    for other in ("bf16", "bf16_gqa"):
        if other in us:
            row[f"speedup_vs_{other}"] = us[other]["median"] / us["fp8"]["median"]
    print(f"{name}  " + "  ".join(
        f"{n} {t['median']:8.1f} us [{t['min']:.1f}, {t['max']:.1f}]" for n, t in us.items())
        + f"  fp8 {row['fp8_gbps']:.0f} GB/s vs copy {row['copy_gbps']:.0f} GB/s", flush=True)
    return row


def bench_store(name, B, Hkv, D, T, S, args):
    g = torch.Generator(device="cuda").manual_seed(1)
    moved = 2 * B * Hkv * T * (2 * D + D + 4)  # bf16 in, codes and scale out
    layers = max(2, min(64, -(-args.footprint_mb * 2**20 // moved)))
    rows = [tuple(torch.randn(B, Hkv, T, D, device="cuda", generator=g).bfloat16()
                  for _ in range(2)) for _ in range(layers)]
    k8, v8 = (torch.zeros(B, Hkv, S, D, dtype=torch.uint8, device="cuda") for _ in range(2))
    ks, vs = (torch.zeros(B, Hkv, S, device="cuda") for _ in range(2))
    idx = torch.zeros(1, dtype=torch.long, device="cuda")
    us = timed({"store": lambda i: ops.kv_store_fp8(*rows[i % layers], k8, ks, v8, vs,
                                                    idx if T == 1 else 0)}, layers, args)
    row = {"shape": name, "B": B, "Hkv": Hkv, "D": D, "T": T, "S": S, "layers": layers,
           "us": us, "gbps": moved / us["store"]["median"] / 1e3}
    print(f"kv_store_fp8 {name}: {us['store']['median']:.1f} us "
          f"[{us['store']['min']:.1f}, {us['store']['max']:.1f}]  {row['gbps']:.0f} GB/s", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--footprint-mb", type=int, default=768)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_kv_fp8 needs a GPU")
    ops._require_ext("bench_kv_fp8")
    result = {"calls": args.calls, "windows": args.windows, "footprint_mb": args.footprint_mb,
              "device": torch.cuda.get_device_name(0),
              "attention": [bench_attention(*s, args) for s in SHAPES],
              "store": [bench_store(*s, args) for s in STORE_SHAPES]}
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
