"""A/B of decode attention for models that share KV heads: the block-per-query-
head kernel (``ops.attention_decode(grouped=False)``, csrc/attn_decode.hip)
against the grouped-query kernel (``grouped=True``, csrc/attn_decode_gqa.hip),
the latter with the key-split heuristic (``num_splits=0``) and with forced
split counts.

Both kernels run in this one process on the same inputs, alternating window by
window (old, new ns=0, new ns=1, ..., old, ...), so drift of the box hits all
alike; the range over the windows is printed next to the median.  Successive
calls walk over as many distinct caches ("layers") as it takes to exceed
``--footprint-mb``, so a call finds its K/V neither in L2 nor in the memory-side
cache, as a decode step over a whole model does not.  One pass over the layers
is captured into a graph per variant, as the decode engine captures its step,
so the host's launch cost stays out of the kernels' times; a window is as many
replays between two device events as make ``--calls`` launches.

    python tools/bench_gqa_decode.py [--out profiles/gqa_decode.json]

Needs a GPU: there is no CPU fallback for a timing."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from trlx_amd import ops  # noqa: E402

# (name, B, Hq, Hkv, D, T): T keys allocated and visible in every row
SHAPES = [
    ("santacoder T=256 ", 128, 16, 1, 128, 256),
    ("santacoder T=1024", 128, 16, 1, 128, 1024),
    ("llama G=4 T=1024 ", 32, 32, 8, 128, 1024),
    ("llama G=8 T=1024 ", 32, 32, 4, 128, 1024),
    ("llama G=8 B=16 T=2048", 16, 32, 4, 128, 2048),
    ("llama G=8 B=4 T=2048", 4, 32, 4, 128, 2048),
    ("llama G=8 B=1 T=4096", 1, 32, 4, 128, 4096),
]
SPLITS = (0, 1, 2, 4, 8, 16)


def bench_shape(name, B, Hq, Hkv, D, T, args):
    g = torch.Generator(device="cuda").manual_seed(0)
    cache_bytes = 2 * B * Hkv * T * D * 2
    layers = max(2, -(-args.footprint_mb * 2**20 // cache_bytes))
    q = torch.randn(B, Hq, 1, D, device="cuda", generator=g).bfloat16()
    caches = [(torch.randn(B, Hkv, T, D, device="cuda", generator=g).bfloat16(),
               torch.randn(B, Hkv, T, D, device="cuda", generator=g).bfloat16())
              for _ in range(layers)]
    lens = torch.full((B,), T, dtype=torch.int32, device="cuda")
    scale = D ** -0.5

    def run(variant, i):
        k, v = caches[i % layers]
        if variant == "old":
            return ops.attention_decode(q, k, v, lens, scale, grouped=False)
        return ops.attention_decode(q, k, v, lens, scale, grouped=True, num_splits=variant)

    variants = ["old"] + list(SPLITS)
    ref = run("old", 0).float()
    diff = {str(v): float((run(v, 0).float() - ref).abs().max()) for v in SPLITS}
    graphs = {}
    side = torch.cuda.Stream()
    for v in variants:
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for i in range(layers):
                run(v, i)
        torch.cuda.current_stream().wait_stream(side)
        graphs[v] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[v]):
            keep = [run(v, i) for i in range(layers)]  # noqa: F841 - the graph owns them
        for _ in range(args.warm):
            graphs[v].replay()
    torch.cuda.synchronize()
    replays = -(-args.calls // layers)
    times = {str(v): [] for v in variants}
    for _ in range(args.windows):
        for v in variants:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(replays):
                graphs[v].replay()
            stop.record()
            stop.synchronize()
            times[str(v)].append(start.elapsed_time(stop) * 1e3 / (replays * layers))
    row = {"shape": name.strip(), "B": B, "Hq": Hq, "Hkv": Hkv, "D": D, "T": T, "layers": layers,
           "kv_mb_per_call": cache_bytes / 2**20, "max_abs_diff_vs_old": diff, "us": {}}
    for v in variants:
        t = times[str(v)]
        row["us"][str(v)] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
    old = row["us"]["old"]["median"]
    print(f"{name}  old {old:8.1f} us  " + "  ".join(
        f"ns={v} {row['us'][str(v)]['median']:8.1f}" for v in SPLITS), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--footprint-mb", type=int, default=768)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_gqa_decode needs a GPU")
    ops._require_ext("bench_gqa_decode")
    rows = [bench_shape(*shape, args) for shape in SHAPES]
    result = {"calls": args.calls, "windows": args.windows, "footprint_mb": args.footprint_mb,
              "device": torch.cuda.get_device_name(0), "shapes": rows}
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
