#!/usr/bin/env python
"""Compare two gfx950 assembly files kernel by kernel.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S ... -o old.s   (parent)
    hipcc ...                                                            -o new.s   (this tree)
    python tools/isa_diff.py old.s new.s [--map map.json] [--mask-sgprs]

Kernels are paired by demangled name without the argument list (c++filt or
llvm-cxxfilt when one is on PATH, the mangled name otherwise).  ``--map`` names
a JSON list of ``[regex, replacement]`` pairs applied to the OLD names first,
for kernels that were renamed or merged, e.g.
``["rmsnorm_fwd_wave_kernel<(\\\\w+), ", "norm_fwd_kernel<\\\\1, WaveRows, false, false, "]``.

Per kernel the instruction stream is taken without comments and directives,
the kernel's own symbol becomes ``KERNEL`` and branch labels are renumbered in
order of appearance, so a kernel that merely moved inside the file compares
equal.  Output per pair: ``identical``, or both instruction counts and a
unified diff; then the resources the code object header records (VGPRs, SGPRs,
static LDS bytes, scratch bytes).  ``--mask-sgprs`` replaces scalar register
numbers by ``s#`` on both sides: what then remains differs in more than the
scalar register allocation.  Exit status 1 when any pair differs or is unpaired.
"""

import argparse
import difflib
import json
import re
import shutil
import subprocess
import sys

RESOURCES = {
    "vgpr": ".amdhsa_next_free_vgpr",
    "sgpr": ".amdhsa_next_free_sgpr",
    "lds": ".amdhsa_group_segment_fixed_size",
    "scratch": ".amdhsa_private_segment_fixed_size",
}
LABEL = re.compile(r"\.LBB\d+_\d+")
SGPR = re.compile(r"\bs(\d+|\[\d+:\d+\])")


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True,
                         check=True).stdout.splitlines()
    return dict(zip(names, out))


def without_args(name):
    """'void ns::k<int, true>(float*, int)' -> 'ns::k<int, true>'."""
    if name.endswith(")"):
        depth = 0
        for i in range(len(name) - 1, -1, -1):
            depth += {")": 1, "(": -1}.get(name[i], 0)
            if depth == 0:
                name = name[:i]
                break
    return name.split(" ", 1)[1] if name.startswith("void ") else name


def kernels(path):
    """{mangled name: (instruction lines, resources)} for every .amdhsa_kernel."""
    lines = open(path).read().splitlines()
    found = {}
    for i, line in enumerate(lines):
        if line.strip().startswith(".amdhsa_kernel "):
            sym = line.split()[1]
            res = {}
            for meta in lines[i + 1:]:
                word = meta.split()
                if word and word[0] == ".end_amdhsa_kernel":
                    break
                for key, directive in RESOURCES.items():
                    if word and word[0] == directive:
                        res[key] = int(word[1], 0)
            found[sym] = res
    out = {}
    for sym, res in found.items():
        start = next(i for i, line in enumerate(lines) if line.startswith(sym + ":"))
        body, labels = [], {}
        for line in lines[start + 1:]:
            if line.startswith(".Lfunc_end"):
                break
            code = line.split(";", 1)[0].rstrip()
            if not code.strip() or (code.lstrip().startswith(".") and not LABEL.match(code)):
                continue
            code = code.replace(sym, "KERNEL")
            code = LABEL.sub(lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), code)
            body.append(" ".join(code.split()))
        out[sym] = (body, res)
    return out


def by_name(path, renames=()):
    ks = kernels(path)
    names = demangle(list(ks))
    out = {}
    for sym, val in ks.items():
        name = without_args(names[sym])
        for pattern, repl in renames:
            name = re.sub(pattern, repl, name)
        assert name not in out, f"{path}: two kernels named {name}"
        out[name] = val
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--map", help="JSON list of [regex, replacement] applied to the old names")
    ap.add_argument("--mask-sgprs", action="store_true")
    args = ap.parse_args()
    renames = json.load(open(args.map)) if args.map else []
    old, new = by_name(args.old, renames), by_name(args.new)
    differ = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print(f"{name}: only in {args.new if name in new else args.old}")
            differ += 1
            continue
        (a, ra), (b, rb) = old[name], new[name]
        if args.mask_sgprs:
            a, b = ([SGPR.sub("s#", line) for line in side] for side in (a, b))
        res = " ".join(f"{k} {ra.get(k)}" + ("" if ra.get(k) == rb.get(k) else f" -> {rb.get(k)}")
                       for k in RESOURCES)
        na, nb = (sum(not line.endswith(":") for line in side) for side in (a, b))
        if a == b:
            print(f"{name}: identical ({na} instructions; {res})")
            continue
        differ += 1
        print(f"{name}: {na} -> {nb} instructions; {res}")
        for line in difflib.unified_diff(a, b, "old", "new", n=2, lineterm=""):
            print("    " + line)
    print(f"{len(set(old) | set(new))} kernels, {differ} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
