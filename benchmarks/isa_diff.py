#!/usr/bin/env python
"""Equality of two builds of libunerf, kernel by kernel -- the check of a refactor of csrc/ that must not move a kernel:

    python benchmarks/isa_diff.py a.so b.so [-o report.json]

Reports the kernel symbols only one library has, the kernels whose listing differs (llvm-objdump -d: text + encoding,
addresses removed) and the kernels whose metadata differs (the whole per-kernel map of the llvm-readelf --notes output:
register counts, LDS, scratch, workgroup size, arguments).  Exit status 1 on any difference."""
import argparse
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uncertainty_nerf_gs_amd import isa_check  # noqa: E402


def listings(path):
    """"<code object>:<symbol>" -> its instruction lines (`text // address: encoding`), the address removed"""
    out = {}
    for i, text in enumerate(isa_check.disassemble(path)):
        lines = None
        for line in text.split("\n"):
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                lines = out.setdefault(f"{i}:{m.group(1)}", [])
            elif lines is not None:
                lines.append(re.sub(r"// [0-9A-Fa-f]+:", "//", line))
    return out


def metadata(path):
    """"<code object>:<kernel>" -> the text of its entry under amdhsa.kernels"""
    out = {}
    for i, text in enumerate(isa_check.disassemble(path, "llvm-readelf", ("--notes",))):
        kernels = text.split("amdhsa.kernels:\n", 1)[1].split("\namdhsa.", 1)[0]
        for entry in re.split(r"^  - ", kernels, flags=re.M)[1:]:
            out[f"{i}:" + re.search(r"^ *\.name: +(\S+)$", entry, re.M).group(1)] = entry
    return out


def per_object(keys):
    return [sum(k.startswith(f"{i}:") for k in keys) for i in range(1 + max(int(k.split(":")[0]) for k in keys))]


def diff(a, b):
    la, lb, ma, mb = listings(a), listings(b), metadata(a), metadata(b)
    return {"a": a, "b": b,
            "symbols_per_code_object": {"a": per_object(la), "b": per_object(lb)},
            "kernels_per_code_object": {"a": per_object(ma), "b": per_object(mb)},
            "only_in_a": sorted((set(la) - set(lb)) | (set(ma) - set(mb))),
            "only_in_b": sorted((set(lb) - set(la)) | (set(mb) - set(ma))),
            "listing_differs": sorted(k for k in set(la) & set(lb) if la[k] != lb[k]),
            "metadata_differs": sorted(k for k in set(ma) & set(mb) if ma[k] != mb[k])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("-o", "--out")
    args = ap.parse_args()
    rep = diff(args.a, args.b)
    print(json.dumps(rep, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rep, f, indent=1)
    sys.exit(1 if any(rep[k] for k in ("only_in_a", "only_in_b", "listing_differs", "metadata_differs")) else 0)


if __name__ == "__main__":
    main()
