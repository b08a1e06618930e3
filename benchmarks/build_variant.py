#!/usr/bin/env python
"""Build one A/B variant of libunerf by the product recipe (lib.compile_library: every source, the product flags, the ISA
hazard check), with extra -D arguments and / or a patched copy in place of unerf_nerf.hip (benchmarks/probe_source.py):

    python benchmarks/build_variant.py <name> [--nerf-source PATH] [-DNAME=VALUE ...]   ->  benchmarks/build_probe/libunerf_<name>.so

`build_variant.py base` is the shipped library under an A/B name.  Used with benchmarks/ab_bench.sh / multi_ab.sh, which
choose a library through UNERF_LIB."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from uncertainty_nerf_gs_amd import lib  # noqa: E402

B = os.path.join(ROOT, "benchmarks", "build_probe")


def variant(name, nerf_source=None, defs=()):
    """-> (output path, extra arguments, replacement) as lib.compile_library takes them"""
    return os.path.join(B, f"libunerf_{name}.so"), list(defs), ("unerf_nerf.hip", nerf_source) if nerf_source else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("name")
    ap.add_argument("--nerf-source", help="compile this file in place of csrc/unerf_nerf.hip")
    a, defs = ap.parse_known_args()
    out, extra, replace = variant(a.name, a.nerf_source, defs)
    os.makedirs(B, exist_ok=True)
    print(lib.compile_library(out, extra, replace, verbose=True))


if __name__ == "__main__":
    main()
