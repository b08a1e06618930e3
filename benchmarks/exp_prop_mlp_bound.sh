#!/bin/bash
# Upper bound on what moving the proposal MLP (10 -> 16 -> 1, 112 of ~540 VALU instructions per sample) to the matrix
# pipe could gain: the proposal kernel with the MLP REMOVED (benchmarks/probe_source.py --no-prop-mlp: ten adds instead; wrong
# results) against the shipped one, same box.
#   here:        bash benchmarks/exp_prop_mlp_bound.sh build
#   on the box:  bash benchmarks/exp_prop_mlp_bound.sh run     -> gpurun_out/multi_ab.json
cd "$(dirname "$0")/.."
B=benchmarks/build_probe
if [ "$1" = build ]; then
    mkdir -p $B
    python benchmarks/build_variant.py base || exit 1
    python benchmarks/probe_source.py --no-prop-mlp -o $B/unerf_nerf_nomlp.hip || exit 1   # a patched COPY of the product source
    python benchmarks/build_variant.py nomlp --nerf-source $B/unerf_nerf_nomlp.hip || exit 1
    exit 0
fi
bash benchmarks/multi_ab.sh active base nomlp
