#!/bin/bash
# Kernel-trace statistics of the per-request sampler at V = 32000 fp16 (tools/sampling_prof.py), one rocprofv3 run per
# configuration and batch; the *_kernel_stats.csv files land in ${1:-profiles/sampling}.
set -u
OUT=${1:-profiles/sampling}
mkdir -p "$OUT"
for bs in 1 128; do
    for kind in all greedy top_p tail ext_mask ext_all ext_top; do
        timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/raw" -o "${kind}_b${bs}" -- \
            python tools/sampling_prof.py "$kind" "$bs" 200 || exit $?
        f=$(find "$OUT/raw" -name "${kind}_b${bs}_kernel_stats.csv" | head -1)
        [ -n "$f" ] && cp "$f" "$OUT/${kind}_b${bs}_kernel_stats.csv"
    done
done
rm -rf "$OUT/raw"
