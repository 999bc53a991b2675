#!/bin/bash
# A/B of a kernel's time per launch (HIP events) between two libraries, alternating
# Usage: bash tools/chain_ab.sh [<workload> [<roofline key> [<libA> <libB>]]]
# (defaults: n1024_fp32, chain_kernel_avg_us — the chain's time per chunk — libekfslam.so against
# libekfslam_base.so; e.g. n1024_fp32_assoc assoc_kernel_avg_us for k_assoc_msg's)
set -o pipefail
wl=${1:-n1024_fp32}; key=${2:-chain_kernel_avg_us}
la=${3:-libekfslam.so}; lb=${4:-libekfslam_base.so}
for r in 1 2 3; do
  for lib in $la $lb; do
    o=gpurun_out/cab_${lib%.so}_$r
    EKF_LIB=$lib timeout -k 10 300 python -u bench.py --workload $wl --full --steps 200 --warmup 20 --no-cpu --traffic off --no-fp64 > $o.json 2> $o.err || exit $?
    python -c "import json;d=json.load(open('$o.json'));r=d['roofline'];print('$lib', $r, round(d['value']), '${key%%_*} %.3f'%r['$key'], 'pass %.2f'%r['avg_launch_us'])"
  done
done
