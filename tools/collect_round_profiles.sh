#!/bin/bash
# After `bash tools/final_profile.sh` ran on the GPU host: copy the judged summaries from $PROFILE_OUT (default profile_out/, untracked) into profiles/ (tracked).
#   bash tools/collect_round_profiles.sh round6
set -e
cd "$(dirname "$0")/.."
r=${1:?round tag, e.g. round6}
O=${PROFILE_OUT:-profile_out}
cp $O/${r}_pmc_hbm_traffic.json profiles/${r}_pmc_hbm_traffic.json
cp $O/${r}_pmc_hbm_traffic.txt profiles/${r}_pmc_hbm_traffic.txt
cp $O/kernel_stats.csv profiles/${r}_kernel_stats.csv
cp $O/prof_full/kernel_stats.csv profiles/${r}_kernel_stats_full_head.csv
cp $O/bench_final.json profiles/${r}_bench_line.json
cp $O/bench_cfg5.json profiles/${r}_bench_line_config5.json
cp $O/north_trace_split.txt profiles/${r}_north_trace_split.txt
ls -la profiles/${r}_*
