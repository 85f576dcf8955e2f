# The round's committed measurements in one gpurun call (run from the repo root on the GPU box):
#   bench line, rocprofv3 kernel stats + the two HBM PMC passes of the same command, the configs[4] line, full-head kernel stats.
# Afterwards, in the build container:  bash tools/collect_round_profiles.sh round6   (copies the summaries into profiles/)
# This is the LAST measurement command of a round: tests/test_host_logic.py::test_committed_roofline_records_match_the_kernel_source holds the tree
# to the source hash these passes record.
O=${PROFILE_OUT:-profile_out}; mkdir -p $O; export PROFILE_OUT=$O
bash tools/profile_round.sh > $O/profile_round.log 2>&1
python tools/pmc_traffic.py $O/prof_round $O/${ROUND:-round6}_pmc_hbm_traffic > $O/pmc_traffic.log 2>&1
python bench.py --full > $O/bench_final.json 2> $O/bench_final.err
python bench.py --full --config 5 --no-cpu-baseline > $O/bench_cfg5.json 2>/dev/null
bash tools/prof_full_head.sh > $O/prof_full_head.log 2>&1
find $O/prof_round -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $O/kernel_stats.csv
python tools/north_trace_split.py $O/prof_round/stats > $O/north_trace_split.txt 2>&1     # in-step against back-to-back launches of the roofline kernel, from the same trace
find $O/prof_round $O/prof_full -name "*kernel_trace.csv" -delete     # (the traces are too large to keep)
tail -c 400 $O/bench_final.json
