#!/bin/bash
# Round-end measurement pass, part B: rocprofv3 kernel stats of the default bench command, serialised breakdowns (full step and E/R/A/D-only step), stream timeline, roll-out kernel trace -> gpurun_out/
cd ${GRAFT_REPO_ROOT:-.}
export TMPDIR=/tmp
mkdir -p gpurun_out
OUT=${OUT:-build/round_end}; mkdir -p $OUT      # bench lines (bench.py --full: the legs these lines read run only with it)
rm -rf $OUT/prof_stats
timeout 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_stats -o bair -- python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-plugin > $OUT/bench_prof.json 2> $OUT/bench_prof.err
python tools/rocprof_summary.py $OUT/prof_stats/bair_results.db "python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-plugin (BAIR 256x256, T=16, B=8 incl. VGG19 perceptual loss; timed steps + erad-only leg + profiled steps + exact-fp32 step + 4 x 36-frame roll-outs)" > $OUT/kernel_stats.txt
head -12 $OUT/kernel_stats.txt | cut -c1-90,105-160
rm -rf gpurun_out/prof_stats gpurun_out/prof_serial
CADDY_STREAMS=0 timeout 600 rocprofv3 --kernel-trace --stats -d gpurun_out/prof_serial -o bair -- python bench.py --steps 3 --warmup 1 --no-cpu-baseline --profile-steps 0 --no-rollout --no-extra-legs --no-plugin > /dev/null 2> gpurun_out/bench_serial.err
python tools/step_breakdown.py gpurun_out/prof_serial/bair_results.db 60 > gpurun_out/step_breakdown_serial.txt; head -3 gpurun_out/step_breakdown_serial.txt
rm -rf gpurun_out/prof_serial
CADDY_STREAMS=0 timeout 600 rocprofv3 --kernel-trace --stats -d gpurun_out/prof_serial -o bair -- python bench.py --steps 3 --warmup 1 --no-cpu-baseline --profile-steps 0 --no-rollout --no-perceptual --no-extra-legs --no-plugin > /dev/null 2> gpurun_out/bench_serial_erad.err
python tools/step_breakdown.py gpurun_out/prof_serial/bair_results.db 60 > gpurun_out/step_breakdown_serial_erad.txt; head -3 gpurun_out/step_breakdown_serial_erad.txt
rm -rf gpurun_out/prof_serial gpurun_out/prof_tl
timeout 600 rocprofv3 --kernel-trace --stats -d gpurun_out/prof_tl -o bair -- python bench.py --steps 3 --warmup 1 --no-cpu-baseline --profile-steps 0 --no-rollout --no-perceptual --no-extra-legs --no-plugin > /dev/null 2> gpurun_out/bench_tl.err
python tools/timeline.py gpurun_out/prof_tl/bair_results.db 40 > gpurun_out/timeline_erad.txt 2>&1; sed -n 2,7p gpurun_out/timeline_erad.txt
rm -rf gpurun_out/prof_tl
bash tools/gpu_rollout_profile.sh 2>&1 | head -3
timeout 300 python tools/layer_profile.py > gpurun_out/layer_profile.txt 2>&1; grep phase gpurun_out/layer_profile.txt
