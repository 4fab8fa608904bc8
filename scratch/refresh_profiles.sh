#!/bin/bash
# Round profile refresh on the GPU box (headline workload): kernel stats + launch order of the default command, the two-stream
# trace, the --full bench line (which runs its own counter passes).  usage: bash scratch/refresh_profiles.sh r4 <output directory>
export TMPDIR=/tmp; R=$GRAFT_REPO_ROOT; RND=${1:-r4}
OUT=$(realpath -m "${2:?usage: bash scratch/refresh_profiles.sh <round> <output directory>}")
mkdir -p $OUT/profiles_new
cd /tmp; rm -rf $OUT/prof_cur $OUT/prof_2s
# single-stream: per-kernel durations add up to the step
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_cur -o $RND -- python3 $R/bench.py --steps 5 --warmup 2 --cpu-scenes 0 --single-stream --no-reference-order --no-native-arith --no-evidence --no-f16x2 --no-counters --no-voxel-density --no-prior-variants --no-launch-power > $OUT/prof_cur.log 2>&1
# two streams (the headline mode): the overlap
rocprofv3 --kernel-trace --output-format csv -d $OUT/prof_2s -o $RND -- python3 $R/bench.py --steps 6 --warmup 2 --cpu-scenes 0 --no-reference-order --no-native-arith --no-evidence --no-f16x2 --no-counters --no-voxel-density --no-prior-variants --no-launch-power > $OUT/prof_2s.log 2>&1
# the same step on clouds at voxel-grid density (bench.py --cloud voxel2mm; value_voxel_density of a --full run)
rm -rf $OUT/prof_vox
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_vox -o ${RND}_voxel2mm -- python3 $R/bench.py --cloud voxel2mm --steps 5 --warmup 2 --cpu-scenes 0 --single-stream --no-reference-order --no-native-arith --no-evidence --no-f16x2 --no-counters --no-prior-variants --no-launch-power > $OUT/prof_vox.log 2>&1
cd $R
cp $OUT/prof_vox/${RND}_voxel2mm_kernel_stats.csv $OUT/profiles_new/${RND}_voxel2mm_kernel_stats.csv
python3 scratch/step_trace.py $OUT/prof_vox/${RND}_voxel2mm_kernel_trace.csv > $OUT/profiles_new/${RND}_voxel2mm_step_trace.txt
cp $OUT/prof_cur/${RND}_kernel_stats.csv $OUT/profiles_new/${RND}_kernel_stats.csv
python3 scratch/step_trace.py $OUT/prof_cur/${RND}_kernel_trace.csv > $OUT/profiles_new/${RND}_step_trace.txt
python3 scratch/two_stream_trace.py $OUT/prof_2s/${RND}_kernel_trace.csv > $OUT/profiles_new/${RND}_two_stream_trace.txt
[ -n "$SKIP_BENCH" ] || python3 bench.py --full > $OUT/bench_cur.json 2> $OUT/bench_cur.err
tail -1 $OUT/bench_cur.json > $OUT/profiles_new/${RND}_bench_n1.json
tail -1 $OUT/bench_cur.json | cut -c1-300
tail -2 $OUT/profiles_new/${RND}_step_trace.txt; tail -1 $OUT/profiles_new/${RND}_two_stream_trace.txt
tail -3 $OUT/bench_cur.err
