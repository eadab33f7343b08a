# rocprofv3 kernel trace of the 256-sequence decode leg (two lanes of 128 for q8 / q4): gpurun -- bash tools/profile_lanes.sh [streams]
# -> $PROFILE_OUT/lanes<streams>_kernel_stats.csv (PROFILE_OUT: default profile_out/ in the repository; copied to profiles/r03b_lanes256_kernel_stats.csv)
W=${1:-256}
R=$GRAFT_REPO_ROOT
O=${PROFILE_OUT:-$R/profile_out}
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
( while sleep 40; do echo tick; done ) & HB=$!
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_lanes -- python3 $R/bench.py --full --no-cpu-baseline --streams 0 --wide-streams $W --no-lanes --prefill 0 --generate 0 --serve 0 --steps 32 --warmup 8 > $O/lanes_bench.json 2> $O/lanes.err
rc=$?
kill $HB
echo rc=$rc
f=$(ls $O/prof_lanes/*/*kernel_stats.csv | head -1)
cp $f $O/lanes${W}_kernel_stats.csv
rm -rf $O/prof_lanes
