# rocprofv3 per-kernel summary of the bench (kernel-trace + stats): TAG names the output files under OUT
set -x
TAG=${TAG:-r4}
R=$GRAFT_REPO_ROOT
OUT=${OUT:-$R/profiles_out}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_kstats -- python3 $R/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $OUT/${TAG}_bench_under_rocprof.json 2> $OUT/${TAG}_kstats.err
echo rc=$?
