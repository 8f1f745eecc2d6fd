# kitti64 / ouster128 / dense1m bench lines (no CPU baseline) + the one-GPU batch table, into OUT/<tag>_*.json
#   bash tools/experiments/r4_bench3.sh TAG OUT
TAG=${1:-r4}
OUT=${2:?usage: r4_bench3.sh TAG OUT}
mkdir -p $OUT
python bench.py --full --no-cpu-baseline > $OUT/${TAG}_kitti64.json 2> $OUT/${TAG}.err
for W in ouster128 dense1m; do python bench.py --full --no-cpu-baseline --no-batch --workload $W > $OUT/${TAG}_$W.json 2>> $OUT/${TAG}.err; done
echo done
