# Bench lines of the other BASELINE configs (C2, C3, C5) and the C4 trainer path, one box, with the
# CPU baseline off (it is the same oracle trainer as the C4 line's) -> var/ev/ (or the directory given)
set -u
O=${1:-var/ev}
mkdir -p $O
for c in c2 c3 c5; do
  timeout -k 10 300 python bench.py --full --config $c --no-cpu-baseline > $O/bench_$c.json 2> $O/bench_$c.err || exit 1
  cat $O/bench_$c.json
done
timeout -k 10 300 python bench.py --full --path trainer --no-cpu-baseline > $O/bench_c4_trainer.json 2> $O/bench_c4_trainer.err || exit 1
cat $O/bench_c4_trainer.json
