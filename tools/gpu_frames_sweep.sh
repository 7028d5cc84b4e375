set -o pipefail
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}
mkdir -p $OUT
for fr in 256 512 1024 256 512 1024; do
  timeout -k 10 300 python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --matcher-steps 0 --rectify-steps 0 --no-side-configs --frames $fr > $OUT/fs.json 2> $OUT/fs.err || { tail -20 $OUT/fs.err; exit 1; }
  python -c "import json;d=json.load(open('$OUT/fs.json'));print($fr, d['value'], d['ms_per_step'], d['stage_ms'], d['parity']['ok'])"
done
