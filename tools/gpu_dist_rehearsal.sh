# GPU box: 2 ranks on cuda:0 over gloo (rehearsal of the multi-rank bench path incl. the slab exchange).
# Plain `bench.py --gpus 2`: bench.py spawns its own torchrun child; --full adds the
# parity check and the config-4 rig legs this script reads. Results go to $OUT (default: bench_out/).
set -o pipefail
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 300 python bench.py --full --gpus 2 --steps 4 --warmup 2 --frames 64 --dist-backend gloo --same-device --no-cpu-baseline --matcher-steps 0 --rectify-steps 0 --stage-steps 1 > $OUT/dist.json 2> $OUT/dist.err || { tail -30 $OUT/dist.err; exit 1; }
python tools/show_bench.py $OUT/dist.json n_gpus value config config4_multi_gpu config4_multi_gpu_k1
