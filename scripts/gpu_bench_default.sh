# The full default bench line (N=1, nested configs, parity, CPU baselines),
# then with "rehearse" a 2-rank gloo rehearsal of the N>1 path on one GPU
# (strong + weak + configs). Lines and logs go to $OUT (default build/bench).
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-build/bench}
mkdir -p "$OUT"
timeout -k 10 600 python bench.py --full --gpus 1 --steps 20 --warmup 5 > "$OUT/bench_default.json" 2> "$OUT/bench_default.err"; rc=$?
echo "bench rc=$rc"; cat "$OUT/bench_default.json"; [ $rc -eq 0 ] || { tail -30 "$OUT/bench_default.err"; exit $rc; }
if [ "${1:-}" = rehearse ]; then
  GDSP_DIST_BACKEND=gloo timeout -k 10 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29513 bench.py --full --gpus 2 --steps 5 --warmup 1 --cpu-seconds 0 --batch 16384 > "$OUT/rehearse2.json" 2> "$OUT/rehearse2.err"; rc=$?
  echo "rehearse rc=$rc"; cat "$OUT/rehearse2.json"; [ $rc -eq 0 ] || { tail -30 "$OUT/rehearse2.err"; exit $rc; }
fi
