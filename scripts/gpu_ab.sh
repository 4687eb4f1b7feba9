# A/B bench of alternate library builds: for each workload in $1, alternate
# the builds in $2 (paths relative to the repo; "default" = go-dsp_amd/lib)
# for $3 rounds (default 2). Parity tests selected by $4 (-k) run first on the
# default build. Lines and logs go to $OUT (default build/bench).
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
ROOT=$PWD
OUT=${OUT:-build/bench}
mkdir -p "$OUT"
if [ -n "$4" ]; then
  timeout -k 10 600 python -u -m pytest tests -m gpu -q -x --timeout 120 --timeout-method thread -k "$4" > "$OUT/ab_pytest.log" 2>&1; rc=$?
  echo "pytest rc=$rc"; tail -5 "$OUT/ab_pytest.log"; [ $rc -eq 0 ] || exit $rc
fi
for r in $(seq 1 ${3:-2}); do
for w in $1; do
  for L in $2; do
    # "default", a library directory, or env:VAR=value (default library, one switch set)
    unset GDSP_LIB; EV=""
    case "$L" in default) ;; env:*) EV="${L#env:}" ;; *) export GDSP_LIB=$ROOT/$L/libgdspfft.so ;; esac
    # --full: the line's parity field is printed beside the timings
    env $EV timeout -k 10 300 python bench.py --full --workload $w --steps 20 --warmup 3 --cpu-seconds 0 > "$OUT/ab.json" 2> "$OUT/ab.err"; rc=$?
    [ $rc -eq 0 ] || { echo "$w $L rc=$rc"; tail -20 "$OUT/ab.err"; exit $rc; }
    python -c "import json;d=json.load(open('$OUT/ab.json'));r=d['roofline'];print('$w','$L',d['ms_per_step'],r['avg_launch_ms'],r['frac'],(d.get('parity') or {}).get('max_nrel_vs_oracle'))"
  done
done
done
