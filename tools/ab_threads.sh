# copy threads per direction A/B on the host paths (C4): readset from unsorted reads in R's form,
# and the default e2e lines:  tools/ab_threads.sh [OUTDIR]
set -o pipefail
OUT=${1:-build/ab_threads}
mkdir -p "$OUT"
for t in 8 12 16; do
  RCP_H2D_THREADS=$t timeout -k 10 200 python3 tools/diag_unsorted.py 3 codes+wruns 2>&1 | grep "readset 2" | sed "s/^/h2d $t: /"
done
for t in 8 12; do
  RCP_H2D_THREADS=$t timeout -k 10 400 python3 bench.py --full --no-cpu --steps 5 --inflight 1 > "$OUT/abt_$t.json" 2>/dev/null || exit 1
  python3 -c "
import json; d=json.load(open('$OUT/abt_$t.json')); e=d['e2e']
print('h2d $t e2e', round(e['ms'],2), 'any', round(e['any_order']['ms'],2), 'pipelined', round(e['samples_pipelined']['ms'],2), 'rle', round(e['rle_path']['ms'],2))"
done
