# 2 ranks sharing the one GPU with the default flags (host-path e2e per rank on its shard, as the
# driver's scaling run would do on 2 GPUs):  tools/share2_full.sh [OUTDIR]
set -o pipefail
OUT=${1:-build/share2}
mkdir -p "$OUT"
RCP_SHARE_GPU=1 timeout -k 10 900 python3 bench.py --full --gpus 2 > "$OUT/share2_full.json" 2> "$OUT/share2_full.err" || { tail -30 "$OUT/share2_full.err"; exit 1; }
python3 -c "import json; d=json.loads([l for l in open('$OUT/share2_full.json') if l.startswith('{')][-1]); print(d['n_gpus'], d['value'], d['ms_per_step'], d['e2e']['ms'], d['e2e'].get('note','')[-60:])"
