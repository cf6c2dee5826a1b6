#!/bin/bash
# Round-end validation on a GPU node: the whole GPU suite, then the profile round (kernel stats, PMC traffic, launch
# table), the instruction counters, the full default bench line and the other-configuration lines.
# usage: bash tools/final_round.sh <tag>      -> $OUT_DIR/<tag>_* (default bench_out/); copy them into profiles/ afterwards
TAG=${1:-r02}
export OUT_DIR=${OUT_DIR:-$PWD/bench_out}
mkdir -p $OUT_DIR
python -m pytest tests -m gpu -x -q > $OUT_DIR/gputest_final.log 2>&1; rc=$?
tail -3 $OUT_DIR/gputest_final.log
[ $rc = 0 ] || exit $rc
set -e
bash tools/profile_round.sh $TAG > $OUT_DIR/prof_round.log 2>&1
cp $OUT_DIR/${TAG}_launches.json $OUT_DIR/${TAG}_pmc_traffic.json profiles/
bash tools/pmc_instr.sh ${TAG}_cfg2 > $OUT_DIR/pmc_instr.log 2>&1
cp $OUT_DIR/${TAG}_cfg2_instr.json profiles/
python bench.py --full > $OUT_DIR/${TAG}_default_bench.json 2> $OUT_DIR/${TAG}_default_bench.err
bash tools/other_configs.sh > $OUT_DIR/${TAG}_other_configs_bench.json 2> $OUT_DIR/other.err
python - "$OUT_DIR" "$TAG" <<'EOF'
import json, csv, sys
out, tag = sys.argv[1], sys.argv[2]
d=json.loads(open(f"{out}/{tag}_default_bench.json").read().strip().splitlines()[-1])
r=d["roofline"]; print(d["value"], d["ms_per_step"], r["frac"], r["kernel_ms"], r["utilisation"]["kernel_ms_isolated"], r["utilisation"]["kernel_ms_isolated_hip_events"], r["traffic"], d["cpu_baseline"]["value"], d["cpu_baseline_config0"]["value"])
for row in csv.DictReader(open(f"{out}/{tag}_default_bench_kernel_stats.csv")):
    if "gq_" in row["Name"] and int(row["Calls"])>40: print(row["Name"][:50], row["Calls"], round(float(row["AverageNs"])/1e3,2), round(float(row["MinNs"])/1e3,2), round(float(row["MaxNs"])/1e3,2))
for l in open(f"{out}/{tag}_other_configs_bench.json"):
    l=l.strip()
    if l.startswith("{"):
        e=json.loads(l); print(e["config"]["workload"][:50], round(e["value"]), round(e["ms_per_step"],4))
EOF
