#!/bin/bash
# bench.py's event-timed launch duration of the headline kernel beside rocprofv3's kernel duration for the same command
# (--full: the roofline entry comes from the kernel probes a plain bench run skips).  Output under prof_out/chk.
cd "$(dirname "$0")/.." || exit 1
rm -rf prof_out/chk && mkdir -p prof_out
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d prof_out/chk -o c -- python3 bench.py --full --no-also --no-cpu-baseline "$@" > prof_out/chk.json 2> prof_out/chk.err
python3 - <<'PY'
import json, glob, csv
j = json.load(open("prof_out/chk.json"))
print("bench:", j["value"], "frames/s,", j["ms_per_step"], "ms/step; roofline", {k: j["roofline"].get(k) for k in ("avg_launch_ms", "avg_ms_alone", "launch_interval_ms", "achieved", "frac")})
for f in glob.glob("prof_out/chk/**/*kernel_stats.csv", recursive=True):
    for r in list(csv.DictReader(open(f)))[:3]:
        print("rocprofv3:", r["Name"][:40], r["Calls"], "calls, avg", r["AverageNs"], "ns")
PY
