#!/bin/bash
# usage (on an MI355X): tools/profile_bench.sh <tag> [bench.py args...]
# writes $PROFILE_OUT/<tag>_bench.json (the --full line, unprofiled), $PROFILE_OUT/<tag>_bench_profiled.json and
# $PROFILE_OUT/<tag>_kernel_stats.csv (rocprofv3 --kernel-trace --stats of the headline alone, kvq kernels only);
# PROFILE_OUT defaults to profile_out/ in the repository
tag=$1; shift
cd "$(dirname "$0")/.." && export TMPDIR=/tmp
out=${PROFILE_OUT:-profile_out}
mkdir -p $out
python bench.py "$@" --full > $out/${tag}_bench.json 2> $out/${tag}_bench.err
rm -rf /tmp/prof_$tag
rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_$tag -o p -- python bench.py "$@" --steps 5 --warmup 2 > $out/${tag}_bench_profiled.json 2> /tmp/prof_$tag.log
f=$(find /tmp/prof_$tag -name "*kernel_stats.csv" | head -1)
python - "$f" $out/${tag}_kernel_stats.csv <<'PY'
import csv, re, sys
rows = list(csv.DictReader(open(sys.argv[1])))
out = csv.writer(open(sys.argv[2], "w", newline=""))
out.writerow(["kernel", "calls", "total_us", "avg_us", "pct"])
for r in rows:
    name = re.sub(r"\(.*", "", r["Name"]).replace("void ", "")
    if "kvq::" not in name:
        continue
    out.writerow([name[:110], r["Calls"], "%.1f" % (float(r["TotalDurationNs"]) / 1e3), "%.2f" % (float(r["AverageNs"]) / 1e3), r["Percentage"]])
PY
cat $out/${tag}_kernel_stats.csv
