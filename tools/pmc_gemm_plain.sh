#!/bin/bash
# SQ counters of the 256x256 NT GEMM (gemm_nt9_kernel) on a plain 8192^3 problem, one rocprofv3 pass per counter set;
# CUM_LIB selects the library build.  Prints the table; traces go to a temporary folder that is removed afterwards.
#   bash tools/pmc_gemm_plain.sh
root=$(cd "$(dirname "$0")/.." && pwd)
work=$(mktemp -d)
trap 'rm -rf "$work"' EXIT
cd "$root"
i=0
for set in "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU" \
           "SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_MFMA SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INST_CYCLES_VMEM" \
           "GRBM_GUI_ACTIVE"; do
  i=$((i+1))
  rocprofv3 --pmc $set --kernel-trace --output-format csv -d "$work/pass_$i" -- python3 tools/gemm_plain.py > "$work/pass_$i.log" 2>&1 \
    || { tail -20 "$work/pass_$i.log"; exit 1; }
  python3 - "$work/pass_$i" "${CUM_LIB:-default}" <<'PY'
import csv, glob, sys, collections
acc = collections.defaultdict(float); cnt = collections.Counter(); dur = []
for f in glob.glob(sys.argv[1] + "/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if "gemm_nt" not in r["Kernel_Name"]: continue
        acc[r["Counter_Name"]] += float(r["Counter_Value"]); cnt[r["Counter_Name"]] += 1
for f in glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if "gemm_nt" in r["Kernel_Name"]: dur.append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
print("lib=%s  kernel us (median of %d): %.1f" % (sys.argv[2], len(dur), sorted(dur)[len(dur) // 2] / 1e3 if dur else -1))
for c, v in sorted(acc.items()): print(f"   {c:30s} {v / cnt[c]:16.0f}")
PY
done
