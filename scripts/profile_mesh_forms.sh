#!/bin/bash
# rocprofv3 kernel stats of the iterate kernels of a large shirt launch (scripts/mesh_forms_trace.py): fs_k_iterate<false>
# against fs_k_iterate_mesh on 192 shirts of ~8.6 k vertices, and against fs_k_iterate_mixed on 96 such shirts + 96 grids of
# equal particle count.  GPU box, repo root; one profiled process per launch class, one after the other; writes
# $OUT/mesh_forms/${TAG}_{mesh,mixed}_kernel_stats.csv.  usage: profile_mesh_forms.sh [TAG] [OUT]; OUT is a directory relative to
# the repo root and defaults to build/profile_out (build/ is kept out of git).
ROOT=$(pwd); TAG=${1:-r29}; OUT=${2:-build/profile_out}
export OUT
mkdir -p $ROOT/$OUT/mesh_forms
for LAUNCH in mesh mixed; do
    rm -rf $ROOT/$OUT/prof_mf_$LAUNCH
    (cd /tmp && TMPDIR=/tmp timeout -k 10 240 rocprofv3 --kernel-trace --stats -d $ROOT/$OUT/prof_mf_$LAUNCH -o mf -- \
        python3 $ROOT/scripts/mesh_forms_trace.py $LAUNCH > $ROOT/$OUT/mesh_forms/${TAG}_${LAUNCH}_run.txt 2>&1) || { echo "$LAUNCH: profiled run failed"; exit 1; }
    grep '^{' $ROOT/$OUT/mesh_forms/${TAG}_${LAUNCH}_run.txt
    TAG=$TAG LAUNCH=$LAUNCH python3 - <<'PY' || exit 1
import csv, glob, os, sqlite3
tag, launch = os.environ["TAG"], os.environ["LAUNCH"]
out = os.environ["OUT"]
f = glob.glob(f"{out}/prof_mf_{launch}/**/*.db", recursive=True)[0]
con = sqlite3.connect(f)
rows = list(con.execute("select name,total_calls,total_duration,average,percentage from top_kernels"))
with open(f"{out}/mesh_forms/{tag}_{launch}_kernel_stats.csv", "w", newline="") as fh:
    w = csv.writer(fh)
    w.writerow([f"kernel (rocprofv3 --kernel-trace --stats -- python3 scripts/mesh_forms_trace.py {launch})", "calls", "total_us", "average_us", "percent"])
    for name, calls, total, avg, pct in rows:
        if pct >= 0.01:
            w.writerow([name[:120], calls, f"{total:.3f}", f"{avg:.3f}", f"{pct:.2f}"])
        if pct >= 0.5:
            print(launch, name[:90], calls, round(avg, 3), round(pct, 2))
PY
    find $ROOT/$OUT/prof_mf_$LAUNCH -name "*.db" -delete
done
