#!/bin/bash
# Everything profiles/object_history_cost.txt reports, on a machine with an MI355X:
#   bash profiles/object_history_cost.sh PARENT_DIR
# PARENT_DIR holds the parent commit's libpt_amd.so and libpt_amd_test.so (make -C project3-cuda-path-tracer_amd/csrc in a checkout of it).
# Each step runs under its own time limit and the script ends at the first step that fails.
set -o pipefail
parent=$(cd "$1" && pwd) || { echo "usage: $0 PARENT_DIR"; exit 1; }
out=out/object_history
mkdir -p $out
# 1 - 3: the kernel forms, the displayed frame, pt_init
timeout -k 10 300 python3 profiles/object_history_cost.py --parent-test-lib $parent/libpt_amd_test.so | tee $out/cost.txt || exit 1
# 4: the kernel names of a flagged renderer with nothing moved, from a trace run of its own
timeout -k 10 200 rocprofv3 --kernel-trace --stats -d $out/trace -o oh -- python3 profiles/object_history_cost.py --trace > $out/trace.txt 2>&1 || { tail -5 $out/trace.txt; exit 1; }
python3 - $out <<'PY' || exit 1
import glob, sqlite3, sys
db = sqlite3.connect(glob.glob(sys.argv[1] + "/trace/**/*results.db", recursive=True)[0])
for name, calls in db.execute("select name, total_calls from top_kernels order by name"):
    print("%6d  %s" % (calls, name))
PY
# 5: bench.py, the parent's build and this tree's alternating, two pairs; the frames compared bit for bit
for pair in 1 2; do
  PT_AMD_LIB=$parent/libpt_amd.so timeout -k 10 170 python3 bench.py --gpus 1 --steps 32 --warmup 4 --repeats 5 --dump-outputs $out/parent$pair > $out/parent$pair.json || exit 1
  timeout -k 10 170 python3 bench.py --gpus 1 --steps 32 --warmup 4 --repeats 5 --dump-outputs $out/new$pair > $out/new$pair.json || exit 1
done
python3 - $out <<'PY'
import glob, json, os, sys
import numpy as np
o = sys.argv[1]
for k in ("parent1", "new1", "parent2", "new2"):
    d = json.loads(open("%s/%s.json" % (o, k)).read().strip().splitlines()[-1])
    print(k, d["metric"], d["value"], "min", d.get("value_min"), "max", d.get("value_max"), "ms_per_step", d["ms_per_step"])
for pair in (1, 2):
    for f in sorted(glob.glob("%s/parent%d/*.npy" % (o, pair))):
        a, b = np.load(f), np.load(f.replace("parent", "new"))
        print("pair", pair, os.path.basename(f), "bit-identical:", bool(np.array_equal(a.view(np.uint32), b.view(np.uint32))))
PY
