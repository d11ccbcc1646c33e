#!/usr/bin/env python3
"""Do two builds launch the same kernels?  Two rocprofv3 --kernel-trace csv files of the same bench.py command (tools/gpu_trace.sh
shows the form): per kernel name the number of calls and the multiset of (grid size, workgroup size, LDS bytes) must agree.
usage: trace_compare.py BEFORE_kernel_trace.csv AFTER_kernel_trace.csv [OUT.json]; exit status 1 when they differ."""
import csv
import json
import sys
from collections import Counter, defaultdict


def launches(path):
    out = defaultdict(Counter)
    for r in csv.DictReader(open(path)):
        shape = tuple(int(r[k]) for k in sorted(r) if k.startswith(("Grid_Size", "Workgroup_Size", "LDS_Block_Size")))
        out[r["Kernel_Name"]][shape] += 1
    return out


def main(a_path, b_path, out=None):
    a, b = launches(a_path), launches(b_path)
    diff = {}
    for k in sorted(set(a) | set(b)):
        if a.get(k) != b.get(k):
            only_a, only_b = a.get(k, Counter()) - b.get(k, Counter()), b.get(k, Counter()) - a.get(k, Counter())
            diff[k] = {"calls": [sum(a.get(k, Counter()).values()), sum(b.get(k, Counter()).values())],
                       "only_before": [[list(s), n] for s, n in sorted(only_a.items())], "only_after": [[list(s), n] for s, n in sorted(only_b.items())]}
    res = {"columns": "Grid_Size_X/Y/Z, LDS_Block_Size, Workgroup_Size_X/Y/Z", "kernel_names": [len(a), len(b)],
           "launches": [sum(sum(c.values()) for c in a.values()), sum(sum(c.values()) for c in b.values())],
           "distinct_shapes": [sum(len(c) for c in a.values()), sum(len(c) for c in b.values())], "differences": diff,
           "calls_before": {k.split("(")[0]: sum(c.values()) for k, c in sorted(a.items())}}
    txt = json.dumps(res, indent=1)
    print(txt)
    if out:
        open(out, "w").write(txt + "\n")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:4]))
