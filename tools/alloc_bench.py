#!/usr/bin/env python3
"""Times cmgpu_store_format with and without --allocate-multi-mappings on the same record store: one batch of read pairs from the
repeat-bearing synthetic genome of `bench.py --full` (--repeats 32,600,3000,0.02), mapped with -n 5 and no preset (the in-memory
flavour), formatted alternately with the flag off and on.  The clock is the host's around the call, which ends in a stream
synchronise; the stage's own time and its host draw's share come from the context (cmgpu_get_option alloc_us / alloc_draw_us).
Prints one JSON object; --out also writes it to a file.  Kernel times: run it under `rocprofv3 --kernel-trace --stats` in a run of
its own (--rounds 2 keeps that short)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chromap_amd import ChromapGPU, _capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4_000_000)
    ap.add_argument("--genome", type=int, default=3_100_000_000)
    ap.add_argument("--nseq", type=int, default=24)
    ap.add_argument("--repeats", default="32,600,3000,0.02")
    ap.add_argument("-n", type=int, default=5)
    ap.add_argument("--distance", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    fam, copies, elen, div = a.repeats.split(",")
    kw = dict(max_num_best_mappings=a.n, mapq_threshold=0)
    t0 = time.perf_counter()
    g = ChromapGPU(synthetic=(a.genome, a.nseq, 1, (int(fam), int(copies), int(elen), float(div))), **kw)
    t_setup = time.perf_counter() - t0
    g.generate_resident(a.pairs, read_length=50, frag_min=30, frag_max=600, sub_rate=0.01, seed=1000)
    g.map_resident()
    n_rec = g.store_append_resident()
    p_off = _capi.default_params(None, **kw)
    p_on = _capi.default_params(None, allocate_multi_mappings=1, multi_mapping_allocation_distance=a.distance, **kw)
    times = {"off": [], "on": []}
    stage, draw, info, lines = [], [], None, {}
    for r in range(a.rounds + 1):  # (round 0 warms up: buffers, code objects)
        for name, p in (("off", p_off), ("on", p_on)):
            t = time.perf_counter()
            nl, nb = g.store_format(_capi.TEXT_BED_PE, params=p)
            dt = time.perf_counter() - t
            if r == 0:
                continue
            times[name].append(dt * 1e3)
            lines[name] = (nl, nb)
            if name == "on":
                stage.append(g.get_option("alloc_us") / 1e3)
                draw.append(g.get_option("alloc_draw_us") / 1e3)
                info = g.store_allocation_info()

    def summary(v):
        return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "runs": len(v)}
    out = {"pairs": a.pairs, "records_in_store": n_rec, "max_num_best_mappings": a.n, "distance": a.distance, "genome": a.genome,
           "repeats": a.repeats, "setup_s": round(t_setup, 1),
           "store_format_flag_off": summary(times["off"]), "store_format_flag_on": summary(times["on"]),
           "allocation_stage": summary(stage), "host_draw": summary(draw),
           "multi_mappings": info[0], "allocated": info[1], "without_overlap": info[2],
           "lines_bytes_flag_off": lines["off"], "lines_bytes_flag_on": lines["on"]}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    g.close()


if __name__ == "__main__":
    main()
