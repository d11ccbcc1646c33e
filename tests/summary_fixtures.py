"""The --summary fixtures of tests/golden/summary/ (tests/golden/make_golden_summary.py): the reference's CSV per case."""
import glob
import gzip
import json
import os

import datasets as ds

DIR = os.path.join(ds.GOLD, "summary")
CASES = sorted(os.path.basename(p)[:-5] for p in glob.glob(os.path.join(DIR, "*.json")))


def meta(name):
    with open(os.path.join(DIR, name + ".json")) as f:
        return json.load(f)


def csv(name):
    with gzip.open(os.path.join(DIR, name + ".csv.gz"), "rb") as f:
        return f.read()


def rows(name):
    """[(barcode, total, duplicate, unmapped, lowmapq), ...] in file order, header left out"""
    out = []
    for ln in csv(name).decode().splitlines()[1:]:
        f = ln.split(",")
        out.append((f[0], int(f[1]), int(f[2]), int(f[3]), int(f[4])))
    return out


def key_of(barcode):
    """GenerateSeedFromSequence (utils.h:111-129): 2 bits per base, anything but ACGT counts as A"""
    k = 0
    for c in barcode:
        k = (k << 2) | {"A": 0, "C": 1, "G": 2, "T": 3}.get(c.upper(), 0)
    return k


def inputs(name):
    """(fa, reads, barcode / whitelist arguments) of a fixture: the command line tail the reference was run with"""
    m = meta(name)
    fa, r1, r2 = ds.case_inputs(m["base_case"])
    mate = m["single_end_mate"]
    reads = ["-1", r1, "-2", r2] if not mate else ["-1", r1 if mate == 1 else r2]
    extra = []
    if m["barcodes"]:
        bc, wl = ds.case_barcode_inputs(m["base_case"])
        extra = ["-b", bc] + (["--barcode-whitelist", wl] if m["barcodes"] == "wl" else [])
    return fa, reads, extra
