"""The single-end --split-alignment fixtures (tests/golden/se_split, made by the reference itself: make_se_split_golden.py there):
names, inputs, expected bytes and parameters, shared by tests/test_hostemu_se_split.py and tests/test_gpu_se_split.py."""
import gzip
import os

import datasets

DIR = "se_split"
CASES = sorted(f[:-5] for f in os.listdir(os.path.join(datasets.GOLD, DIR)) if f.endswith(".json"))
COUNTERS = ("num_candidates", "num_mappings", "num_mapped_reads", "num_uniquely_mapped_reads")
BC_COUNTERS = COUNTERS + ("num_barcode_in_whitelist", "num_corrected_barcode")


def meta(case):
    return datasets.case_meta(DIR + "/" + case)


def flags(case):
    return meta(case)["chromap_flags"]


def is_sam(case):
    return "--SAM" in flags(case)


def is_tagalign(case):
    return "--TagAlign" in flags(case)


def has_barcodes(case):
    return "bc" in meta(case)["input_md5"]


def inputs(case):
    """(fa, fastq of the mate that is mapped as single-end reads)"""
    fa, r1, r2 = datasets.case_inputs(DIR + "/" + case)
    return fa, (r1 if meta(case)["single_end_mate"] == 1 else r2)


def barcode_inputs(case):
    return datasets.case_barcode_inputs(DIR + "/" + case)


def index(case):
    return datasets.case_index(DIR + "/" + case)


def golden(case):
    with gzip.open(os.path.join(datasets.GOLD, DIR, case + ".out.gz"), "rb") as f:
        return f.read()


def params_kw(case):
    """the case's chromap flags as parameter overrides (split_alignment among them)"""
    fl = [f for f in flags(case) if f != "--split-alignment"]
    preset, kw = datasets.flags_to_params(fl)
    assert preset is None and "--split-alignment" in flags(case)
    kw["split_alignment"] = 1
    return kw


def first_difference(got, want):
    """a readable assertion message for two texts that should be equal"""
    g, w = got.split(b"\n"), want.split(b"\n")
    for i in range(min(len(g), len(w))):
        if g[i] != w[i]:
            return "line %d: got %r, want %r" % (i + 1, g[i], w[i])
    return "%d lines, want %d" % (len(g), len(w))
