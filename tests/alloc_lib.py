"""What the --allocate-multi-mappings tests share: the fixtures of tests/golden/alloc (made by the reference binary,
tests/golden/alloc/make_alloc_golden.py) and the translation of their flags."""
import gzip
import os

import datasets

DIR = os.path.join(datasets.GOLD, "alloc")
CASES = sorted("alloc/" + f[:-5] for f in os.listdir(DIR) if f.endswith(".json"))
BULK_CASES = [c for c in CASES if not datasets.has_barcodes(c)]
ALLOC_FLAGS = {"--allocate-multi-mappings": ("allocate_multi_mappings", 0),
               "--multi-mapping-allocation-distance": ("multi_mapping_allocation_distance", 1),
               "--multi-mapping-allocation-seed": ("multi_mapping_allocation_seed", 1)}


def golden(case):
    with gzip.open(os.path.join(datasets.GOLD, case + ".out.gz"), "rb") as f:
        return f.read()


def params_of(flags):
    """chromap flags of a fixture -> (preset, overrides): datasets.flags_to_params plus the three allocation options"""
    rest, kw = [], {}
    i = 0
    while i < len(flags):
        if flags[i] in ALLOC_FLAGS:
            name, takes_value = ALLOC_FLAGS[flags[i]]
            kw[name] = int(flags[i + 1]) if takes_value else 1
            i += 1 + takes_value
        else:
            rest.append(flags[i])
            i += 1
    preset, more = datasets.flags_to_params(rest)
    kw.update(more)
    return preset, kw


def counts(meta):
    a = meta["allocation"]
    return a["n_multi"], a["n_allocated"], a["n_without_overlap"]
