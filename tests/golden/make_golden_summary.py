#!/usr/bin/env python3
"""Regenerates tests/golden/summary/*.csv.gz + *.json: the --summary CSV the REFERENCE writes (oracle/_ref/chromap, -t 1) for inputs
that make_golden.py already defines.

The whole file is a fair byte-for-byte demand only while the reference's minimizer cache never answers a read (its per-barcode
hit counts depend on the thread schedule, and this project does not model the cache): the script asserts that every `cachehit`
of a fixture is 0 and refuses to write one where it is not.  Each JSON names the golden case whose inputs were mapped, the flags,
and the md5 of the mapping output of that very run (BED / pairs / SAM), so a test can tell that --summary changed nothing else.
"""
import gzip
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

OUT = os.path.join(HERE, "summary")

# name -> (golden case whose inputs are mapped, mapping flags, barcodes: None = none, "wl" = with the whitelist, "nowl" = without,
#          golden output of an existing case these flags reproduce, or None)
CASES = {
    "b1_atac_bc": ("b1_atac_bc", ["--preset", "atac"], "wl", "b1_atac_bc"),
    "b3_bulk_level_bc_q0": ("b3_bulk_level_bc_q0", ["--preset", "atac", "--remove-pcr-duplicates-at-bulk-level", "-q", "0"], "wl",
                            "b3_bulk_level_bc_q0"),
    "b1_inmem_bc": ("b1_inmem_bc", ["-l", "2000", "--remove-pcr-duplicates", "--Tn5-shift", "--trim-adapters"], "wl", "b1_inmem_bc"),
    "b1_se_bc": ("b1_se_bc", ["--preset", "atac"], "wl", "b1_se_bc"),
    "b1_atac_bc_keep": ("b1_atac_bc", ["--preset", "atac", "--output-mappings-not-in-whitelist"], "wl", None),
    "b1_atac_bc_nowl": ("b1_atac_bc", ["--preset", "atac"], "nowl", None),
    "b1_bulk_chip": ("b1_atac_bc", ["--preset", "chip"], None, None),
    "s1_se_chip": ("s1_se_chip", ["--preset", "chip"], None, "s1_se_chip"),
    "h1_hic_dedup": ("h1_hic", ["--preset", "hic", "--remove-pcr-duplicates"], None, None),
    "s1_chip_sam": ("s1_chip_sam", ["--preset", "chip", "--SAM"], None, "s1_chip_sam"),
    "b1_bc_sam": ("b1_bc_sam", ["--preset", "atac", "--SAM"], "wl", "b1_bc_sam"),
    "b1_atac_bc_noslots": ("b1_atac_bc", ["--preset", "atac", "--turn-off-num-uniq-cache-slots"], "wl", None),
    "b1_atac_bc_nowl_noslots": ("b1_atac_bc", ["--preset", "atac", "--turn-off-num-uniq-cache-slots"], "nowl", None),
}


def main():
    only = set(sys.argv[1:])
    os.makedirs(OUT, exist_ok=True)
    for name, (base, flags, bc, golden) in CASES.items():
        if only and name not in only:
            continue
        gen = mg.CASES[base][0]
        tmp = tempfile.mkdtemp(prefix="golden_summary_")
        try:
            subprocess.check_call([sys.executable, mg.GEN, "--out", os.path.join(tmp, "d")] + gen)
            fa, r1, r2 = (os.path.join(tmp, f) for f in ("d.fa", "d_1.fq", "d_2.fq"))
            idx = os.path.join(tmp, "d.idx")
            subprocess.check_call([mg.REF, "-i", "-r", fa, "-o", idx], stderr=subprocess.DEVNULL)
            mate = mg.SINGLE_END.get(base, 0)
            reads = ["-1", r1, "-2", r2] if not mate else ["-1", r1 if mate == 1 else r2]
            extra = []
            if bc:
                extra = ["-b", os.path.join(tmp, "d_bc.fq")]
                if bc == "wl":
                    extra += ["--barcode-whitelist", os.path.join(tmp, "d.whitelist.txt")]
            out, csv = os.path.join(tmp, "out.txt"), os.path.join(tmp, "summary.csv")
            subprocess.run([mg.REF] + flags + extra + ["-x", idx, "-r", fa] + reads + ["-o", out, "--summary", csv, "-t", "1"],
                           stderr=subprocess.PIPE, check=True)
            text = open(csv, "rb").read()
            lines = text.decode().splitlines()
            header = lines[0].split(",")
            assert header[:6] == ["barcode", "total", "duplicate", "unmapped", "lowmapq", "cachehit"], header
            hits = [ln.split(",")[5] for ln in lines[1:]]
            assert all(h == "0" for h in hits), "%s: the reference's cache answered reads; the case cannot be a byte-exact fixture" % name
            meta = {"base_case": base, "chromap_flags": flags, "barcodes": bc, "single_end_mate": mate, "golden_output": golden,
                    "output_md5": mg.md5(out), "summary_md5": hashlib.md5(text).hexdigest(), "rows": len(lines) - 1,
                    "input_md5": {"fa": mg.md5(fa), "r1": mg.md5(r1), "r2": mg.md5(r2)}}
            with gzip.GzipFile(os.path.join(OUT, name + ".csv.gz"), "wb", mtime=0) as g:
                g.write(text)
            with open(os.path.join(OUT, name + ".json"), "w") as f:
                json.dump(meta, f, indent=1, sort_keys=True)
            print(name, len(lines) - 1, "rows;", lines[-1])
        finally:
            shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
