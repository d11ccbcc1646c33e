"""chromap-amd --output-csi: beside a --BAM file and beside a BGZF BED file it writes <output>.csi, a BGZF stream whose payload is the
plain-Python model's (tests/csi_model.py) of the written output, at depth 5 (no golden reference is longer than 2^29); region queries
through it return what a walk over the output returns; the output file is the one written without the flag, and beside --output-bai
the .bai is byte for byte the one of a run without --output-csi.  (A chromosome longer than 2^29 is not mapped here -- its reference
file alone has more than 500 MB; tests/test_gpu_csi.py covers the long coordinates through the library, with synthetic records.)"""
import gzip
import os
import re
import subprocess

import pytest

import bgzf_texts as bt
import csi_model as cm
import datasets
import tbi_texts as tt

pytestmark = pytest.mark.gpu
CLI = os.path.join(datasets.ROOT, "chromap_amd", "chromap-amd")


def _run(args):
    r = subprocess.run([CLI] + args, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    return r.stderr


def _payload(path, stderr):
    packed = open(path, "rb").read()
    assert packed.endswith(bt.EOF_BLOCK) and packed.count(bt.EOF_BLOCK) == 1
    bt.blocks(packed)
    payload = gzip.decompress(packed)
    m = re.search(rb"Built the CSI index \(depth (\d)\) on the device and wrote (\S+) \((\d+) bytes before compression\)", stderr)
    assert m and (int(m.group(1)), m.group(2).decode(), int(m.group(3))) == (5, path, len(payload)), stderr[-600:]
    return payload


def test_bam(tmp_path):
    import test_gpu_bai as tgb
    import test_gpu_bam as tb
    case = "s1_chip_sam"
    out, both = str(tmp_path / "out.bam"), str(tmp_path / "both.bam")
    stderr = _run(tb._cli_args(case) + ["--BAM", "--output-csi", "-o", out])
    raw = open(out, "rb").read()
    payload = _payload(out + ".csi", stderr)
    assert payload == cm.bam_model(raw, 5) and cm.parse_csi(payload)["depth"] == 5
    assert cm.check_bam_queries(raw, payload, tgb._regions_of(raw, case)) > 10
    # beside --output-bai: both files, the .bai that of a run without --output-csi
    stderr = _run(tb._cli_args(case) + ["--BAM", "--output-bai", "--output-csi", "-o", both])
    assert open(both, "rb").read() == raw and _payload(both + ".csi", stderr) == payload
    plain = str(tmp_path / "plain.bam")
    _run(tb._cli_args(case) + ["--BAM", "--output-bai", "-o", plain])
    assert open(plain, "rb").read() == raw, "the flag changes the BAM file"
    assert open(both + ".bai", "rb").read() == open(plain + ".bai", "rb").read()
    assert sorted(os.listdir(str(tmp_path))) == ["both.bam", "both.bam.bai", "both.bam.csi", "out.bam", "out.bam.csi", "plain.bam", "plain.bam.bai"]


def test_scatac_bed(tmp_path):
    import test_gpu_tabix as tx
    case = "b1_atac_bc"
    want = datasets.case_golden_bed(case)
    out = str(tmp_path / "out.bed.gz")
    stderr = _run(tx._cli_args(case) + ["--output-bgzf", "--output-csi", "--output-tbi", "-o", out])
    raw = open(out, "rb").read()
    assert gzip.decompress(raw) == want and raw.endswith(bt.EOF_BLOCK) and raw.count(bt.EOF_BLOCK) == 1
    payload = _payload(out + ".csi", stderr)
    assert payload == cm.bed_model(want, bt.blocks(raw[:-28]), 0, 5) and cm.parse_csi(payload)["depth"] == 5
    assert cm.check_bed_queries(raw, payload, want, tt.random_queries(want, 60)) > 60
    plain = str(tmp_path / "plain.bed.gz")
    _run(tx._cli_args(case) + ["--output-bgzf", "--output-tbi", "-o", plain])
    assert open(plain, "rb").read() == raw, "the flag changes the BED file"
    assert open(out + ".tbi", "rb").read() == open(plain + ".tbi", "rb").read()
    assert sorted(os.listdir(str(tmp_path))) == ["out.bed.gz", "out.bed.gz.csi", "out.bed.gz.tbi", "plain.bed.gz", "plain.bed.gz.tbi"]
