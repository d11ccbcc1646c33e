"""--summary at scale against the REFERENCE BINARY (in the manner of tests/test_gpu_scale.py): scATAC, 4 M pairs, the 737 280-barcode
whitelist, the reference at -t 16.  Same barcodes in the same row order, the first five columns identical in every row -- no row is
left out.  The four cache columns are the only thing not compared (chromap-amd does not model the reference's minimizer cache and
writes zeros); how many reference rows had a non-zero cachehit is recorded in the test's output, so the size of the ignored part is known."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.slow]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "chromap")


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/chromap not built")
def test_scatac_summary_equals_reference_binary(tmp_path, record_property):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "ref_baseline.py"), "--genome", "400000000", "--nseq", "24", "--dir", str(tmp_path / "w"),
           "--seed0", "9000", "--preset", "atac", "--pairs", "2000000", "--batches", "2", "--barcodes", "737280", "--threads", "16", "--summary"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    r = json.loads(p.stdout.decode().strip().splitlines()[-1])
    assert "error" not in r and "error" not in r["reference"] and "error" not in r["chromap_amd"], r
    s = r["summary"]
    print("summary at scale:", json.dumps(s))
    record_property("reference_rows_with_cachehit", s["reference_rows_with_cachehit"])
    record_property("reference_cachehit_total", s["reference_cachehit_total"])
    assert r["pairs"] >= 4_000_000 and r["bed_identical_to_reference"] is True
    assert s["header_identical"] and s["rows_reference"] == s["rows_chromap_amd"] > 100_000
    assert s["same_barcodes_same_order"] is True
    assert s["rows_differing_in_first_five_columns"] == 0
