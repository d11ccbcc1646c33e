"""The command line of --allocate-multi-mappings, as far as it goes without a GPU: the options parse, the help names them, and the
combinations this build has no stage for are refused from the arguments alone -- before any file is opened or emptied."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "chromap_amd", "chromap-amd")
ALLOC = ["--allocate-multi-mappings", "--multi-mapping-allocation-distance", "200", "--multi-mapping-allocation-seed", "7"]

pytestmark = pytest.mark.skipif(not os.path.exists(CLI), reason="chromap-amd is not built")


def run(args):
    return subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)


def test_help_names_the_options():
    out = run(["-h"]).stdout.decode()
    for o in ("--allocate-multi-mappings", "--multi-mapping-allocation-distance", "--multi-mapping-allocation-seed"):
        assert o in out


@pytest.mark.parametrize("extra,word", [
    (["--SAM"], "--SAM"),
    (["--pairs", "-2", "r2.fq"], "pairs"),
    (["--summary", "s.csv"], "--summary"),
    (["--gpus", "2"], "--gpus"),
    (["--force-exchange"], "--force-exchange"),
])
def test_refused_combinations(extra, word, tmp_path):
    out = tmp_path / "out.txt"
    out.write_bytes(b"precious\n")
    r = run(ALLOC + ["-x", "no.idx", "-r", "no.fa", "-1", "r1.fq", "-o", str(out)] + extra)
    err = r.stderr.decode()
    assert r.returncode != 0
    assert "--allocate-multi-mappings" in err and word in err, err
    assert "unsupported option" not in err
    assert out.read_bytes() == b"precious\n"


@pytest.mark.parametrize("extra", [[], ["--TagAlign"], ["-2", "r2.fq", "--remove-pcr-duplicates"],
                                   # the reference allocates nothing in low-memory mode: there the flag is accepted with anything
                                   ["--low-mem", "--SAM"], ["--preset", "hic", "-2", "r2.fq"], ["--preset", "atac", "--summary", "s.csv"]])
def test_accepted_invocations_fail_on_the_missing_files(extra, tmp_path):
    r = run(ALLOC + ["-x", str(tmp_path / "no.idx"), "-r", str(tmp_path / "no.fa"), "-1", str(tmp_path / "r1.fq"), "-o", str(tmp_path / "o")] + extra)
    err = r.stderr.decode()
    assert r.returncode != 0
    assert "unsupported option" not in err and "outside this build" not in err and "missing value" not in err, err
    assert "no.fa" in err or "no.idx" in err, err


def test_options_need_their_values():
    for o in ("--multi-mapping-allocation-distance", "--multi-mapping-allocation-seed"):
        r = run(["-x", "i", "-r", "f", "-1", "r", "-o", "o", o])
        assert r.returncode != 0 and "missing value for " + o in r.stderr.decode()
