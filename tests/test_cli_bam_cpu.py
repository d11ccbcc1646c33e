"""chromap-amd --BAM on a box without a GPU: the flag is known, and every combination this build does not write is refused from the
arguments alone -- before a file is opened or a GPU touched -- with a message that says "outside this build"."""
import os
import subprocess

import pytest

import datasets

CLI = os.path.join(datasets.ROOT, "chromap_amd", "chromap-amd")
BASE = ["-x", "x", "-r", "y", "-1", "a"]

REFUSALS = [
    (["--BAM", "--host-ingest"], b"--BAM with --host-ingest is outside this build"),
    (["--BAM", "--barcode-translate", "t.tsv"], b"--BAM with --barcode-translate is outside this build"),
    (["--BAM", "-n", "2"], b"--BAM with -n > 1 is outside this build"),
    (["--BAM", "--output-tbi"], b"--output-tbi with --BAM is outside this build"),
    (["--BAM", "--output-bgzf", "--output-tbi"], b"--output-tbi with --BAM is outside this build"),
    (["--BAM", "--gpus", "2"], b"--BAM with --gpus > 1 or --force-exchange is outside this build"),
    (["--BAM", "--force-exchange"], b"--BAM with --gpus > 1 or --force-exchange is outside this build"),
    (["--BAM", "--allocate-multi-mappings"], b"--allocate-multi-mappings with --BAM is outside this build"),
]


def _run(*args):
    return subprocess.run([CLI] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE)


@pytest.mark.parametrize("flags,message", REFUSALS, ids=[" ".join(f) for f, _ in REFUSALS])
def test_refusals(flags, message, tmp_path):
    out = tmp_path / "kept.bam"
    new = tmp_path / "new.bam"
    out.write_bytes(b"last run's output")
    for o in (out, new):
        r = _run(*flags, *BASE, "-o", str(o))
        assert r.returncode != 0 and message in r.stderr, r.stderr
        assert b"unsupported option" not in r.stderr
    assert out.read_bytes() == b"last run's output", "a refused invocation leaves an existing output file alone"
    assert sorted(p.name for p in tmp_path.iterdir()) == ["kept.bam"], "... and creates none"


def test_refusals_with_real_inputs_leave_the_output_alone(tmp_path):
    """the same with a reference and an index that exist: nothing is read, opened or emptied before the arguments are checked"""
    fa, r1, r2 = datasets.case_inputs("toy_atac")
    idx = datasets.case_index("toy_atac")
    out = tmp_path / "kept.bam"
    for flags, message in REFUSALS:
        out.write_bytes(b"last run's output")
        r = _run(*flags, "-x", idx, "-r", fa, "-1", r1, "-2", r2, "-o", str(out))
        assert r.returncode != 0 and message in r.stderr, (flags, r.stderr)
        assert out.read_bytes() == b"last run's output"
    assert sorted(p.name for p in tmp_path.iterdir()) == ["kept.bam"]


@pytest.mark.parametrize("flags", [["--BAM"], ["--BAM", "--output-bgzf"], ["--BAM", "--summary", "s.csv"], ["--BAM", "--low-mem", "--allocate-multi-mappings"],
                                   ["--BAM", "--remove-pcr-duplicates", "-q", "0"], ["--preset", "chip", "--BAM"]],
                         ids=lambda f: " ".join(f))
def test_accepted_flags_get_past_the_argument_checks(flags, tmp_path):
    """... and fail on the missing files, not on the flag"""
    o = tmp_path / "o"
    r = _run(*flags, *BASE, "-o", str(o))
    assert r.returncode != 0
    assert b"unsupported option" not in r.stderr and b"outside this build" not in r.stderr, r.stderr
    assert b"Cannot find sequence file y" in r.stderr, r.stderr
    assert not o.exists()


def test_a_later_format_flag_takes_bam_back(tmp_path):
    """--BAM --SAM is --SAM: -n 2 is then refused in SAM's words, and --output-tbi in those of SAM text"""
    r = _run("--BAM", "--SAM", "-n", "2", *BASE, "-o", str(tmp_path / "o"))
    assert r.returncode != 0 and b"--SAM with -n > 1" in r.stderr
    r = _run("--SAM", "--BAM", "-n", "2", *BASE, "-o", str(tmp_path / "o"))
    assert r.returncode != 0 and b"--BAM with -n > 1" in r.stderr
    r = _run("--BAM", "--BED", "--output-tbi", *BASE, "-o", str(tmp_path / "o"))
    assert r.returncode != 0 and b"--output-tbi needs --output-bgzf" in r.stderr


def test_help_names_the_flag():
    r = _run("-h")
    assert r.returncode == 0 and b"--BAM" in r.stdout and b"|--SAM|--BAM" in r.stdout
