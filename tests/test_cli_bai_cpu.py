"""chromap-amd --output-bai on a box without a GPU: the flag is known, it is refused without --BAM from the arguments alone -- before a
file is opened or a GPU touched -- and with --BAM it gets past the argument checks."""
import os
import subprocess

import pytest

import datasets

CLI = os.path.join(datasets.ROOT, "chromap_amd", "chromap-amd")
BASE = ["-x", "x", "-r", "y", "-1", "a"]
NEEDS_BAM = b"--output-bai needs --BAM"


def _run(*args):
    return subprocess.run([CLI] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE)


@pytest.mark.parametrize("flags", [["--output-bai"], ["--SAM", "--output-bai"], ["--output-bai", "--SAM"], ["--BAM", "--BED", "--output-bai"],
                                   ["--BAM", "--output-bai", "--SAM"], ["--output-bgzf", "--output-bai"]], ids=lambda f: " ".join(f))
def test_refused_without_bam(flags, tmp_path):
    out = tmp_path / "kept.bam"
    out.write_bytes(b"last run's output")
    for o in (out, tmp_path / "new.bam"):
        r = _run(*flags, *BASE, "-o", str(o))
        assert r.returncode != 0 and NEEDS_BAM in r.stderr, r.stderr
        assert b"unsupported option" not in r.stderr
    assert out.read_bytes() == b"last run's output", "a refused invocation leaves an existing output file alone"
    assert sorted(p.name for p in tmp_path.iterdir()) == ["kept.bam"], "... and creates none, no index either"


def test_refused_with_real_inputs_leaves_the_output_alone(tmp_path):
    fa, r1, r2 = datasets.case_inputs("toy_atac")
    out = tmp_path / "kept.bam"
    out.write_bytes(b"last run's output")
    r = _run("--SAM", "--output-bai", "-x", datasets.case_index("toy_atac"), "-r", fa, "-1", r1, "-2", r2, "-o", str(out))
    assert r.returncode != 0 and NEEDS_BAM in r.stderr, r.stderr
    assert out.read_bytes() == b"last run's output"
    assert sorted(p.name for p in tmp_path.iterdir()) == ["kept.bam"]


@pytest.mark.parametrize("flags", [["--BAM", "--output-bai"], ["--output-bai", "--BAM"], ["--preset", "chip", "--BAM", "--output-bai", "--summary", "s.csv"]],
                         ids=lambda f: " ".join(f))
def test_with_bam_gets_past_the_argument_checks(flags, tmp_path):
    """... and fails on the missing files, not on the flag"""
    o = tmp_path / "o.bam"
    r = _run(*flags, *BASE, "-o", str(o))
    assert r.returncode != 0
    assert b"unsupported option" not in r.stderr and b"outside this build" not in r.stderr and NEEDS_BAM not in r.stderr, r.stderr
    assert b"Cannot find sequence file y" in r.stderr, r.stderr
    assert list(tmp_path.iterdir()) == []


def test_what_bam_refuses_stays_refused_in_its_words(tmp_path):
    for flags, message in ((["--BAM", "--output-bai", "-n", "2"], b"--BAM with -n > 1 is outside this build"),
                           (["--BAM", "--output-bai", "--output-tbi"], b"--output-tbi with --BAM is outside this build"),
                           (["--BAM", "--output-bai", "--host-ingest"], b"--BAM with --host-ingest is outside this build"),
                           (["--BAM", "--output-bai", "--gpus", "2"], b"--BAM with --gpus > 1 or --force-exchange is outside this build")):
        r = _run(*flags, *BASE, "-o", str(tmp_path / "o.bam"))
        assert r.returncode != 0 and message in r.stderr, (flags, r.stderr)
    assert list(tmp_path.iterdir()) == []


def test_help_names_the_flag():
    r = _run("-h")
    assert r.returncode == 0 and b"--output-bai" in r.stdout and b"<output>.bai" in r.stdout
    assert b"no index (.bai) is written" not in r.stdout
    r = _run("--PAF", *BASE, "-o", "o")
    assert r.returncode != 0 and b"unsupported option --PAF" in r.stderr
