"""chromap-amd --output-csi on a box without a GPU: the flag is known; it is refused from the arguments alone -- before a file is
opened or a GPU touched -- in the settings where --output-tbi / --output-bai are refused (SAM text, pairs, paired-end TagAlign,
more than one GPU, no BGZF), each with its reason; with --BAM and with --output-bgzf BED it gets past the argument checks, beside
--output-bai / --output-tbi too."""
import os
import subprocess

import pytest

import datasets

CLI = os.path.join(datasets.ROOT, "chromap_amd", "chromap-amd")
SE = ["-x", "x", "-r", "y", "-1", "a"]
PE = SE + ["-2", "b"]

REFUSED = {
    "sam": (["--SAM", "--output-bgzf", "--output-csi"], SE, b"--output-csi with --SAM is outside this build"),
    "sam_after_bam": (["--BAM", "--SAM", "--output-bgzf", "--output-csi"], SE, b"--output-csi with --SAM is outside this build"),
    "pairs": (["--pairs", "--output-bgzf", "--output-csi"], PE, b"--output-csi with pairs output is outside this build"),
    "tagalign_paired": (["--TagAlign", "--output-bgzf", "--output-csi"], PE, b"--output-csi with paired-end --TagAlign is outside this build"),
    "gpus_2": (["--output-bgzf", "--output-csi", "--gpus", "2"], PE, b"--output-csi with --gpus > 1 or --force-exchange is outside this build"),
    "force_exchange": (["--output-bgzf", "--output-csi", "--force-exchange"], PE, b"--output-csi with --gpus > 1 or --force-exchange is outside this build"),
    "no_bgzf_bed": (["--output-csi"], PE, b"--output-csi needs --BAM or --output-bgzf"),
    "no_bgzf_tagalign": (["--TagAlign", "--output-csi"], SE, b"--output-csi needs --BAM or --output-bgzf"),
    "no_bgzf_sam": (["--SAM", "--output-csi"], SE, b"--output-csi needs --BAM or --output-bgzf"),
    "bam_gpus_2": (["--BAM", "--output-csi", "--gpus", "2"], SE, b"--BAM with --gpus > 1 or --force-exchange is outside this build"),
}


def _run(*args):
    return subprocess.run([CLI] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE)


@pytest.mark.parametrize("kind", sorted(REFUSED))
def test_refused_from_the_arguments_alone(kind, tmp_path):
    flags, reads, message = REFUSED[kind]
    out = tmp_path / "kept.out"
    out.write_bytes(b"last run's output")
    for o in (out, tmp_path / "new.out"):
        r = _run(*flags, *reads, "-o", str(o))
        assert r.returncode != 0 and message in r.stderr, r.stderr
        assert b"unsupported option" not in r.stderr
    assert out.read_bytes() == b"last run's output", "a refused invocation leaves an existing output file alone"
    assert sorted(p.name for p in tmp_path.iterdir()) == ["kept.out"], "... and creates none, no index either"


ACCEPTED = {
    "bam": (["--BAM", "--output-csi"], SE),
    "bam_paired_with_bai": (["--preset", "chip", "--BAM", "--output-bai", "--output-csi"], PE),
    "bed_bgzf": (["--output-bgzf", "--output-csi"], PE),
    "bed_bgzf_with_tbi": (["--output-csi", "--output-tbi", "--output-bgzf"], PE),
    "tagalign_single_end": (["--TagAlign", "--output-bgzf", "--output-csi"], SE),
}


@pytest.mark.parametrize("kind", sorted(ACCEPTED))
def test_gets_past_the_argument_checks(kind, tmp_path):
    """... and fails on the missing files, not on the flag"""
    flags, reads = ACCEPTED[kind]
    r = _run(*flags, *reads, "-o", str(tmp_path / "o"))
    assert r.returncode != 0
    assert b"unsupported option" not in r.stderr and b"outside this build" not in r.stderr and b"--output-csi needs" not in r.stderr, r.stderr
    assert b"Cannot find sequence file y" in r.stderr, r.stderr
    assert list(tmp_path.iterdir()) == []


def test_help_names_the_flag():
    r = _run("-h")
    assert r.returncode == 0 and b"--output-csi" in r.stdout and b"<output>.csi" in r.stdout
