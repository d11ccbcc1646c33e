"""--output-tbi of chromap-amd as far as a box without a GPU can see it: the flag is known and documented, accepted where an index can
be built, and every combination that has no index is refused from the arguments alone -- before the output file is opened -- with a
message that names the flag."""
import os
import subprocess

import pytest

import datasets

CLI = os.path.join(datasets.ROOT, "chromap_amd", "chromap-amd")


def _run(*args):
    assert os.path.exists(CLI), "chromap-amd not built (python -c 'import __graft_entry__ as g; g.build()')"
    return subprocess.run([CLI] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_help_names_the_flag():
    r = _run("-h")
    assert r.returncode == 0 and b"--output-tbi" in r.stdout and b"<output>.tbi" in r.stdout


def test_the_flag_is_accepted_and_missing_files_are_what_fails(tmp_path):
    o = str(tmp_path / "o")
    for flags, reads in (([], ["-1", "a", "-2", "b"]), (["--preset", "atac"], ["-1", "a", "-2", "b", "-b", "c"]), (["--TagAlign"], ["-1", "a"]),
                         (["--barcode-translate", "t.tsv"], ["-1", "a", "-2", "b", "-b", "c"]), (["--BED"], ["-1", "a"])):
        r = _run("--output-bgzf", "--output-tbi", *flags, "-x", "x", "-r", "y", *reads, "-o", o)
        assert r.returncode != 0, flags
        assert b"unsupported option" not in r.stderr and b"--output-tbi" not in r.stderr and b"outside this build" not in r.stderr, (flags, r.stderr)
        assert b"Cannot find sequence file y" in r.stderr, (flags, r.stderr)
    assert os.listdir(tmp_path) == []


REFUSED = {
    "without_output_bgzf": ([], ["-1", "a", "-2", "b"], b"needs --output-bgzf"),
    "pairs": (["--output-bgzf", "--preset", "hic"], ["-1", "a", "-2", "b"], b"pairs output"),
    "pairs_flag": (["--output-bgzf", "--pairs"], ["-1", "a", "-2", "b"], b"pairs output"),
    "sam": (["--output-bgzf", "--SAM"], ["-1", "a", "-2", "b"], b"--SAM"),
    "paired_tagalign": (["--output-bgzf", "--TagAlign"], ["-1", "a", "-2", "b"], b"paired-end --TagAlign"),
    "gpus": (["--output-bgzf", "--gpus", "2"], ["-1", "a", "-2", "b"], b"--gpus > 1 or --force-exchange"),
    "force_exchange": (["--output-bgzf", "--force-exchange"], ["-1", "a", "-2", "b"], b"--gpus > 1 or --force-exchange"),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusals_come_from_the_arguments_alone_and_leave_the_output_alone(name, tmp_path):
    flags, reads, words = REFUSED[name]
    fa, _, _ = datasets.case_inputs("toy_atac")
    idx = datasets.case_index("toy_atac")
    out, tbi = tmp_path / "kept.bed.gz", tmp_path / "kept.bed.gz.tbi"
    args = ["--output-tbi"] + flags + ["-x", idx, "-r", fa] + reads + ["-o", str(out)]
    out.write_bytes(b"the last run's output\n")
    tbi.write_bytes(b"the last run's index\n")
    r = _run(*args)
    assert r.returncode != 0 and b"--output-tbi" in r.stderr and words in r.stderr, r.stderr
    assert b"unsupported option" not in r.stderr
    assert out.read_bytes() == b"the last run's output\n" and tbi.read_bytes() == b"the last run's index\n"
    out.unlink()
    tbi.unlink()
    r = _run(*args)
    assert r.returncode != 0 and words in r.stderr
    assert os.listdir(tmp_path) == []
