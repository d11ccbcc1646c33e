"""--output-bgzf of chromap-amd as far as a box without a GPU can see it: the flag is known and documented, and the two SAM routes whose
text the host renders refuse it from the arguments alone -- before the output file is opened."""
import os
import subprocess

import datasets

CLI = os.path.join(datasets.ROOT, "chromap_amd", "chromap-amd")


def _run(*args):
    assert os.path.exists(CLI), "chromap-amd not built (python -c 'import __graft_entry__ as g; g.build()')"
    return subprocess.run([CLI] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_help_names_the_flag():
    r = _run("-h")
    assert r.returncode == 0 and b"--output-bgzf" in r.stdout


def test_the_flag_is_accepted_and_missing_files_are_what_fails(tmp_path):
    o = str(tmp_path / "o")
    for flags in ([], ["--preset", "hic"], ["--SAM"], ["--TagAlign"], ["--force-exchange"]):
        r = _run("--output-bgzf", *flags, "-x", "x", "-r", "y", "-1", "a", "-2", "b", "-o", o)
        assert r.returncode != 0, flags
        assert b"unsupported option" not in r.stderr and b"--output-bgzf" not in r.stderr and b"outside this build" not in r.stderr, (flags, r.stderr)
        assert b"Cannot find sequence file y" in r.stderr, (flags, r.stderr)


def _host_rendered(out):
    fa, _, _ = datasets.case_inputs("toy_atac")
    idx = datasets.case_index("toy_atac")
    return (["--output-bgzf", "--host-ingest", "--SAM", "-x", idx, "-r", fa, "-1", "a.fq", "-2", "b.fq", "-o", out],
            ["--SAM", "--barcode-translate", "t.tsv", "--output-bgzf", "-x", idx, "-r", fa, "-1", "a.fq", "-2", "b.fq", "-b", "c.fq", "-o", out])


def test_host_rendered_sam_routes_refuse_the_flag_and_leave_the_output_alone(tmp_path):
    out = tmp_path / "kept.sam"
    for args in _host_rendered(str(out)):
        out.write_bytes(b"@SQ\tSN:last\tLN:1\n")
        r = _run(*args)
        assert r.returncode != 0 and b"--output-bgzf" in r.stderr and b"the host renders that text" in r.stderr, r.stderr
        assert b"unsupported option" not in r.stderr
        assert out.read_bytes() == b"@SQ\tSN:last\tLN:1\n"
        out.unlink()
        r = _run(*args)
        assert r.returncode != 0 and b"the host renders that text" in r.stderr
        assert os.listdir(tmp_path) == []
