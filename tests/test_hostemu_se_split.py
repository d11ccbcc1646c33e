"""Single-end reads with split alignment through the stage functions compiled for the host (cm_emit_single_record's split form,
cm_stages.h): the text equals the reference's own output byte for byte (tests/golden/se_split) and the counters equal its stderr
counters.  Without the split form the non-split record is produced and every case fails."""
import hashlib

import pytest

import hostemu_lib as he
import oracle_lib as ol
import se_split_cases as sc


def _check_counters(case, st, keys):
    ref = sc.meta(case)["reference_stderr_counters"]
    s = st.as_dict()
    for key in keys:
        assert s[key] == ref[key], key


def _check_text(case, path, lines=None):
    got = open(path, "rb").read()
    want = sc.golden(case)
    assert got == want, sc.first_difference(got, want)
    m = sc.meta(case)
    assert hashlib.md5(got).hexdigest() == m["output_md5"] and len(got) == m["output_bytes"]
    if lines is not None:
        assert lines == m["reference_stderr_counters"]["num_output"]


def test_fixtures_reach_the_split_code():
    """what the maker checked and recorded: reads that were cut on both strands, multi-mappers beyond -n"""
    assert len(sc.CASES) == 6
    for case in sc.CASES:
        m = sc.meta(case)
        assert m["cut_records"]["plus"] >= 100 and m["cut_records"]["minus"] >= 100, case
        assert m["differs_from_non_split_output"] is True
        if "-n" in m["chromap_flags"]:
            assert m["reads_with_more_best_mappings_than_n"] > 0


@pytest.mark.parametrize("case", [c for c in sc.CASES if not sc.is_sam(c) and not sc.has_barcodes(c)])
def test_bed_and_tagalign_match_reference(case, tmp_path):
    fa, fq = sc.inputs(case)
    kw = sc.params_kw(case)
    h = he.HostEmu(sc.index(case), fa, he.params(**kw))
    b, off = ol.read_fastx(fq)
    rec, k, st = h.map_single(b, off)
    out = str(tmp_path / "e.txt")
    if sc.is_tagalign(case):  # text by the oracle's writer, as for the other single-end TagAlign cases
        o = ol.Oracle(sc.index(case), fa, ol.params(**kw))
        o.p.output_format = 2
        lines = ol.write_bed_se(o, rec, k, out)
        o.close()
    else:
        lines = h.write_bed_se(rec, k, out)
    _check_text(case, out, lines)
    _check_counters(case, st, sc.COUNTERS)


@pytest.mark.parametrize("case", [c for c in sc.CASES if sc.has_barcodes(c)])
def test_barcoded_bed_matches_reference(case, tmp_path):
    fa, fq = sc.inputs(case)
    bcf, wlf = sc.barcode_inputs(case)
    kw = sc.params_kw(case)
    h = he.HostEmu(sc.index(case), fa, he.params(**kw))
    b, off = ol.read_fastx(fq)
    bc, bcq, bco = ol.read_fastq_qual(bcf)
    wl = ol.Whitelist(wlf, int(bco[1] - bco[0]))
    assert wl.abundance(bc, bco) > 0
    keys, _ = wl.export()
    rec, k, st = h.map_single_bc(b, off, bc.copy(), bcq, bco, keys)
    o = ol.Oracle(sc.index(case), fa, ol.params(**kw))
    out = str(tmp_path / "e.bed")
    lines = ol.write_se_bc(o, rec, k, wl.barcode_length, wl, False, out)
    o.close()
    _check_text(case, out, lines)
    _check_counters(case, st, sc.BC_COUNTERS)


@pytest.mark.parametrize("case", [c for c in sc.CASES if sc.is_sam(c)])
def test_sam_matches_reference(case, tmp_path):
    fa, fq = sc.inputs(case)
    h = he.HostEmu(sc.index(case), fa, he.params(**sc.params_kw(case)))
    b, q, off = ol.read_fastq_qual(fq)
    so, st = he.map_sam(h, b, off)
    out = str(tmp_path / "e.sam")
    lines = he.write_sam(h.L, h.ref, h.p, so, False, ol.read_names(fq), None, b, q, off, None, None, None, out)
    _check_text(case, out, lines)
    _check_counters(case, st, sc.COUNTERS)
