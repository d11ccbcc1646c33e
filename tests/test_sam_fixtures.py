"""The committed gap-rich SAM fixtures (made by the reference binary, tests/golden/make_golden.py) checked from scratch against the
regenerated reference sequence: every CIGAR consumes exactly its read and its span, NM and MD recomputed equal the text, the
CIGAR's affine score is the plain unbanded global optimum over the reported span, and the fixtures stay gap-rich."""
import pytest

import datasets
import plain_align as pa
import sam_check as sc

GAP_SAM_CASES = ["x2_gaps_sam_q0", "x4_gaps_hic_sam_q0", "x5_gaps_e15_sam_q0", "x6_gaps_se_sam_q0"]
BAND_BINDING = sc.BAND_BINDING
READ_LENGTH = {"x4_gaps_hic_sam_q0": 100}


def checkable(case, recs):
    """split alignment prints SEQ cut to the CIGAR's query length, from the front of the stored read whichever part was aligned
    (sam_mapping.h:186-193): of the hic fixture, the records that print the whole read are replayed; the cut ones get
    sam_check.check_cut_record"""
    if case in READ_LENGTH:
        return [r for r in recs if len(r["seq"]) == READ_LENGTH[case]]
    return recs


@pytest.mark.parametrize("case", GAP_SAM_CASES)
def test_gap_rich_sam_fixture(case):
    fa, _, _ = datasets.case_inputs(case)
    ref = sc.load_fasta(fa)
    recs = sc.records(datasets.case_golden_bed(case))
    gapped = long_gap = near_end = 0
    binding = set()
    some = checkable(case, recs)
    assert len(some) * 2 >= len(recs)  # (the hic fixture: most records print the whole read)
    for r in recs:
        if len(some) < len(recs) and len(r["seq"]) != READ_LENGTH[case]:
            sc.check_cut_record(r)
    for r in some:
        score, span = sc.check_record(r, ref)
        # a record without a difference scores its length, the most any alignment of the read can
        if case in BAND_BINDING and r["nm"] > 0 and pa.global_affine(span, r["seq"]) != score:
            binding.add(r["name"])
    for r in recs:
        g, lg, ne = sc.gap_profile(r)
        gapped += g
        long_gap += lg
        near_end += ne
    if case in BAND_BINDING:
        assert binding == set(BAND_BINDING[case])
        assert len(BAND_BINDING[case]) * 100 <= len(recs)
    assert gapped * 4 >= len(recs), (gapped, len(recs))
    assert long_gap >= 200
    assert near_end >= 100
