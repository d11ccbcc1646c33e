"""The plain-Python BAM index (tests/bai_model.py) on the synthetic record sets (tests/bai_records.py): region queries through the
index it builds find what a walk over all records finds, the sets that cannot be indexed are refused with their cause and record, and
one small file's index is the payload worked out by hand from the SAM specification below -- the anchor that keeps the model from
being checked against itself only."""
import struct

import pytest

import bai_model as bai
import bai_records as br
import bgzf_texts as bt


def _file(rs):
    return rs.file(bai.bgzf_blocks_of(rs.data))


@pytest.mark.parametrize("name", br.good())
def test_queries_through_the_index_equal_the_brute_force(name):
    rs = br.sets()[name]
    raw = _file(rs)
    payload = bai.model(raw)
    index, n_no_coor = bai.parse_bai(payload)
    f = bai.File(raw)
    assert len(index) == rs.n_ref == f.n_ref and n_no_coor == 0
    assert [at - f.first_record for at, *_ in bai.records(f)] == rs.starts[:-1]
    found = 0
    for tid, beg, end in br.regions(rs):
        got, want = bai.query(f, index, tid, beg, end), bai.brute(f, tid, beg, end)
        assert got == want, (tid, beg, end)
        found += len(want)
    assert found or not rs.starts[1:], "the regions find records"
    # what the index says about every reference is what the records say
    per_ref = [[r for r in bai.records(f) if r[2] == t] for t in range(rs.n_ref)]
    for t, r in enumerate(index):
        if not per_ref[t]:
            assert r["bins"] == {} and r["pseudo"] is None and r["lin"] == []
            continue
        assert r["order"] == sorted(r["order"])
        assert r["pseudo"] == (f.voff(per_ref[t][0][0]), f.voff(per_ref[t][-1][0] + per_ref[t][-1][1]), sum(1 for x in per_ref[t] if not x[5] & 4),
                               sum(1 for x in per_ref[t] if x[5] & 4))
        assert len(r["lin"]) == max((x[4] - 1) >> 14 for x in per_ref[t]) + 1
        assert r["lin"] == sorted(r["lin"])


def test_chunks_of_interleaved_bins():
    """A B A within one block: one chunk for A; with more than a block of B between: two"""
    for name, want in (("bins_a_b_a_near", 1), ("bins_a_b_a_far", 2)):
        index, _ = bai.parse_bai(bai.model(_file(br.sets()[name])))
        assert len(index[0]["bins"][585]) == want, name


@pytest.mark.parametrize("name", [n for n in br.refused() if br.sets()[n].chain])
def test_refused_sets(name):
    rs = br.sets()[name]
    with pytest.raises(bai.NotIndexable) as e:
        bai.model(_file(rs))
    assert (e.value.cause, e.value.record) == rs.refused


def test_a_file_worked_out_by_hand():
    # Two references; three records of 48 bytes each (br.PLAIN), all in the second block of the file:
    #   r0: ref0, pos 100,   5M  -> [100, 105):     window 0;        bin 4681 + (100 >> 14) = 4681
    #   r1: ref0, pos 16380, 10M -> [16380, 16390): windows 0 and 1; 16380 >> 14 = 0 but 16389 >> 14 = 1, 16380 >> 17 == 16389 >> 17 = 0: bin 585 + 0
    #   r2: ref1, pos 40000, 5M  -> [40000, 40005): window 2 (40000 >> 14);  bin 4681 + 2 = 4683
    # The header takes one block of H bytes, the records one block of R bytes; the file ends with the 28-byte end-of-file block.
    # Virtual offsets: v0 = H << 16 | 0, v1 = H << 16 | 48, v2 = H << 16 | 96; the records end where the next block begins: ve = (H + R) << 16.
    # SAM spec 5.2:  magic, n_ref = 2
    #   ref0: n_bin = 3 (two bins and the pseudo-bin), in ascending order:
    #           bin 585,  1 chunk (v1, v2);   bin 4681, 1 chunk (v0, v1)
    #           bin 37450, 2 chunks: (ref_beg, ref_end) = (v0, v2), (n_mapped, n_unmapped) = (2, 0)
    #         n_intv = 2: window 0 -> v0 (r0 is the first record that overlaps it), window 1 -> v1
    #   ref1: n_bin = 2: bin 4683, 1 chunk (v2, ve);   bin 37450: (v2, ve), (1, 0)
    #         n_intv = 3: windows 0 and 1 hold no record and take window 2's offset: v2, v2, v2
    #   n_no_coor = 0
    recs = [br.record(0, 100), br.record(0, 16380, ((10, "M"),)), br.record(1, 40000)]
    assert [len(r) for r in recs] == [48, 48, 48]
    head, body = bai.bgzf_blocks_of(bai.bam_header(2)), bai.bgzf_blocks_of(b"".join(recs))
    assert len(bt.blocks(head)) == 1 and len(bt.blocks(body)) == 1
    H, R = len(head), len(body)
    v0, v1, v2, ve = H << 16, H << 16 | 48, H << 16 | 96, (H + R) << 16
    want = b"BAI\1" + struct.pack("<I", 2)
    want += struct.pack("<I", 3)
    want += struct.pack("<IiQQ", 585, 1, v1, v2) + struct.pack("<IiQQ", 4681, 1, v0, v1) + struct.pack("<IiQQQQ", 37450, 2, v0, v2, 2, 0)
    want += struct.pack("<iQQ", 2, v0, v1)
    want += struct.pack("<I", 2)
    want += struct.pack("<IiQQ", 4683, 1, v2, ve) + struct.pack("<IiQQQQ", 37450, 2, v2, ve, 1, 0)
    want += struct.pack("<iQQQ", 3, v2, v2, v2)
    want += struct.pack("<Q", 0)
    assert bai.model(head + body + bt.EOF_BLOCK) == want
