"""The sequential model of the CSI index (tests/csi_model.py) against the specification's own arithmetic, against brute force and
against the models already trusted: at depth 5 its bins and chunks are those of the .bai / .tbi model's payload and every loffset is
that payload's linear-index entry at the bin's first window; region queries through it -- reg2bins for any depth, min_off from the
bins' loffsets -- return what a walk over the records or a scan of the text returns, with every hit at or behind min_off.  No device."""
import random
import struct

import pytest

import bai_model as bai
import bai_records as br
import bgzf_texts as bt
import csi_cases as cc
import csi_model as cm
import hostemu_deflate_lib as hd
import tbi_model as tm
import tbi_texts as tt


def all_texts():
    return {**tt.small_texts(), **tt.edge_texts(), "ladder": tt.ladder_text(), "big": tt.big_text()}


def fake_sizes(text):
    """block sizes that no compressor made: the model asks for the sizes alone"""
    return [60 + 13 * (k % 11) for k in range((len(text) + tm.SLICE - 1) // tm.SLICE)]


def test_the_specifications_numbers():
    assert [cm.pseudo_bin(d) for d in (1, 5, 6)] == [10, 37450, 299594]
    assert [cm.max_end(d) for d in (1, 2, 5, 6)] == [131072, 1 << 20, 1 << 29, 0xffffffff]
    assert [cm.level_first(l) for l in range(7)] == [0, 1, 9, 73, 585, 4681, 37449]
    assert cm.reg2bin(0, 0xffffffff, 6) == 0 and cm.reg2bin(0xfffffffe, 0xffffffff, 6) == 37449 + 262143 == 299592
    rnd = random.Random(3)
    for depth in (1, 2, 3, 4, 5, 6):
        lim = cm.max_end(depth)
        for _ in range(400):
            beg = rnd.randrange(lim)
            end = min(lim, beg + rnd.choice((1, 2, 100, 1 << 14, 1 << 17, 1 << 22, 1 << 28, lim)))
            b = cm.reg2bin(beg, end, depth)
            if depth == 5:
                assert b == tm.reg2bin(beg, end)
            l = cm.bin_level(b)
            assert cm.level_first(l) <= b < cm.level_first(l + 1) and l <= depth
            first, size = cm.bin_begin(b, depth), 1 << (14 + 3 * (depth - l))
            assert first <= beg and end <= first + size, "the record does not lie in its bin"
            assert l == depth or (beg >> (14 + 3 * (depth - l - 1))) != ((end - 1) >> (14 + 3 * (depth - l - 1))), "a smaller bin holds it too"
            for q in (cm.reg2bins(beg, end, depth), cm.reg2bins(beg, beg + 1, depth), cm.reg2bins(end - 1, end, depth)):
                assert b in q and len(set(q)) == len(q)
            if depth == 5:
                assert cm.reg2bins(beg, end, 5) == tm.reg2bins(beg, end)


def _same_as_linear(csi_ref, bins, lin, depth=5):
    assert csi_ref["bins"] == bins and csi_ref["order"] == sorted(bins)
    for b, loff in csi_ref["loff"].items():
        assert loff == lin[cm.bin_begin(b, depth) >> 14], b


@pytest.mark.parametrize("name", br.good())
def test_depth_5_is_the_bai_models_index(name):
    rs = br.sets()[name]
    raw = rs.file(bai.bgzf_blocks_of(rs.data))
    csi = cm.parse_csi(cm.bam_model(raw, 5))
    refs, _ = bai.parse_bai(bai.model(raw))
    assert csi["depth"] == 5 and csi["aux"] == b"" and len(csi["refs"]) == len(refs)
    for a, b in zip(csi["refs"], refs):
        assert a["pseudo"] == b["pseudo"]
        _same_as_linear(a, b["bins"], b["lin"])


@pytest.mark.parametrize("name", sorted(all_texts()))
def test_depth_5_is_the_tbi_models_index(name):
    text = all_texts()[name]
    sizes = fake_sizes(text)
    csi = cm.parse_csi(cm.bed_model(text, sizes, 777, 5))
    tbi = tm.parse_tbi(tm.model(text, sizes, 777))
    assert csi["names"] == tbi["names"] and csi["n_no_coor"] == 0
    assert csi["aux"] == tm.model(text, sizes, 777)[8:36 + sum(len(n) + 1 for n in tbi["names"])], "aux: the tabix header behind magic and n_ref"
    for a, b in zip(csi["refs"], tbi["refs"]):
        pseudo = b["bins"][tm.PSEUDO_BIN]
        assert a["pseudo"] == pseudo[0] + pseudo[1]
        bins = {k: v for k, v in b["bins"].items() if k != tm.PSEUDO_BIN}
        _same_as_linear(a, bins, b["ioff"])


@pytest.mark.parametrize("depth", [5, 6])
@pytest.mark.parametrize("name", br.good())
def test_bam_queries_against_brute_force(name, depth):
    rs = br.sets()[name]
    raw = rs.file(bai.bgzf_blocks_of(rs.data))
    found = cm.check_bam_queries(raw, cm.bam_model(raw, depth), cc.regions(rs, depth))
    assert found or name == "empty"


@pytest.mark.parametrize("name", sorted(cc.record_sets()))
def test_the_csi_record_sets(name):
    rs, depth = cc.record_sets()[name]
    raw = rs.file(bai.bgzf_blocks_of(rs.data))
    if rs.refused:
        with pytest.raises(bai.NotIndexable) as e:
            cm.bam_model(raw, depth)
        assert (e.value.cause, e.value.record) == rs.refused
        assert cm.parse_csi(cm.bam_model(raw, 6))["depth"] == 6
        return
    payload = cm.bam_model(raw, depth)
    assert cm.check_bam_queries(raw, payload, cc.regions(rs, depth)) > 0
    idx = cm.parse_csi(payload)
    if name == "wide_bins":
        assert 65536 + cc.X in idx["refs"][0]["bins"] and cc.X not in idx["refs"][0]["bins"]
        assert cc.X in idx["refs"][1]["bins"] and 65536 + cc.X not in idx["refs"][1]["bins"]
    if name == "depth1":
        assert sorted(idx["refs"][0]["bins"]) == [0, 1, 2, 8]


@pytest.mark.parametrize("name", [n for n in br.refused() if br.sets()[n].chain])   # (the model reads the file: the chain's own starts)
def test_what_the_bai_refuses(name):
    """beyond 2^29 is no cause at depth 6; every other cause stays"""
    rs = br.sets()[name]
    raw = rs.file(bai.bgzf_blocks_of(rs.data))
    if rs.refused[0] == bai.RANGE:
        with pytest.raises(bai.NotIndexable) as e:
            cm.bam_model(raw, 5)
        assert (e.value.cause, e.value.record) == rs.refused
        payload = cm.bam_model(raw, 6)
        f = bai.File(raw)
        regions = [(rid, p, p + 1) for _, _, rid, pos, end, _ in bai.records(f) for p in (pos, end - 1, end)] + [(0, 0, 0xffffffff), (0, 1 << 29, (1 << 29) + 1)]
        assert cm.check_bam_queries(raw, payload, regions) > 0
    else:
        with pytest.raises(bai.NotIndexable) as e:
            cm.bam_model(raw, 6)
        assert (e.value.cause, e.value.record) == rs.refused


_comp = {}


def compressed(text):
    if text not in _comp:
        _comp[text] = hd.deflate(text, 0)
    return _comp[text]


@pytest.mark.parametrize("depth", [5, 6])
@pytest.mark.parametrize("name", sorted(set(all_texts()) - {"big", "empty"}))
def test_bed_queries_against_a_scan(name, depth):
    text = all_texts()[name]
    comp = compressed(text)
    payload = cm.bed_model(text, bt.blocks(comp), 0, depth)
    queries = tt.ladder_queries() if name == "ladder" else tt.random_queries(text, 25)
    assert cm.check_bed_queries(comp + bt.EOF_BLOCK, payload, text, queries) > 0


@pytest.mark.parametrize("name", sorted(cc.texts()))
def test_the_csi_texts(name):
    text, depth, queries = cc.texts()[name]
    comp = compressed(text)
    payload = cm.bed_model(text, bt.blocks(comp), 0, depth)
    assert cm.check_bed_queries(comp + bt.EOF_BLOCK, payload, text, queries + tt.random_queries(text, 25)) > 0
    idx = cm.parse_csi(payload)
    if name == "wide_bins":
        assert 65536 + cc.X in idx["refs"][0]["bins"] and cc.X in idx["refs"][1]["bins"]


def test_texts_refused():
    for name, (text, depth, line) in cc.REFUSED_TEXTS.items():
        with pytest.raises(tm.NotIndexable) as e:
            cm.bed_model(text, fake_sizes(text), 0, depth)
        assert (e.value.cause, e.value.line) == ("beyond the limit", line), name
    text, cause, line, _ = tt.refused_texts()["end_beyond_2_29"]
    with pytest.raises(tm.NotIndexable) as e:
        cm.bed_model(text, fake_sizes(text), 0, 5)
    assert e.value.line == line
    assert cm.parse_csi(cm.bed_model(text, fake_sizes(text), 0, 6))["depth"] == 6
    for name in ("unsorted_start", "name_recurs", "two_columns", "non_digit", "no_final_newline"):
        text, cause, line, _ = tt.refused_texts()[name]
        with pytest.raises(tm.NotIndexable) as e:
            cm.bed_model(text, fake_sizes(text), 0, 6)
        assert (e.value.cause, e.value.line) == (cause, line)


def test_empty():
    assert cm.bed_model(b"", [], 0, 6) == struct.pack("<4s3i6iii", b"CSI\1", 14, 6, 28, 0x10000, 1, 2, 3, 35, 0, 0, 0) + struct.pack("<Q", 0)
    rs = br.sets()["empty"]
    assert cm.bam_model(rs.file(b""), 5) == struct.pack("<4s4i", b"CSI\1", 14, 5, 0, 3) + struct.pack("<3iQ", 0, 0, 0, 0)
