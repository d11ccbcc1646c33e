"""The sequential model of the tabix index (tests/tbi_model.py) against the format itself: its payload parses, has the structure the
specification asks for, and region queries through it -- with a reader written from the specification -- return what a scan of the
text returns.  The block sizes are those of the host build of the device's compressor.  No device."""
import struct

import pytest

import bgzf_texts as bt
import datasets
import hostemu_deflate_lib as hd
import tbi_model as tm
import tbi_texts as tt

_comp = {}


def compressed(text):
    if text not in _comp:
        _comp[text] = hd.deflate(text, 0)
    return _comp[text]


def indexed(text, base=0):
    comp = compressed(text)
    return comp, tm.model(text, bt.blocks(comp), base)


def test_reg2bin_and_reg2bins_agree_on_every_boundary():
    for B in tt.LADDER + [1 << 29]:
        for beg, end in ((B - 1, B), (B - 1, B + 1), (B, B + 1), (B - 150, B), (B - 150, B + 150), (B - 2, B - 1)):
            if end > 1 << 29:
                continue
            b = tm.reg2bin(beg, end)
            assert b in tm.reg2bins(beg, end) and b in tm.reg2bins(beg, beg + 1) and b in tm.reg2bins(end - 1, end)
    assert tm.reg2bin(0, 1 << 29) == 0 and tm.reg2bin(0, 1) == 4681 and tm.reg2bin((1 << 29) - 1, 1 << 29) == 37448
    assert tm.reg2bin((1 << 14) - 1, 1 << 14) == 4681 and tm.reg2bin((1 << 14) - 1, (1 << 14) + 1) == 585


def test_golden_barcoded_bed_has_the_figures_of_the_prototype():
    text = bt.golden_text("bed_bc")
    comp, payload = indexed(text)
    assert text.count(b"\n") == 17723 and len(bt.blocks(comp)) == 11
    assert tm.model.last_stats == {"raw": 336, "merged": 157} and len(payload) == 4920
    tt.check_queries(comp + bt.EOF_BLOCK, payload, text, tt.random_queries(text, 300))


@pytest.mark.parametrize("case", ["s1_atac", "b1_atac_bc"])
def test_golden_bed_texts(case):
    text = datasets.case_golden_bed(case)
    comp, payload = indexed(text)
    idx = tm.parse_tbi(payload)
    names = []
    for ln in text.splitlines():
        n = ln.split(b"\t")[0]
        if not names or names[-1] != n:
            names.append(n)
    assert idx["names"] == names and idx["n_no_coor"] == 0
    lines = 0
    for r in idx["refs"]:
        (v0, v1), (n, zero) = r["bins"][tm.PSEUDO_BIN]
        assert v0 < v1 and zero == 0
        lines += n
        assert r["ioff"] == sorted(r["ioff"]) and len(r["ioff"]) >= 1
        for b, chunks in r["bins"].items():
            assert b == tm.PSEUDO_BIN or all(c[0] < c[1] for c in chunks) and chunks == sorted(chunks)
    assert lines == text.count(b"\n")
    tt.check_queries(comp + bt.EOF_BLOCK, payload, text, tt.random_queries(text, 100))


def test_empty_text():
    payload = tm.model(b"", [], 0)
    assert payload == struct.pack("<4s8iQ", b"TBI\1", 0, 0x10000, 1, 2, 3, 35, 0, 0, 0)
    assert tm.parse_tbi(payload) == {"names": [], "refs": [], "n_no_coor": 0}


def test_bin_ladder():
    text = tt.ladder_text()
    comp, payload = indexed(text, base=0)
    idx = tm.parse_tbi(payload)
    assert idx["names"] == list(tt.LADDER_NAMES)
    last = {}
    for ln in text.splitlines():
        c = ln.split(b"\t")
        last[c[0]] = max(last.get(c[0], 0), (max(int(c[2]), int(c[1]) + 1) - 1 >> 14) + 1)
    assert [len(r["ioff"]) for r in idx["refs"]] == [last[n] for n in tt.LADDER_NAMES]
    assert [len(r["ioff"]) for r in idx["refs"]][:2] == [32768, 32768] and len(idx["refs"][2]["ioff"]) < 32768
    for r in idx["refs"]:
        assert 0 in r["bins"] and 4681 in r["bins"] and 1 in r["bins"]   # across 2^26, across 2^23 only, within a leaf
        io = r["ioff"]
        assert io == sorted(io)
        assert io[0] < io[1] == io[2] == io[3] == io[4]                   # (0, 1), then (0, 70000): five windows, the last four its own
        assert len(set(io[200:1000])) < 100                                # back-fill: runs of equal offsets above 3 Mb
    tt.check_queries(comp + bt.EOF_BLOCK, payload, text, tt.ladder_queries())


@pytest.mark.parametrize("name", sorted(tt.small_texts()) + sorted(tt.edge_texts()))
def test_small_and_edge_texts(name):
    text = {**tt.small_texts(), **tt.edge_texts()}[name]
    comp, payload = indexed(text, base=12345)
    if text:
        raw = b"\0" * 12345 + comp + bt.EOF_BLOCK    # (nothing is read below the base)
        tt.check_queries(raw, payload, text, tt.random_queries(text, 25))


def test_the_model_refuses_paired_tagalign_text():
    text = datasets.case_golden_bed("s2_tagalign_q0")
    with pytest.raises(tm.NotIndexable) as e:
        tm.model(text, [28] * ((len(text) + tm.SLICE - 1) // tm.SLICE), 0)
    assert e.value.cause == "not sorted"


@pytest.mark.parametrize("name", sorted(tt.refused_texts()))
def test_the_model_refuses(name):
    text, cause, line, _ = tt.refused_texts()[name]
    with pytest.raises(tm.NotIndexable) as e:
        tm.model(text, [28] * ((len(text) + tm.SLICE - 1) // tm.SLICE), 0)
    assert (e.value.cause, e.value.line) == (cause, line)
