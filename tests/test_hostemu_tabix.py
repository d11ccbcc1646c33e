"""The device's tabix indexer built for the host (tests/hostemu/hostemu_tabix.cpp: the stage functions and the serialiser of
chromap_amd/csrc/cm_tabix.h) gives the sequential model's bytes (tests/tbi_model.py) -- with one lane, with 64 emulated lanes in
ascending and in descending order, with the device's 256 -- and refuses what the model refuses, at the same line.  No device."""
import pytest

import bgzf_texts as bt
import datasets
import hostemu_deflate_lib as hd
import hostemu_tabix_lib as ht
import tbi_model as tm
import tbi_texts as tt

_sizes = {}


def sizes_of(text):
    if text not in _sizes:
        _sizes[text] = [s for _, s in bt.blocks(hd.deflate(text, 0))]
    return _sizes[text]


def _same(text, base, modes):
    sizes = sizes_of(text)
    want = tm.model(text, sizes, base)
    for mode in modes:
        assert ht.index(text, sizes, base, mode) == want, "mode %d" % mode


def test_reg2bin():
    for B in tt.LADDER + [1 << 29]:
        for beg, end in ((B - 1, B), (B - 1, B + 1), (B, B + 1), (B - 150, B), (B - 150, B + 150), (B - 2, B - 1), (0, B), (B - 1, B)):
            if end <= 1 << 29:
                assert ht.reg2bin(beg, end) == tm.reg2bin(beg, end)


@pytest.mark.parametrize("name", sorted(tt.small_texts()) + sorted(tt.edge_texts()))
def test_small_and_edge_texts(name):
    _same({**tt.small_texts(), **tt.edge_texts()}[name], 4711, (0, 1, 2, 3))


def test_bin_ladder():
    _same(tt.ladder_text(), 0, (0, 1, 2))


@pytest.mark.parametrize("case", ["s1_atac", "b1_atac_bc"])
def test_golden_bed_texts(case):
    _same(datasets.case_golden_bed(case), 47, (0, 1, 2))


def test_block_offsets_enter_every_virtual_offset():
    """other block sizes and another base: other bytes, and the model's"""
    text = tt.edge_texts()["name_runs_cross_slices"]
    n = (len(text) + tm.SLICE - 1) // tm.SLICE
    a = ht.index(text, [100 + 7 * i for i in range(n)], 0, 0)
    assert a == tm.model(text, [100 + 7 * i for i in range(n)], 0)
    assert a != ht.index(text, [101 + 7 * i for i in range(n)], 0, 0) and a != ht.index(text, [100 + 7 * i for i in range(n)], 1, 0)


@pytest.mark.parametrize("name", sorted(tt.refused_texts()))
def test_refusals(name):
    text, cause, line, _ = tt.refused_texts()[name]
    sizes = [28] * ((len(text) + tm.SLICE - 1) // tm.SLICE)
    for mode in (0, 1, 2):
        if cause == "no final newline":
            with pytest.raises(ValueError, match="no final newline"):
                ht.index(text, sizes, 0, mode)
        else:
            with pytest.raises(ht.Refused) as e:
                ht.index(text, sizes, 0, mode)
            assert (ht.CAUSES[e.value.cause], e.value.line) == (cause, line)


def test_paired_tagalign_text_is_refused():
    text = datasets.case_golden_bed("s2_tagalign_q0")
    with pytest.raises(ht.Refused) as e:
        ht.index(text, [28] * ((len(text) + tm.SLICE - 1) // tm.SLICE), 0, 1)
    with pytest.raises(tm.NotIndexable) as m:
        tm.model(text, [28] * ((len(text) + tm.SLICE - 1) // tm.SLICE), 0)
    assert (ht.CAUSES[e.value.cause], e.value.line) == (m.value.cause, m.value.line)
