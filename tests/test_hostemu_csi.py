"""The device's CSI indexer built for the host (tests/hostemu/hostemu_csi.cpp: the stage functions of chromap_amd/csrc/cm_tabix.h and
cm_bai.h with the depth in their arrays, the loffset function, the CSI serialiser) gives the plain-Python model's bytes
(tests/csi_model.py) at depths 1, 2, 5 and 6 on every record set and text -- record by record, in waves of 64 in ascending and in
descending order, in blocks of 256 -- and refuses what the model refuses, with the same cause at the same record or line.  A
stand-alone build of the same functions runs a few of the sets under AddressSanitizer and UndefinedBehaviorSanitizer.  No device."""
import subprocess

import pytest

import bai_model as bai
import bai_records as br
import bgzf_texts as bt
import csi_cases as cc
import csi_model as cm
import hostemu_csi_lib as hc
import tbi_model as tm
import tbi_texts as tt

MODES = (0, 1, 2, 3)
TBX_CAUSES = {"malformed": 1, "name recurs": 2, "not sorted": 3, "beyond the limit": 4}


def _blocks(rs):
    blocks = bai.bgzf_blocks_of(rs.data)
    return blocks, [s for _, s in bt.blocks(blocks)]


def _bam_same_as_model(rs, depth):
    blocks, sizes = _blocks(rs)
    base = len(rs.header_blocks())
    try:
        want = cm.bam_model(rs.file(blocks), depth)
    except bai.NotIndexable as m:
        for mode in MODES:
            with pytest.raises(hc.Refused) as e:
                hc.index_bam(rs.data, rs.starts, rs.n_ref, sizes, depth, base, mode)
            assert (e.value.cause, e.value.item) == (m.cause, m.record), "mode %d" % mode
        return None
    for mode in MODES:
        assert hc.index_bam(rs.data, rs.starts, rs.n_ref, sizes, depth, base, mode) == want, "mode %d" % mode
    return want


def test_reg2bin_and_the_bins_first_window():
    import random
    rnd = random.Random(17)
    L = hc.lib()
    for depth in range(1, 7):
        lim = cm.max_end(depth)
        pairs = [(0, 1), (0, lim), (lim - 1, lim), (16383, 16385)] + [(b, min(lim, b + w)) for b, w in ((rnd.randrange(lim), rnd.choice((1, 70, 20000, 1 << 21, lim))) for _ in range(300))]
        for beg, end in pairs:
            b = L.hostemu_csi_reg2bin(beg, end, depth)
            assert b == cm.reg2bin(beg, end, depth), (beg, end, depth)
            assert L.hostemu_csi_bin_window(b, depth) == cm.bin_begin(b, depth) >> 14, (b, depth)


@pytest.mark.parametrize("depth", cc.DEPTHS)
@pytest.mark.parametrize("name", br.good())
def test_record_sets(name, depth):
    """(at depths 1 and 2 most sets end beyond the limit: the refusal is the model's)"""
    got = _bam_same_as_model(br.sets()[name], depth)
    assert got is not None or depth < 5


@pytest.mark.parametrize("name", sorted(cc.record_sets()))
def test_csi_record_sets(name):
    rs, depth = cc.record_sets()[name]
    assert (_bam_same_as_model(rs, depth) is None) == (rs.refused is not None)


@pytest.mark.parametrize("name", br.refused())
def test_what_the_bai_refuses(name):
    rs = br.sets()[name]
    _, sizes = _blocks(rs)
    for depth in (5, 6):
        if rs.refused[0] == bai.RANGE and depth == 6:
            assert _bam_same_as_model(rs, 6) is not None
            continue
        for mode in MODES:
            with pytest.raises(hc.Refused) as e:
                hc.index_bam(rs.data, rs.starts, rs.n_ref, sizes, depth, 0, mode)
            assert (e.value.cause, e.value.item) == rs.refused, "mode %d" % mode


def _fake_sizes(text):
    return [60 + 13 * (k % 11) for k in range((len(text) + tm.SLICE - 1) // tm.SLICE)]


def _bed_same_as_model(text, depth, base=4711):
    sizes = _fake_sizes(text)
    try:
        want = cm.bed_model(text, sizes, base, depth)
    except tm.NotIndexable as m:
        for mode in MODES:
            with pytest.raises(hc.Refused) as e:
                hc.index_bed(text, sizes, depth, base, mode)
            assert (e.value.cause, e.value.item) == (TBX_CAUSES[m.cause], m.line), "mode %d" % mode
        return None
    for mode in MODES:
        assert hc.index_bed(text, sizes, depth, base, mode) == want, "mode %d" % mode
    return want


@pytest.mark.parametrize("depth", cc.DEPTHS)
@pytest.mark.parametrize("name", sorted({**tt.small_texts(), **tt.edge_texts()}) + ["ladder"])
def test_texts(name, depth):
    text = {**tt.small_texts(), **tt.edge_texts(), "ladder": tt.ladder_text()}[name]
    got = _bed_same_as_model(text, depth)
    assert got is not None or depth < 5


@pytest.mark.parametrize("name", sorted(cc.texts()))
def test_csi_texts(name):
    text, depth, _ = cc.texts()[name]
    assert _bed_same_as_model(text, depth) is not None


def test_texts_refused():
    for name, (text, depth, line) in cc.REFUSED_TEXTS.items():
        assert _bed_same_as_model(text, depth) is None, name
    for name, (text, cause, line, _) in tt.refused_texts().items():
        if name == "no_final_newline":
            continue   # (found before the lines are looked at: -3, as tests/test_hostemu_tabix.py has it)
        assert (_bed_same_as_model(text, 6) is None) == (name != "end_beyond_2_29"), name
        assert _bed_same_as_model(text, 5) is None, name


def test_base_moves_every_offset_and_no_pseudo_bin():
    rs = br.sets()["block_seams"]
    _, sizes = _blocks(rs)
    a = cm.parse_csi(hc.index_bam(rs.data, rs.starts, rs.n_ref, sizes, 6, 0))["refs"][0]
    b = cm.parse_csi(hc.index_bam(rs.data, rs.starts, rs.n_ref, sizes, 6, 4711))["refs"][0]
    shift = 4711 << 16
    assert b["bins"] == {k: [(x + shift, y + shift) for x, y in ch] for k, ch in a["bins"].items()}
    assert b["loff"] == {k: v + shift for k, v in a["loff"].items()} and a["loff"]
    assert b["pseudo"][:2] == (a["pseudo"][0] + shift, a["pseudo"][1] + shift) and b["pseudo"][2:] == a["pseudo"][2:]


def test_sanitizer_program(tmp_path):
    paths = []
    for name, (rs, depth) in [("block_seams", (br.sets()["block_seams"], 6)), ("cigars", (br.sets()["cigars"], 2))] + \
            [(n, cc.record_sets()[n]) for n in ("depth1", "wide_bins", "pos_2_31")]:
        blocks, sizes = _blocks(rs)
        base = len(rs.header_blocks())
        paths.append(str(tmp_path / (name + ".bam.case")))
        hc.write_case(paths[-1], 0, rs.data, rs.starts, rs.n_ref, sizes, base, depth, cm.bam_model(rs.file(blocks), depth))
    texts = {n: (t, d) for n, (t, d, _) in cc.texts().items()}
    texts["line_straddles_slice"] = (tt.edge_texts()["line_straddles_slice"], 5)
    for name, (text, depth) in sorted(texts.items()):
        sizes = _fake_sizes(text)
        paths.append(str(tmp_path / (name + ".bed.case")))
        hc.write_case(paths[-1], 1, text, [0], 0, sizes, 99, depth, cm.bed_model(text, sizes, 99, depth))
    r = subprocess.run([hc.sanitizer_program()] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-3000:]
    assert r.stdout.count(b"four modes equal") == len(paths)
