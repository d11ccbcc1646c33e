"""The device's BAM indexer built for the host (tests/hostemu/hostemu_bai.cpp: the per-record functions and the serialiser of
chromap_amd/csrc/cm_bai.h, the chunk functions of cm_tabix.h) gives the plain-Python model's bytes (tests/bai_model.py) on every
synthetic record set (tests/bai_records.py) -- record by record, in waves of 64 in ascending and in descending order, in blocks of
256 -- and refuses what is to be refused, with the same cause at the same record.  A stand-alone build of the same function runs
two of the block-seam sets under AddressSanitizer and UndefinedBehaviorSanitizer.  No device."""
import subprocess

import pytest

import bai_model as bai
import bai_records as br
import bgzf_texts as bt
import hostemu_bai_lib as hb


def _blocks(rs):
    blocks = bai.bgzf_blocks_of(rs.data)
    return blocks, [s for _, s in bt.blocks(blocks)]


@pytest.mark.parametrize("name", br.good())
def test_payload_is_the_models(name):
    rs = br.sets()[name]
    blocks, sizes = _blocks(rs)
    base = len(rs.header_blocks())
    want = bai.model(rs.file(blocks))
    for mode in (0, 1, 2, 3):
        assert hb.index(rs.data, rs.starts, rs.n_ref, sizes, base, mode) == want, "mode %d" % mode


def test_block_offsets_and_base_enter_every_virtual_offset():
    rs = br.sets()["block_seams"]
    _, sizes = _blocks(rs)
    a = hb.index(rs.data, rs.starts, rs.n_ref, sizes, 0)
    assert a != hb.index(rs.data, rs.starts, rs.n_ref, sizes, 1) and a != hb.index(rs.data, rs.starts, rs.n_ref, [sizes[0] + 1] + sizes[1:], 0)
    # the same offsets: a base that is a header of 4711 bytes shifts every chunk by 4711 << 16
    refs_a, _ = bai.parse_bai(a)
    refs_b, _ = bai.parse_bai(hb.index(rs.data, rs.starts, rs.n_ref, sizes, 4711))
    shift = 4711 << 16
    assert refs_b[0]["lin"] == [v + shift for v in refs_a[0]["lin"]]
    assert refs_b[0]["bins"] == {b: [(x + shift, y + shift) for x, y in ch] for b, ch in refs_a[0]["bins"].items()}


@pytest.mark.parametrize("name", br.refused())
def test_refusals(name):
    rs = br.sets()[name]
    _, sizes = _blocks(rs)
    for mode in (0, 1, 2, 3):
        with pytest.raises(hb.Refused) as e:
            hb.index(rs.data, rs.starts, rs.n_ref, sizes, 0, mode)
        assert (e.value.cause, e.value.record) == rs.refused, "mode %d" % mode


def test_the_first_offender_wins():
    """an unsorted record ahead of one that ends beyond 2^29: the earlier record is named, whatever order the lanes come in"""
    recs = [br.record(0, 100), br.record(0, 50), br.record(0, (1 << 29) - 1, ((5, "M"),)), br.record(3, 0)]
    rs = br.RecordSet("two_offenders", 1, recs)
    _, sizes = _blocks(rs)
    for mode in (0, 1, 2, 3):
        with pytest.raises(hb.Refused) as e:
            hb.index(rs.data, rs.starts, rs.n_ref, sizes, 0, mode)
        assert (e.value.cause, e.value.record) == (bai.UNSORTED, 2)


def test_sanitizer_program(tmp_path):
    paths = []
    for name in ("block_seams", "ends_on_a_seam", "cigars"):
        rs = br.sets()[name]
        blocks, sizes = _blocks(rs)
        base = len(rs.header_blocks())
        paths.append(str(tmp_path / (name + ".case")))
        hb.write_case(paths[-1], rs.data, rs.starts, rs.n_ref, sizes, base, bai.model(rs.file(blocks)))
    r = subprocess.run([hb.sanitizer_program()] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-3000:]
    assert r.stdout.count(b"four modes equal") == len(paths)
