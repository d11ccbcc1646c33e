"""The device's BGZF compressor (chromap_amd/csrc/cm_deflate.h) compiled for the host and run by emulated lanes
(tests/hostemu/hostemu_deflate.cpp): every block must inflate to its slice with zlib, with gzip and with the project's own decoder
(cm_inflate.h), keep inside its output slot (guard bytes, checked by the harness), and be the same bytes whatever group runs it -- one
lane, 64 lanes in either order, 256 lanes.  The code shapes that can go wrong are reached on purpose and checked in the block's own header
(tests/bgzf_texts.py: read_dynamic_block): a literal code and a code-length code whose Huffman trees are deeper than 15 and 7, a coded block
without a match; and the code builder is run alone on counts far deeper than either limit.  On the golden SAM, BED and pairs texts the blocks together are at most what zlib's level 1
needs with fixed codes.

Ratios measured with this test (printed with -s): against zlib level 1 with fixed codes / with its default strategy, same slices --
SAM 0.738 / 0.957, barcoded BED 0.693 / 0.937, pairs 0.724 / 0.928 (compressed size over text: 0.214, 0.340, 0.309)."""
import ctypes as C
import zlib

import numpy as np
import pytest

import bgzf_texts as bt
import hostemu_deflate_lib as hd
import hostemu_lib as he


def _inflate_block(payload, n_out, crc):
    L = he.lib()
    guard = 64
    out = np.full(n_out + 2 * guard, 0x5A, np.uint8)
    cin = np.frombuffer(payload, np.uint8).copy()
    f = L.hostemu_inflate_block
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
    rc = f(cin.ctypes.data, len(payload), out.ctypes.data + guard, n_out, crc, 0)
    assert (out[:guard] == 0x5A).all() and (out[guard + n_out:] == 0x5A).all()
    return rc, bytes(out[guard:guard + n_out])


SHAPES = ("fibonacci", "de_bruijn", "code_length_code_deep")


def _check_shape(name, comp, text):
    """what the block's own header says: the code shape the text is there for was really reached"""
    at, size = bt.blocks(comp)[0]
    h = bt.read_dynamic_block(comp[at + 18:at + size - 8])
    assert h["out"] == text
    assert bt.kraft(h["ll"], 15) == 1 << 15 and bt.kraft(h["cl"], 7) == 1 << 7, "every code complete, none over-subscribed"
    if name == "fibonacci":  # Huffman's tree for the block's own counts is deeper than 15: the limit step ran
        assert bt.natural_depth(h["ll_cnt"]) > 15 and max(h["ll"]) == 15
    if name in ("fibonacci", "de_bruijn"):  # no match at all: one distance length, zero
        assert sum(h["ll_cnt"][257:]) == 0 and h["hdist"] == 1 and h["d"] == [0]
    if name == "code_length_code_deep":  # the same for the code-length code and 7
        assert bt.natural_depth(h["cl_cnt"]) > 7 and max(h["cl"]) == 7
        assert bt.kraft(h["d"], 15) == 1 << 15


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f


@pytest.mark.parametrize("maxbits", [15, 7])
@pytest.mark.parametrize("counts", ["fibonacci", "powers_of_two", "fibonacci_shuffled", "flat", "two", "one_heavy"])
def test_code_lengths_are_a_complete_code_within_the_limit(counts, maxbits):
    """cm_df_huff alone, on counts whose Huffman tree is many levels deeper than the limit: the lengths must be a complete prefix code
    (Kraft sum exactly 1 -- an over-subscribed code is one no inflater accepts), within the limit, never longer for a commoner symbol,
    and the same whatever group builds them"""
    n = 22 if maxbits == 15 else 19
    cnt = {"fibonacci": _fib(n), "powers_of_two": [1 << i for i in range(n)], "fibonacci_shuffled": list(np.random.default_rng(1).permutation(_fib(n))),
           "flat": [7] * n, "two": [0, 5, 0, 9] + [0] * (n - 4), "one_heavy": [1] * (n - 1) + [1 << 20]}[counts]
    cnt = [int(c) for c in cnt]
    lens = hd.huff_lengths(cnt, maxbits, 0)
    assert bt.kraft(lens, maxbits) == 1 << maxbits, lens
    assert all((l > 0) == (c > 0) for l, c in zip(lens, cnt)) and max(lens) <= maxbits
    if counts in ("fibonacci", "powers_of_two", "fibonacci_shuffled"):
        assert bt.natural_depth(cnt) > maxbits + 2 and max(lens) == maxbits
    for a in range(len(cnt)):
        for b in range(len(cnt)):
            assert not (cnt[a] > cnt[b] > 0 and lens[a] > lens[b])
    if bt.natural_depth(cnt) <= maxbits:  # nothing to limit: Huffman's own cost
        assert max(lens) == bt.natural_depth(cnt)
    for mode in (1, 2):
        assert hd.huff_lengths(cnt, maxbits, mode) == lens


def test_random_skewed_texts_always_inflate():
    """bytes drawn with probabilities 2^-L for random L: trees of every depth around the two limits"""
    rng = np.random.default_rng(11)
    for it in range(150):
        k = int(rng.integers(2, 200))
        groups = [(1, int(L)) for L in rng.integers(1, 16, k)]
        text = bt._skewed_text(it, int(rng.integers(300, 9000)), groups)
        bt.check_bgzf(hd.deflate(text, 0), text)


def test_shared_memory_leaves_room_for_two_workgroups_per_compute_unit():
    assert hd.lib().hostemu_deflate_shared_bytes() + 1024 <= 80 * 1024


@pytest.mark.parametrize("name", sorted(bt.small_texts()))
def test_small_texts_inflate_and_do_not_depend_on_the_lanes(name):
    text = bt.small_texts()[name]
    comp = hd.deflate(text, 0)
    kinds = bt.check_bgzf(comp, text, _inflate_block)
    assert hd.deflate(text, 0) == comp, "the same text twice"
    for mode in (1, 2):
        assert hd.deflate(text, mode) == comp, "64 lanes, order %d" % mode
    if len(text) <= bt.SLICE + 1000:
        assert hd.deflate(text, 3) == comp, "256 lanes"
    if name == "len0":
        assert comp == b""
    if name in ("random", "len1", "len2", "len3", "len4", "all_256_once"):
        assert set(kinds) == {0}, "what does not shrink is stored"
        assert len(comp) == len(text) + 31 * len(kinds)
    if name in ("fibonacci", "de_bruijn", "code_length_code_deep", "one_byte_repeated", "acgt_repeated", "period3", "one_literal_long", "match_at_32768", "match_at_32769",
                "no_match_low_entropy", "slice", "slice-1"):
        assert set(kinds) == {2}, "dynamic codes"
    if name == "last_slice_1_byte":
        assert kinds == [2, 0]
    if name in SHAPES:
        _check_shape(name, comp, text)
    if name == "one_byte_repeated":  # 0xff00 bytes as 253 matches of 258 and a rest: far below a byte per match
        assert len(comp) < 400
    if name == "match_at_32768":  # the second copy of the 100 bytes costs a match, not 100 literals of 8 bits and more
        assert len(comp) + 60 < len(hd.deflate(bt.small_texts()["match_at_32769"], 0))


@pytest.mark.parametrize("key", sorted(bt.GOLDEN_TEXTS))
def test_golden_texts_inflate_and_beat_fixed_codes(key):
    text = bt.golden_text(key)
    comp = hd.deflate(text, 0)
    # zlib and gzip inflate every block.  The project's own decoder runs as 64 emulated lanes, 0.12 s a block: on the SAM text's 240 blocks
    # that is half a minute, so it takes every eighth block and the last there (and the first three whole in the test below), every block
    # of the two other texts
    bt.check_bgzf(comp, text, _inflate_block, own_every=8 if key == "sam" else 1)
    assert hd.deflate(text, 0) == comp
    fixed = bt.zlib_level1_size(text, zlib.Z_FIXED)
    default = bt.zlib_level1_size(text, zlib.Z_DEFAULT_STRATEGY)
    print("%s: %d bytes of text -> %d (%.3f); zlib level 1 fixed codes %d (ours / it %.3f), default strategy %d (ours / it %.3f)" % (
        key, len(text), len(comp), len(comp) / len(text), fixed, len(comp) / fixed, default, len(comp) / default))
    assert len(comp) <= fixed


def test_golden_sam_head_through_the_projects_decoder_and_every_group():
    text = bt.golden_text("sam")[:3 * bt.SLICE + 11]
    comp = hd.deflate(text, 0)
    bt.check_bgzf(comp, text, _inflate_block)
    for mode in (1, 2):
        assert hd.deflate(text, mode) == comp
