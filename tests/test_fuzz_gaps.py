"""Keeps the gap-rich fuzz configurations (tests/fuzz_data.py, ids 7-10) from becoming vacuous: the oracle's trace and the
generator's truth, per configuration.  The floors are conditions on the data and the oracle alone."""
import ctypes as C
import hashlib

import pytest

import fuzz_data
import oracle_lib as ol

# (chromosomes, read 1, read 2) of configurations 1-6 as they were before the generator learnt gaps: its options are off by
# default and draw nothing then
OLD_DATA_MD5 = {
    1: "cdccfb2b99ca5a8fa7e8f9b7d1a2b5fe", 2: "d82c40dc58c1a7cc5cf2115da2435b8b", 3: "ad47e426bab1625effd79b7fe7aef54b",
    4: "ce6b93ee3fb3f499383566d7c8bf633d", 5: "53b081947dabfba230a8634885950a97", 6: "1b2622a906a539ff20a8a8c08a44f270",
}


@pytest.mark.parametrize("cfg", fuzz_data.CONFIGS[:6], ids=[str(c[0]) for c in fuzz_data.CONFIGS[:6]])
def test_earlier_configurations_are_untouched(cfg):
    seed, _, _, gen = cfg
    ch, r1, r2 = fuzz_data.make_case(seed, **gen)
    got = hashlib.md5(b"".join(c.tobytes() for c in ch) + b"|".join(r1) + b"#" + b"|".join(r2)).hexdigest()
    assert got == OLD_DATA_MD5[seed]


def test_gap_configurations_are_appended():
    assert [c[0] for c in fuzz_data.CONFIGS] == list(range(1, 11)) and fuzz_data.GAP_CONFIGS == fuzz_data.CONFIGS[6:]


def _comp(b):
    return b.translate(bytes.maketrans(b"ACGTN", b"TGCAN"))[::-1]


@pytest.mark.parametrize("cfg", fuzz_data.GAP_CONFIGS, ids=[str(c[0]) for c in fuzz_data.GAP_CONFIGS])
def test_gap_rich_data_reaches_the_gapped_paths(cfg, tmp_path):
    seed, preset, kw, gen = cfg
    fa, b1, o1, b2, o2 = fuzz_data.write_case(str(tmp_path), seed, **gen)
    ch, r1, r2, truth = fuzz_data.make_case_with_truth(seed, **gen)
    o = ol.Oracle(None, fa, ol.params(preset, **kw))
    e, L = o.p.error_threshold, gen["L"]
    assert e == gen["gap_e"]
    _, _, _, tr = o.map_pairs(b1, o1, b2, o2, trace=True)
    split = bool(o.p.split_alignment)
    pairs = at_e = long_gap = end_gap = edge = 0
    for i, t in enumerate(truth):
        c = ch[t["chr"]]
        any_gapped = False
        for nd, me, script, read, (lo, hi, strand) in ((tr[i].n_draft1, tr[i].min_err1, t["scripts"][0], r1[i], t["where"][0]),
                                                       (tr[i].n_draft2, tr[i].min_err2, t["scripts"][1], r2[i], t["where"][1])):
            mapped = nd >= 1 and me <= e
            if not mapped:
                continue
            if split:
                # split alignment keeps the negated aligned length in min_err; the edit count of such a read is taken from the
                # oracle's band at the place and on the strand the generator cut this read from
                me = e + 1
                if lo >= e and lo + len(read) + e <= len(c):
                    ep = C.c_int(-1)
                    me = o.L.ora_banded_align(e, c[lo - e:lo + len(read) + e].tobytes(), _comp(read) if strand else read, len(read), C.byref(ep))
            at_e += me == e
            gaps = [x for x in script if x[0] in "id"]
            if gaps:
                any_gapped = True
                long_gap += any(x[2] >= 2 for x in gaps)
                end_gap += any(x[1] < 3 or x[1] >= len(read) - 3 for x in gaps)
                edge += lo < L + e or hi > len(c) - (L + e)  # this read's own bases, not its fragment's
        pairs += any_gapped
    o.close()
    print("config %d: gapped mapped pairs %d of %d, reads at e %d, gap runs >= 2: %d, gaps at an end: %d, at a chromosome end: %d"
          % (seed, pairs, len(truth), at_e, long_gap, end_gap, edge))
    assert pairs * 10 >= 3 * len(truth)
    assert at_e >= 50
    if e >= 2:  # with e = 1 a gap run of 2 bases cannot be aligned: not applicable
        assert long_gap >= 50
    assert end_gap >= 50
    assert edge >= 20
