"""Synthetic BAM alignment records for the BAM index's tests (tests/test_bai_model.py on the model, tests/test_hostemu_bai.py on the
host emulation, tests/test_gpu_bai.py on the device): minimal valid records -- a name, a CIGAR, four bases -- in named sets, each the
smallest shape at which an index builder can go wrong.  Test infrastructure only."""
import struct

import bai_model as bai
import bam_model as bm
import bgzf_texts as bt

SLICE = bt.SLICE
BLOCK = 256   # lanes of the device's per-record kernels (chromap_amd/csrc/cm_tabix.hip: TX_LANES)
PLAIN = 48    # bytes of record(...) with a one-letter name and one CIGAR operation


def record(tid, pos, cigar=((5, "M"),), flag=0, name=b"r"):
    """one record: l_seq 4 (ACGT, quality 30), no mate, no tags; bin as the specification computes it"""
    ref_len = sum(n for n, op in cigar if op in "MDN=X")
    words = [n << 4 | bm.CIGAR_OPS.index(op) for n, op in cigar]
    body = struct.pack("<iiBBHHHIiii", tid, pos, len(name) + 1, 30, bm.reg2bin(max(pos, 0), max(pos, 0) + max(1, ref_len)) & 0xffff, len(words), flag, 4, -1, -1, 0)
    body += name + b"\0" + struct.pack("<%dI" % len(words), *words) + b"\x12\x48" + b"\x1e" * 4
    return struct.pack("<I", len(body)) + body


def sized(tid, pos, size, **kw):
    """a record of exactly `size` bytes (PLAIN .. PLAIN + 253): the name makes up the difference"""
    assert PLAIN <= size <= PLAIN + 253
    r = record(tid, pos, name=b"r" * (1 + size - PLAIN), **kw)
    assert len(r) == size
    return r


class RecordSet:
    def __init__(self, name, n_ref, recs, refused=None, starts=None, cut=0, seams=()):
        self.name, self.n_ref, self.refused = name, n_ref, refused
        self.data = b"".join(recs)
        self.starts = [0]
        for r in recs:
            self.starts.append(self.starts[-1] + len(r))
        if cut:   # the last record runs past the end
            self.data = self.data[:-cut]
            self.starts[-1] = len(self.data)
        self.chain = starts is None   # the starts are those of the chain of records: a reader of the file finds the same
        if starts is not None:
            self.starts = starts(self.starts)
        self.seams = list(seams)   # (reference, position): where queries are asked, each +- 1

    def header_blocks(self):
        return bai.bgzf_blocks_of(bai.bam_header(self.n_ref))

    def file(self, blocks):
        """the BAM file whose records are the BGZF blocks `blocks`"""
        return self.header_blocks() + blocks + bt.EOF_BLOCK


def _up_to(tid, pos, at, target):
    """records at (tid, pos) from offset `at` on, the last of which ends exactly at `target`"""
    out = []
    while target - at > PLAIN + 253:   # (what is left then is more than 253 bytes: room for the sized one)
        out.append(record(tid, pos))
        at += PLAIN
    out.append(sized(tid, pos, target - at))
    return out


def _ladder():
    recs, seams = [], []
    for shift in (14, 17, 20, 23, 26):
        s = 1 << shift
        recs += [record(0, s - 10, ((10, "M"),)), record(0, s - 5, ((10, "M"),)), record(0, s, ((10, "M"),))]
        seams += [(0, s - 10), (0, s), (0, s + 5), (0, s + 10)]
    recs.append(record(0, (1 << 29) - 10, ((10, "M"),)))   # end == 2^29: accepted
    seams.append((0, (1 << 29) - 10))
    return recs, seams


def _seam_sets():
    out = []
    # a record ends exactly on the block seam and the next one starts on it; then one that lies across the second seam
    recs = _up_to(0, 100, 0, SLICE)
    recs.append(record(0, 200))                                       # starts exactly on the seam
    recs += _up_to(0, 300, SLICE + PLAIN, 2 * SLICE - 20)             # ends 20 bytes before the second seam
    recs.append(record(0, 20000, ((10, "M"),)))                       # across it, in another bin and window
    recs.append(record(0, 40000))
    out.append(RecordSet("block_seams", 1, recs, seams=[(0, 100), (0, 200), (0, 300), (0, 20000), (0, 40000)]))
    # ... the last record of all ends exactly on a seam: the file's end is the block behind it
    out.append(RecordSet("ends_on_a_seam", 1, _up_to(0, 7, 0, SLICE), seams=[(0, 7)]))
    return out


def _interleaved(far):
    a = ((20000, "M"),)   # two windows: bin 585
    between = [record(0, 200 + k) for k in range(1400 if far else 3)]   # bin 4681; 1400 x 48 bytes > 0xff00
    recs = [record(0, 100, a)] + between + [record(0, 2000, a), record(0, 2100)]
    return RecordSet("bins_a_b_a_far" if far else "bins_a_b_a_near", 1, recs, seams=[(0, 100), (0, 200), (0, 2000), (0, 16384), (0, 20100)])


_sets = None


def sets():
    """name -> RecordSet, the refused ones included"""
    global _sets
    if _sets is not None:
        return _sets
    s = []
    s.append(RecordSet("empty", 3, []))
    s.append(RecordSet("one_record", 1, [record(0, 12345)], seams=[(0, 12345), (0, 12350)]))
    s.append(RecordSet("one_position_1000", 1, [record(0, 777)] * 1000, seams=[(0, 777), (0, 782)]))
    lad, seams = _ladder()
    s.append(RecordSet("bin_ladder", 1, lad, seams=seams))
    s.append(RecordSet("cigars", 2, [record(0, 16380, ((10, "S"), (5, "M"))),                      # end = pos + 5: window 1 is not touched
                                     record(0, 16380, ((3, "M"), (2, "D"), (1, "M"), (16000, "N"), (4, "M"))),   # D and N count
                                     record(0, 16383, ((9, "I"),)),                                   # end = pos + 1
                                     record(0, 16383, ()),                                             # no CIGAR: end = pos + 1
                                     record(1, 16383, ((1, "="), (1, "X"), (5, "H"), (2, "P")))],      # = and X count, H and P do not
                       seams=[(0, 16380), (0, 16384), (0, 16385), (0, 16390), (0, 32390), (1, 16384), (1, 16385)]))
    s.append(RecordSet("empty_references", 6, [record(1, 5), record(1, 70000), record(2, 0), record(4, 99), record(4, 99)],
                       seams=[(0, 5), (1, 5), (1, 70000), (2, 0), (3, 99), (4, 99), (5, 99)]))
    s.append(RecordSet("unmapped_with_position", 2, [record(0, 10), record(0, 20, flag=4), record(1, 5, flag=4 | 1), record(1, 6)], seams=[(0, 20), (1, 5)]))
    s.append(_interleaved(False))
    s.append(_interleaved(True))
    s += _seam_sets()
    for n in (3 * BLOCK - 1, 3 * BLOCK, 3 * BLOCK + 1):   # the per-record kernels' last block: one lane short, full, one lane over
        s.append(RecordSet("records_%d" % n, 3, [record(i * 3 // n, i * 50, ((60, "M"),)) for i in range(n)],
                           seams=[(0, 16384), (1, 16384), (2, 32768), (2, 50 * (n - 1))]))
    # ---- refused: (cause, 1-based record)
    ok = [record(0, 100), record(0, 200)]
    s.append(RecordSet("refused_pos_decreasing", 1, ok + [record(0, 150), record(0, 300)], refused=(bai.UNSORTED, 3)))
    s.append(RecordSet("refused_refid_decreasing", 2, [record(1, 5), record(0, 500)], refused=(bai.UNSORTED, 2)))
    s.append(RecordSet("refused_refid_n_ref", 2, ok + [record(1, 5), record(2, 5)], refused=(bai.NOREF, 4)))
    s.append(RecordSet("refused_refid_minus_1", 2, [record(-1, 0)] + ok, refused=(bai.NOREF, 1)))
    s.append(RecordSet("refused_end_beyond", 1, ok + [record(0, (1 << 29) - 9, ((10, "M"),))], refused=(bai.RANGE, 3)))
    s.append(RecordSet("refused_start_off_chain", 1, ok + [record(0, 300), record(0, 400)], refused=(bai.MALFORMED, 2),
                       starts=lambda st: st[:2] + [st[2] + 4] + st[3:]))
    s.append(RecordSet("refused_last_past_end", 1, ok + [record(0, 300)], refused=(bai.MALFORMED, 3), cut=3))
    _sets = {x.name: x for x in s}
    assert len(_sets) == len(s)
    return _sets


def good():
    return [n for n, x in sets().items() if x.refused is None]


def refused():
    return [n for n, x in sets().items() if x.refused is not None]


def regions(rs, seed=5):
    """(reference, beg, end) to query: every seam +- 1 as a one-base and a 100-base region, and 25 seeded random regions"""
    import random
    rnd = random.Random("%s/%d" % (rs.name, seed))
    out = []
    for tid, p in rs.seams:
        for q in (p - 1, p, p + 1):
            if q >= 0:
                out += [(tid, q, q + 1), (tid, q, q + 100), (tid, max(0, q - 100), q), (tid, max(0, q - 1), q + 1)]
    tops = [p for _, p in rs.seams] or [1000]
    for _ in range(25):
        tid = rnd.randrange(max(1, rs.n_ref))
        top = rnd.choice(tops) + 40000
        beg = rnd.randrange(top)
        out.append((tid, beg, min(1 << 29, beg + rnd.choice((1, 10, 1000, 20000, 1 << 20, 1 << 29)))))
    return [(t, b, e) for t, b, e in out if e > b and t < rs.n_ref]
