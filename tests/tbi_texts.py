"""The texts the tabix indexer is tested on -- by the sequential model (tests/test_tbi_model.py), by the host build of the device's stage
functions (tests/test_hostemu_tabix.py) and on the device (tests/test_gpu_tabix.py) -- and the region queries that go with them.
Test infrastructure only."""
import random

import tbi_model as tm

SLICE = tm.SLICE
_cache = {}


def line(name, beg, end, extra=None):
    return b"%s\t%d\t%d%s\n" % (name, beg, end, b"" if extra is None else b"\t" + extra)


def padded_to(text, total, name, beg, end):
    """text + one more line name:beg-end whose column 4 is as long as it takes for the whole to have `total` bytes"""
    bare = line(name, beg, end, b"")
    fill = total - len(text) - len(bare)
    assert fill >= 0
    return text + line(name, beg, end, b"x" * fill)


def _rows(name, n, first=100, step=37, length=120, extra=b"AAACGGGTCATTCGAG\t1"):
    return b"".join(line(name, first + i * step, first + i * step + length, extra) for i in range(n))


def small_texts():
    if "small" not in _cache:
        t = {}
        t["empty"] = b""
        t["one_line"] = line(b"chr1", 100, 200)
        t["contigs_300"] = b"".join(line(b"ctg%03d" % i, 10 * i, 10 * i + 50, b"N") for i in range(300))
        t["one_bin"] = _rows(b"chr1", 500, first=5 * 16384 + 3, step=30, length=90)   # all within [5, 6) * 16384
        _cache["small"] = t
    return _cache["small"]


def edge_texts():
    """slice (0xff00 bytes) and tile (4096 bytes) edges"""
    if "edge" not in _cache:
        t = {}
        body = _rows(b"chr1", 1500)
        body = body[:body.rindex(b"\n", 0, SLICE - 200) + 1]
        last = 100 + 37 * body.count(b"\n")
        ends = padded_to(body, SLICE, b"chr1", last, last + 10)       # the last line ends exactly at byte 0xff00: the text's end
        assert len(ends) == SLICE
        t["line_ends_at_slice"] = ends
        t["line_begins_at_slice"] = ends + _rows(b"chr1", 40, first=last + 50)
        strad = padded_to(body, SLICE + 17, b"chr1", last, last + 10)  # a line across the boundary
        t["line_straddles_slice"] = strad + _rows(b"chr1", 40, first=last + 50)
        two = t["line_begins_at_slice"] + _rows(b"chr2", 1400)
        two = two[:two.rindex(b"\n", 0, 2 * SLICE - 200) + 1]
        t["exactly_two_slices"] = padded_to(two, 2 * SLICE, b"chr2", 90000, 90010)
        assert len(t["exactly_two_slices"]) == 2 * SLICE
        # lines of 5000 bytes: whole tiles of 4096 bytes without a newline, lines longer than a tile
        t["long_lines"] = b"".join(line(b"chr%d" % (1 + i // 25), 1000 * (i % 25), 1000 * (i % 25) + 300, b"y" * 4980) for i in range(45))
        # three names whose runs each cross a slice boundary
        t["name_runs_cross_slices"] = _rows(b"chrA", 1200) + _rows(b"chrB_with_a_longer_name", 1700) + _rows(b"chrC", 1500)
        assert len(t["name_runs_cross_slices"]) > 2 * SLICE
        _cache["edge"] = t
    return _cache["edge"]


LADDER = [k << s for s in (14, 17, 20, 23, 26) for k in (1, 3)]
LADDER_NAMES = (b"chr1", b"chr2", b"chrX")


def ladder_text():
    """records on every bin boundary, a few thousand random fragments (most below 3 Mb: empty windows and back-fill above), three names"""
    if "ladder" not in _cache:
        out = []
        for ci, name in enumerate(LADDER_NAMES):
            rng = random.Random(5 + ci)
            recs = []
            for B in LADDER:
                recs += [(B - 1, B), (B - 1, B + 1), (B, B + 1), (B - 150, B), (B - 150, B + 150), (B - 2, B - 1)]
            recs += [(0, 1), (0, 70000), (5, 5)]
            if ci < 2:
                recs.append(((1 << 29) - 200, 1 << 29))
            for _ in range(2500):
                b = rng.randrange(3000000) if rng.random() < 0.9 else rng.randrange(1 << 28)
                recs.append((b, b + rng.randrange(1, 1200)))
            recs.sort()
            out += [line(name, b, e, b"ACGTACGTACGTACGT\t%d" % (i % 7)) for i, (b, e) in enumerate(recs)]
        _cache["ladder"] = b"".join(out)
    return _cache["ladder"]


def ladder_queries():
    q = []
    for name in LADDER_NAMES:
        for B in LADDER:
            q += [(name, B - 1, B), (name, B, B + 1), (name, B + 1, B + 2), (name, B - 1, B + 1), (name, B - 200, B + 200)]
        # windows no record overlaps (above the random fragments, between the ladder's steps), and one beyond every record
        q += [(name, 300000000, 300000100), (name, 420000000, 420100000), (name, (1 << 29) - 100, 1 << 29), (name, 0, 1), (name, 5, 6),
              (name, 69999, 70001), (name, 0, 1 << 29)]
    q.append((b"chr_not_there", 0, 1000))
    return q


def big_text():
    """more than 2 048 slices (one compressor launch holds 2 048) at about 1 KB per line, two names"""
    if "big" not in _cache:
        n_bytes = 2051 * SLICE + 777
        n = n_bytes // len(line(b"chr1", 0, 500, b"ACGT" * 240)) + 1   # (the shortest line)
        half = n // 2
        fill = b"ACGT" * 240
        parts = []
        for i in range(n):
            name, j = (b"chr1", i) if i < half else (b"chr2", i - half)
            parts.append(line(name, 997 * j, 997 * j + 500, fill))
        _cache["big"] = b"".join(parts)
        assert len(_cache["big"]) > 2049 * SLICE
    return _cache["big"]


def random_queries(text, n, seed=1):
    """n regions around the text's own records and between them"""
    rng = random.Random(seed)
    lines = text.splitlines()
    out = []
    for _ in range(n):
        cols = rng.choice(lines).split(b"\t")
        b = max(0, int(cols[1]) + rng.randrange(-40000, 40000))
        out.append((cols[0], b, b + rng.choice((1, 100, 20000, 500000))))
    return out


def check_queries(raw, payload, text, queries):
    """every query through the index returns what a scan of the text returns"""
    idx = tm.parse_tbi(payload)
    table = {}
    for ln in text.splitlines(True):
        cols = ln.split(b"\t", 3)
        b, e = int(cols[1]), int(cols[2])
        table.setdefault(cols[0], []).append((b, e if e > b else b + 1, ln))
    for name, beg, end in queries:
        want = [ln for b, e, ln in table.get(name, ()) if b < end and e > beg]
        assert tm.query(raw, idx, name, beg, end) == want, (name, beg, end)


# texts the indexer must refuse: name -> (text, the model's cause, the 1-based line, a piece of the library's message)
def refused_texts():
    good = _rows(b"chr1", 50) + _rows(b"chr2", 50)
    lines = good.splitlines(True)
    t = {}
    t["unsorted_start"] = (b"".join(lines[:30] + [line(b"chr1", 5, 90)] + lines[30:]), "not sorted", 31, "not sorted by start")
    t["name_recurs"] = (good + _rows(b"chr1", 3, first=900000), "name recurs", 101, "second run")
    t["end_beyond_2_29"] = (good + line(b"chr2", 1 << 28, (1 << 29) + 1), "beyond 2^29", 101, "2^29")
    t["two_columns"] = (b"".join(lines[:10] + [b"chr1\t500\n"] + lines[10:]), "malformed", 11, "malformed")
    t["non_digit"] = (b"".join(lines[:10] + [b"chr1\t5x0\t600\tN\n"] + lines[10:]), "malformed", 11, "malformed")
    t["no_final_newline"] = (good[:-1], "no final newline", 100, "newline")
    return t
