"""Crafted references for the index-build tests (tests/test_hostemu_index.py on the CPU,
tests/test_gpu_index_build.py and tests/test_gpu_reference_binary.py on the GPU).  Plain
module, deterministic, no files of its own: every generator returns [(name, bytes)].

The device builder cuts every sequence into chunks of CHUNK positions, starts each
WARM positions early and runs it 2w + 2 past its end (cm_ref_chunk_minimizers); the edge
reference puts what can go wrong there at, before and across the chunk seams.  Each
generator asserts, from the sequences alone, the properties its cases rely on."""
import numpy as np

CHUNK = 2048   # SY_CHUNK of cm_synth.hip
WARM = 96      # SY_WARM

PAL_UNITS = (b"AT", b"CG", b"ACGT")
PAL_LENGTHS = (40, 100, 160, 300)
_COMP = {65: 84, 67: 71, 71: 67, 84: 65}   # A C G T


def _random_bases(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.randint(0, 4, n)].copy()


def _tandem(unit, n):
    return np.frombuffer((unit * (n // len(unit) + 1))[:n], np.uint8)


def write_fasta(path, seqs, width=70):
    with open(path, "wb") as f:
        for name, s in seqs:
            f.write(b">" + name + b"\n")
            for i in range(0, len(s), width):
                f.write(s[i:i + width] + b"\n")
    return path


def runs_of(seq, pred):
    """maximal [start, end) intervals of positions i with pred[i]"""
    out, i, n = [], 0, len(pred)
    while i < n:
        if pred[i]:
            j = i
            while j < n and pred[j]:
                j += 1
            out.append((i, j))
            i = j
        else:
            i += 1
    return out


def n_runs(seq):
    a = np.frombuffer(seq, np.uint8)
    return runs_of(seq, a == ord("N"))


def palindromic_positions(seq, k):
    """pred[i]: the k-mer ending at i has k plain bases and equals its reverse complement (the positions the
    reference's minimizer pass skips, away from ambiguous bases)"""
    up = seq.upper()
    pred = np.zeros(len(seq), bool)
    for i in range(k - 1, len(seq)):
        km = up[i - k + 1:i + 1]
        if all(c in _COMP for c in km) and bytes(_COMP[c] for c in reversed(km)) == km:
            pred[i] = True
    return pred


def tandem_runs(seq, unit, min_len=24):
    """maximal runs of the tandem repeat of `unit` (any phase), at least min_len long"""
    up = np.frombuffer(seq.upper(), np.uint8)
    p = len(unit)
    same = np.zeros(len(up), bool)
    same[p:] = up[p:] == up[:-p]
    out = []
    for a, b in runs_of(seq, same):
        a -= p
        if b - a >= min_len and bytes(up[a:a + p]) in [(unit * 2)[i:i + p] for i in range(p)]:
            out.append((a, b))
    return out


def _placement(a, b, length):
    """how [a, b) lies to the seams inside a sequence of `length`: 'straddles', 'ends_before' (0 .. WARM positions
    before one) or 'inside'"""
    for m in range(CHUNK, length + 1, CHUNK):
        if a < m < b:
            return "straddles"
    for m in range(CHUNK, length + 1, CHUNK):
        if 0 <= m - b <= WARM:
            return "ends_before"
    return "inside"


UNIT_LEN = 700
LONG_N = 2106   # [1990, 4096) of the 4096-base sequence: chunk 1 of it has no minimizer


def edge_reference(k, w):
    """9 sequences, 14.9 kb at the most: a 4500-base one, four of exactly 2047, 2048, 2049 and 4096 bases, four of
    k - 1, k, k + w - 1 and k + w bases (a length of 0 is left out)."""
    rng = np.random.RandomState(20240 + 101 * k + w)
    unit = _random_bases(rng, UNIT_LEN)
    lens = {"main": 4500, "s2047": 2047, "s2048": 2048, "s2049": 2049, "s4096": 4096}
    seq = {n: _random_bases(rng, l) for n, l in lens.items()}

    def put(name, start, data):
        assert 0 <= start and start + len(data) <= lens[name]
        seq[name][start:start + len(data)] = data

    def pal(name, start, unit_, n):
        put(name, start, _tandem(unit_, n))
        # the neighbours must not continue the run
        for at, nb in ((start - 1, start + len(unit_) - 1), (start + n, start + n - len(unit_))):
            if 0 <= at < lens[name] and seq[name][at] == seq[name][nb]:
                seq[name][at] = {65: 67, 67: 65, 71: 84, 84: 71}[int(seq[name][nb])]

    def ns(name, start, n):
        put(name, start, np.full(n, ord("N"), np.uint8))
        for at in (start - 1, start + n):
            if 0 <= at < lens[name] and seq[name][at] == ord("N"):
                seq[name][at] = ord("A")

    # the planted unit: three copies -> multi-occurrence keys
    put("main", 100, unit)
    put("main", 2400, unit)
    put("s2049", 300, unit)
    # main: seams at 2048 and 4096
    pal("main", 0, b"AT", 40)               # starts at position 0
    pal("main", 850, b"ACGT", 100)          # inside a chunk
    ns("main", 1000, w)                     # inside
    ns("main", 1100, 97)                    # inside
    pal("main", 1900, b"AT", 300)           # straddles 2048
    ns("main", 2300, 1)                     # inside
    ns("main", 3200, 200)                   # inside
    pal("main", 3500, b"CG", 160)           # inside
    pal("main", 3900, b"CG", 100)           # ends 96 before 4096
    ns("main", 4000, 200)                   # straddles 4096
    seq["main"][4250:4290] = np.frombuffer(bytes(seq["main"][4250:4290]).lower(), np.uint8)
    seq["main"][4300] = ord("R")            # an IUPAC code
    pal("main", 4460, b"ACGT", 40)          # ends at the sequence end
    # 2047: no seam inside
    pal("s2047", 500, b"AT", 160)
    pal("s2047", 900, b"ACGT", 160)
    ns("s2047", 1900, 97)
    ns("s2047", 2047 - w, w)                # ends at the sequence end
    # 2048: the seam is the sequence end
    ns("s2048", 0, 95)                      # starts at position 0
    pal("s2048", 300, b"AT", 100)
    pal("s2048", 700, b"CG", 40)
    pal("s2048", 1748, b"ACGT", 300)        # ends at the seam = at the sequence end
    # 2049: one position behind the seam
    ns("s2049", 1100, 96)
    pal("s2049", 1300, b"CG", 300)
    ns("s2049", 1700, 1)
    ns("s2049", 1870, 95)                   # ends 83 before 2048
    pal("s2049", 2009, b"CG", 40)           # straddles 2048, ends at the sequence end
    # 4096: a run of N over the whole second chunk
    pal("s4096", 200, b"ACGT", 300)
    pal("s4096", 700, b"AT", 40)
    ns("s4096", 900, w)
    pal("s4096", 1100, b"ACGT", 100)
    ns("s4096", 1500, 96)                   # inside
    ns("s4096", 1700, 200)                  # inside
    pal("s4096", 1920, b"CG", 60)           # ends 68 before 2048
    ns("s4096", 1985, 1)                    # ends 62 before 2048
    ns("s4096", 1990, LONG_N)               # straddles 2048, ends at the sequence end

    out = [(n.encode(), bytes(seq[n])) for n in ("main", "s2047", "s2048", "s2049", "s4096")]
    for ln in sorted({k - 1, k, k + w - 1, k + w}):
        if ln > 0:
            out.append((b"tiny%d" % ln, bytes(_random_bases(rng, ln))))
    _check_edge_reference(out, k, w)
    return out


def _check_edge_reference(seqs, k, w):
    by = dict(seqs)
    assert 5 <= len(seqs) <= 9 and 12000 <= sum(len(s) for _, s in seqs) <= 15000
    assert {2047, 2048, 2049, 4096} <= {len(s) for _, s in seqs}
    assert {k, k + w - 1, k + w} <= {len(s) for _, s in seqs} and (k == 1 or k - 1 in {len(s) for _, s in seqs})
    # palindromic tandem runs: every unit and every length, the three placements, both sequence ends
    found, places, at0, at_end = set(), set(), False, False
    for name, s in seqs:
        for u in PAL_UNITS:
            for a, b in tandem_runs(s, u):
                found.add((u, b - a))
                places.add(_placement(a, b, len(s)))
                at0 |= a == 0
                at_end |= b == len(s)
    assert {(u, l) for u in PAL_UNITS for l in PAL_LENGTHS} <= found, found
    assert places == {"straddles", "ends_before", "inside"} and at0 and at_end
    # runs of N: 1, w, 95, 96, 97, 200 and one that leaves a whole chunk without a k-mer
    nl, nplaces, n0, nend, empty_chunk = set(), set(), False, False, False
    for name, s in seqs:
        for a, b in n_runs(s):
            nl.add(b - a)
            nplaces.add(_placement(a, b, len(s)))
            n0 |= a == 0
            nend |= b == len(s)
            empty_chunk |= any(a <= m and m + CHUNK <= b for m in range(0, len(s), CHUNK))
    assert {1, w, 95, 96, 97, 200} <= nl, nl
    assert max(nl) > CHUNK and empty_chunk
    assert nplaces == {"straddles", "ends_before", "inside"} and n0 and nend
    # lower case and one IUPAC code
    main = by[b"main"]
    assert any(c in b"acgt" for c in main) and sum(c not in b"ACGTNacgt" for c in main) == 1
    # the unit: three copies
    u = main[100:100 + UNIT_LEN]
    assert sum(s.count(u) for _, s in seqs) == 3
    # even k: a stretch of at least 2w + 2 + k positions that do not advance the minimizer window lies over a seam,
    # so the chunk behind the seam starts inside it and the chunk in front of it ends inside it
    if k % 2 == 0:
        ok = False
        for name, s in seqs:
            pred = palindromic_positions(s, k)
            for a, b in runs_of(s, pred):
                ok |= b - a >= 2 * w + 2 + k and any(a < m < b for m in range(CHUNK, len(s), CHUNK))
        assert ok, (k, w)


def placement_sweep():
    """360 placements of one palindromic tandem run over 7000 random bases, around the first seam: yields
    (unit, start, length, sequence)"""
    rng = np.random.RandomState(7000)
    base = _random_bases(rng, 7000)
    n = 0
    for unit in PAL_UNITS:
        for length in (24, 40, 60, 100, 160, 300):
            for start in range(1880, 2052, 9):
                s = base.copy()
                s[start:start + length] = _tandem(unit, length)
                n += 1
                yield unit, start, length, bytes(s)
    assert n == 360


# ---- tiny references for the table-sizing seams -------------------------------------------
# one random sequence cut after TINY_LENGTHS[n_keys] bases has n_keys distinct minimizers at k 17, w 7 (the test
# asks the oracle); khash then has 4, 4, 8, 8, 16, 16, 32 buckets
TINY_K, TINY_W = 17, 7
TINY_BUCKETS = {1: 4, 3: 4, 4: 8, 6: 8, 7: 16, 12: 16, 13: 32}
TINY_LENGTHS = {1: 17, 3: 26, 4: 33, 6: 40, 7: 45, 12: 64, 13: 65}


def tiny_sequence():
    return bytes(_random_bases(np.random.RandomState(4242), 400))


def tiny_reference(n_bases):
    return [(b"tiny", tiny_sequence()[:n_bases])]


def no_kmer_reference(k):
    """nothing the builder can index: every sequence is shorter than k or has an N in every k-mer"""
    rng = np.random.RandomState(99)
    a = _random_bases(rng, 3 * k)
    a[k - 1::k] = ord("N")
    return [(b"short", bytes(_random_bases(rng, max(1, k - 1)))), (b"holes", bytes(a))]


def ref_view(seqs):
    """the C ABI's view of [(name, bytes)]: (RefView, objects that own its memory)"""
    import ctypes as C
    from chromap_amd import _capi
    n = len(seqs)
    names = (C.c_char_p * n)(*[nm for nm, _ in seqs])
    bufs = [C.create_string_buffer(s, len(s) + 64) for _, s in seqs]   # (the loaders pad sequences the same way)
    ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    lens = (C.c_uint32 * n)(*[len(s) for _, s in seqs])
    rv = _capi.RefView(n, names, ptrs, lens)
    return rv, (names, bufs, ptrs, lens)
