"""Plain dynamic-programming references for the alignment primitives (test infrastructure only).

Integer DP tables in numpy, one table row at a time, batched over cases: every function takes one
case (bytes) or a batch (2-D uint8 arrays, one case per row; all cases of a batch share e and L).
No bit vectors and no code shared with oracle/ or cm_stages.h: the conventions below are restated
from the reference's text (alignment.cc, ksw.cc), the arithmetic is the textbook recurrence.

Conventions of the band (BandedAlignPatternToText, alignment.cc:141-192):
  window  L + 2e bases, read L bases; cell (i, j) = read base i against window base j, used only
          where 0 <= j - i <= 2e, anything outside the band is unreachable;
  start   free over window positions 0 .. 2e (the row above the table is 0 everywhere);
  cost    1 per substitution, inserted or deleted base; two bases match when their classes are
          equal (A C G T in either case: 0..3, every other byte: 4, so N matches N);
  end     the minimum of the last row over its 2e + 1 cells, the cell at offset e on a tie, else
          the first minimum;
  exit    e + 1 (and no end position: -1 here) as soon as a diagonal-0 cell (i, i) exceeds 3e.
"""
import numpy as np

BIG = 1 << 20

_CLS = np.full(256, 4, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CLS[_c] = _i
    _CLS[_c + 32] = _i


def classes(x):
    """CharToUint8 (utils.h:87-104) of bytes / a uint8 array"""
    return _CLS[np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else np.asarray(x, np.uint8)]


def _batch(window, read):
    single = isinstance(window, (bytes, bytearray)) or np.asarray(window).ndim == 1
    w = np.atleast_2d(np.frombuffer(window, np.uint8) if isinstance(window, (bytes, bytearray)) else np.asarray(window, np.uint8))
    r = np.frombuffer(read, np.uint8) if isinstance(read, (bytes, bytearray)) else np.asarray(read, np.uint8)
    r = r.reshape(w.shape[0], -1)
    return single, w, r


def _band_rows(e, wc, rc, stop_above):
    """Rows of the band table for class arrays wc (n, >= L + 2e) and rc (n, L).  Yields nothing; returns
    (rows, stopped) with rows[i + 1] = the (n, 2e + 1) cells of read base i (index k = j - i), rows[0] = the free row, and
    stopped[n] = the first i whose diagonal-0 cell exceeds stop_above (L when none does).  A case's rows after its stop are
    not meaningful."""
    n, L = rc.shape
    B = 2 * e + 1
    ks = np.arange(B)
    prev = np.zeros((n, B), np.int64)
    rows = [prev]
    stopped = np.full(n, L, np.int64)
    for i in range(L):
        sub = (wc[:, i:i + B] != rc[:, i:i + 1]).astype(np.int64)
        up = np.concatenate([prev[:, 1:], np.full((n, 1), BIG, np.int64)], axis=1) + 1  # (i - 1, j): diagonal k + 1 of the row above
        t = np.minimum(prev + sub, up)
        cur = np.minimum.accumulate(t - ks, axis=1) + ks  # the left neighbour, cost 1 per step, swept along the row
        rows.append(cur)
        first = (cur[:, 0] > stop_above) & (stopped == L)
        stopped[first] = i
        prev = cur
    return rows, stopped


def _pick_end(e, last):
    """(minimum, offset) of one band row per case: offset e on a tie, else the first minimum"""
    mn = last.min(axis=1)
    off = np.argmin(last, axis=1)
    off = np.where(last[:, e] == mn, e, off)
    return mn, off


def band_distance(e, window, read):
    """(errors, end) of the banded semi-global edit distance; end is the window index of the last aligned base"""
    single, w, r = _batch(window, read)
    L = r.shape[1]
    assert w.shape[1] >= L + 2 * e
    rows, stopped = _band_rows(e, classes(w), classes(r), 3 * e)
    mn, off = _pick_end(e, rows[L])
    err = np.where(stopped < L, e + 1, mn)
    end = np.where(stopped < L, -1, L - 1 + off)
    return (int(err[0]), int(end[0])) if single else (err, end)


def band_start(e, errors, window, read):
    """start offset of the alignment in the window (BandedTraceback, alignment.cc:656-718): e when the distance is 0 or equals
    the raw byte-wise Hamming count at offset e; else the band run over both strings reversed, whose last row is searched for
    cells equal to `errors` at reversed end offsets 1 .. 2e: offset e if it is one, else the largest, and 2e - offset is the
    start (2e when there is none)."""
    single, w, r = _batch(window, read)
    n, L = r.shape
    errors = np.broadcast_to(np.asarray(errors, np.int64), (n,))
    ham = (w[:, e:e + L] != r).sum(axis=1)
    rows, _ = _band_rows(e, classes(w[:, :L + 2 * e][:, ::-1]), classes(r[:, ::-1]), BIG)
    hit = rows[L] == errors[:, None]
    hit[:, 0] = False
    k = np.where(hit.any(axis=1), 2 * e - np.argmax(hit[:, ::-1], axis=1), 0)
    k = np.where(hit[:, e], e, k)
    start = np.where((errors == 0) | (ham == errors), e, 2 * e - k)
    return int(start[0]) if single else start


def dropoff(e, window, read):
    """(errors, end, mapped_length) of BandedAlignPatternToTextWithDropOff (alignment.cc:197-283): the band stops at the first
    read base i whose diagonal-0 cell exceeds 2e; the answer is read off the row before it (the free row when i = 0), and
    mapped_length = i.  end is negated when the stop came early (i < 4e and i < L / 2) or, for reads over 60 bases, when
    fewer than 30 bases are left (end + 1 - e - errors < 30).  The 3'-end form (alignment.cc:285-376) is this function on the
    reversed window and the reversed read."""
    single, w, r = _batch(window, read)
    n, L = r.shape
    rows, stopped = _band_rows(e, classes(w), classes(r), 2 * e)
    table = np.stack(rows, axis=1)  # (n, L + 1, 2e + 1)
    last = table[np.arange(n), stopped]  # rows[i] is the row of read base i - 1
    mn, off = _pick_end(e, last)
    end = stopped - 1 + off
    fail = (stopped < L) & (stopped < 4 * e) & (stopped < L // 2)
    short = (L > 60) & (end + 1 - e - mn < 30)
    end = np.where(fail | short, -end, end)
    return (int(mn[0]), int(end[0]), int(stopped[0])) if single else (mn, end, stopped)


GAP_OPEN, GAP_EXT, MATCH, MISMATCH = 6, 1, 1, -4


def affine_best(window, read, w):
    """(score, end) of ksw_semi_global3 (ksw.cc:505-626): affine-gap DP, read = rows, window = columns, cell (i, j) used where
    0 <= j - i <= w.  The first read base may start at window columns 0 .. w for free; a gap of n bases costs 6 + n and is
    opened from a diagonal move only (ksw's recurrence: E and F take `M - 7`, M = diagonal predecessor + substitution score,
    not the cell's maximum); a base of class 4 on either side scores 0.  The end is the best of the last row's cells among
    the last w window columns, the rightmost on a tie; `end` is one past the last aligned window base."""
    single, wb, rb = _batch(window, read)
    wc, rc = classes(wb).astype(np.int64), classes(rb).astype(np.int64)
    n, L = rc.shape
    Q = wc.shape[1]
    NEG = -(1 << 40)
    oe = GAP_OPEN + GAP_EXT
    # full (Q) columns per row, out-of-band cells at NEG
    cols = np.arange(Q)
    Hprev = np.full((n, Q), NEG, np.int64)       # H(i - 1, j)
    Eprev = np.full((n, Q), NEG, np.int64)       # vertical gap state leaving (i - 1, j) downwards
    for i in range(L):
        inband = (cols >= i) & (cols <= i + w)
        if i == 0:
            diag = np.zeros((n, Q), np.int64)
        else:
            diag = np.concatenate([np.full((n, 1), NEG, np.int64), Hprev[:, :-1]], axis=1)
        amb = (wc > 3) | (rc[:, i:i + 1] > 3)
        sc = np.where(amb, 0, np.where(wc == rc[:, i:i + 1], MATCH, MISMATCH))
        M = np.where(inband, diag + sc, NEG)
        M = np.maximum(M, NEG)
        # horizontal gap entering cell j: max over j' < j of M(i, j') - 6 - (j - j')
        F = np.maximum.accumulate(np.concatenate([np.full((n, 1), NEG, np.int64), (M - GAP_OPEN + cols)[:, :-1]], axis=1), axis=1) - cols
        F = np.maximum(F, NEG)
        H = np.where(inband, np.maximum(np.maximum(M, Eprev), F), NEG)
        Eprev = np.where(inband, np.maximum(Eprev - GAP_EXT, M - oe), NEG)
        Eprev = np.maximum(Eprev, NEG)
        Hprev = H
    tail = Hprev[:, Q - w:]  # window columns Q - w .. Q - 1 -> end = column + 1
    score = tail.max(axis=1)
    end = Q - np.argmax(tail[:, ::-1], axis=1)
    return (int(score[0]), int(end[0])) if single else (score, end)


def global_affine(ref_span, read):
    """the plain unbanded global optimum (Gotoh, gap of n bases = -(6 + n), gaps may follow one another) of one read against
    one reference span; both are consumed entirely"""
    a, b = classes(read).astype(np.int64), classes(ref_span).astype(np.int64)
    n, m = len(a), len(b)
    NEG = -(1 << 40)
    js = np.arange(m + 1)
    H = np.where(js == 0, 0, -(GAP_OPEN + GAP_EXT * js))
    E = np.full(m + 1, NEG, np.int64)
    for i in range(1, n + 1):
        E = np.maximum(E - GAP_EXT, H - GAP_OPEN - GAP_EXT)      # read base i - 1 inserted
        sc = np.where((b > 3) | (a[i - 1] > 3), 0, np.where(b == a[i - 1], MATCH, MISMATCH))
        T = np.maximum(E, np.concatenate([[NEG], H[:-1] + sc]))
        T[0] = -(GAP_OPEN + GAP_EXT * i)
        # deletions along the row: H[j] = max(T[j], max over j' < j of H[j'] - 6 - (j - j')), and H[j'] may be replaced by T[j']
        F = np.maximum.accumulate(np.concatenate([[NEG], (T - GAP_OPEN + js)[:-1]])) - js
        H = np.maximum(T, F)
        E[0] = NEG
    return int(H[m])


CIGAR_OPS = "MIDNSHP=X"


def parse_cigar(cigar):
    """'12M3I' or packed uint32 (len << 4 | op) -> [(op letter, length)]"""
    if isinstance(cigar, (str, bytes)):
        s = cigar.decode() if isinstance(cigar, bytes) else cigar
        out, num = [], ""
        for ch in s:
            if ch.isdigit():
                num += ch
            else:
                assert num, "CIGAR operation without a length: %r" % s
                out.append((ch, int(num)))
                num = ""
        assert not num, "CIGAR ends in a number: %r" % s
        return out
    return [c if isinstance(c, tuple) else (CIGAR_OPS[int(c) & 0xf], int(c) >> 4) for c in cigar]


def replay(cigar, ref_span, read):
    """(score, NM, MD) of an alignment given as a CIGAR (M / I / D / S), recomputed base by base.  Asserts that the CIGAR
    consumes exactly the read and exactly the reference span, that no operation is empty and that neighbours differ.
    score: match 1, mismatch -4, class-4 base 0, gap of n bases -(6 + n).  NM / MD as GenerateNMAndMDTag (alignment.cc:85-139)
    writes them: a base matches when the bytes are equal or the reference byte is the read's letter in lower case."""
    ops = parse_cigar(cigar)
    ref_span, read = bytes(ref_span), bytes(read)
    rc, fc = classes(read), classes(ref_span)
    rp = fp = score = nm = run = 0
    md = []
    last = None
    for op, ln in ops:
        assert ln > 0, "empty CIGAR operation"
        assert op != last, "two neighbouring %s operations" % op
        last = op
        if op == "M":
            assert rp + ln <= len(read) and fp + ln <= len(ref_span), "M runs past the read or the reference span"
            for _ in range(ln):
                a, b = rc[rp], fc[fp]
                score += 0 if (a > 3 or b > 3) else (MATCH if a == b else MISMATCH)
                if ref_span[fp] == read[rp] or ref_span[fp] - 32 == read[rp]:
                    run += 1
                else:
                    nm += 1
                    md.append(str(run) + chr(ref_span[fp]))
                    run = 0
                rp += 1
                fp += 1
        elif op == "I":
            assert rp + ln <= len(read), "I runs past the read"
            score -= GAP_OPEN + GAP_EXT * ln
            nm += ln
            rp += ln
        elif op == "D":
            assert fp + ln <= len(ref_span), "D runs past the reference span"
            score -= GAP_OPEN + GAP_EXT * ln
            nm += ln
            md.append(str(run) + "^" + ref_span[fp:fp + ln].decode("latin-1"))
            run = 0
            fp += ln
        elif op == "S":
            rp += ln
        else:
            raise AssertionError("unexpected CIGAR operation " + op)
    md.append(str(run))
    assert rp == len(read), "CIGAR consumes %d read bases of %d" % (rp, len(read))
    assert fp == len(ref_span), "CIGAR consumes %d reference bases of %d" % (fp, len(ref_span))
    return score, nm, "".join(md)


# ---- gap-rich cases -------------------------------------------------------------------------
WORD_LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 150)
_ACGT = np.frombuffer(b"ACGT", np.uint8)
_ODD = np.frombuffer(b"NNacgtRYKMnx", np.uint8)


def geometric(rng, p, hi):
    """1 .. hi, each value p times as likely as the one before"""
    wts = p ** np.arange(hi)
    return 1 + int(rng.choice(hi, p=wts / wts.sum()))


def edit_script(rng, L, e, budget, end_share=0.3, len_p=None):
    """`budget` edits for a read of L bases: [(kind, read position, length)], kind 's' / 'i' / 'd', gaps of 1 .. e bases (uniform,
    or with len_p each length len_p times as likely as the one before), `end_share` of the gaps in the first or last 3 bases"""
    script = []
    for _ in range(budget):
        kind = "sid"[int(rng.integers(0, 3))]
        ln = 1 if kind == "s" else int(rng.integers(1, e + 1)) if len_p is None else geometric(rng, len_p, e)
        if kind != "s" and rng.random() < end_share:
            pos = int(rng.integers(0, 3)) if rng.random() < 0.5 else L - 1 - int(rng.integers(0, 3))
        else:
            pos = int(rng.integers(0, L))
        script.append((kind, max(0, min(L - 1, pos)), ln))
    return script


def apply_script(rng, src, L, script):
    """the bases of `src` (a uint8 array long enough to refill what deletions take) with the script applied at its read
    positions, cut to L bases.  Returns (read, applied): an edit whose position an earlier insertion has run over is dropped,
    and `applied` lists the ones that took place."""
    at = {}
    for kind, pos, ln in script:
        at.setdefault(pos, []).append((kind, ln))
    out, applied = [], []
    s = 0
    while len(out) < L:
        p = len(out)
        sub = False
        for kind, ln in at.pop(p, ()):
            applied.append((kind, p, ln))
            if kind == "i":
                out.extend(int(x) for x in _ACGT[rng.integers(0, 4, ln)])
            elif kind == "d":
                s += ln
            else:
                sub = True
        base = int(src[s])
        s += 1
        if sub:
            base = int(_ACGT[(int(classes(bytes([base]))[0]) + 1 + int(rng.integers(0, 3))) % 4])
        out.append(base)
    return np.array(out[:L], np.uint8), applied


def gap_rich_cases(seed, e, L, n, clean_text=False):
    """n (window, read) cases for one (e, L): random windows of L + 2e bases, reads = the window's middle under a script of
    0 .. e + 3 edits; 5 % of the bytes on either side N, lower case or IUPAC (clean_text: the read keeps to ACGTN, as the
    reverse complement of a read does).  Returns (windows (n, L + 2e), reads (n, L))."""
    rng = np.random.default_rng([seed, e, L])
    W = np.empty((n, L + 2 * e), np.uint8)
    R = np.empty((n, L), np.uint8)
    for c in range(n):
        long = _ACGT[rng.integers(0, 4, L + 4 * e + 8 + e * (e + 3))]
        W[c] = long[:L + 2 * e]
        script = edit_script(rng, L, e, int(rng.integers(0, e + 4)))
        shift = e + int(rng.integers(-1, 2)) if rng.random() < 0.2 else e
        R[c], _ = apply_script(rng, long[shift:], L, script)
        if rng.random() < 0.05:  # an unrelated read: the early exit
            R[c] = _ACGT[rng.integers(0, 4, L)]
        for arr, clean in ((W[c], False), (R[c], clean_text)):
            m = rng.random(len(arr)) < 0.05
            k = int(m.sum())
            if k:
                arr[m] = ord("N") if clean else np.where(rng.random(k) < 0.4, arr[m] | 0x20, _ODD[rng.integers(0, len(_ODD), k)])
    return W, R
