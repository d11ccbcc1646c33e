"""The argument tuples on which the MAPQ functions are compared (tests/test_mapq_cpu.py, tests/test_gpu_mapq.py,
tests/hostemu/mapq_san_main.cpp): the model of tests/mapq_model.py, the product's stage functions on the host and on the device, and
the oracle's.  Deterministic (no random numbers: crossed value lists, and index arithmetic where a full cross would be too large);
at most MAX_CASES tuples in all.

groups() returns a list of Group(name, kind, e, reads, pairs): the two int32 matrices of cmgpu_debug_mapq (include/chromap_amd_debug.h),
reads [9, 2 n] and pairs [6, n], for one kind and one error threshold.

Three families.
  single  (kind SINGLE; e in 3, 8, 12, 15, max_num_error_difference 2 and e): every table index 1 .. 65535; the lengths 45 .. 55 around
          the table's switch crossed with each other argument's values (a full cross of the small lists, and each long list on its own);
          alignment length below / equal to / above the read length; 0 .. 15 errors; second_min_num_errors from three below the errors
          to two above errors + max_diff, and e + 1, which the stages keep when there is no second-best mapping; 0 .. 3 best mappings;
          num_second_best_mappings 0 and b - 1, b, b + 1 for each of the 94 breakpoints of the penalty; repeat lengths 0, 1, L / 3,
          L - 1, L, L + 1, 2 L; and the 35 (errors, length) pairs whose identity is exactly 19/20, 97/100 or 999/1000, with the two
          neighbouring lengths.
  paired  (kind PAIRED): reads taken from the single family's value lists, the alignment shorter than, as long as and longer than the
          read, and the 35 threshold pairs with their neighbours (with themselves and with an error-free mate, so that the pair's
          identity stands exactly at 0.95, 0.97 and 0.999); the pair's min_sum and second_sum around
          min1 + min2 + 3; 0, 1, 2 best pairs; second-best pairs at the breakpoints (so that the penalty exceeds mapq_pe and the
          uint8_t wraps); repeat lengths whose sum is below, equal to and above the two read lengths; force_mapq -1 and 0.
  split   (kinds SPLIT and PAIRED_SPLIT; e in 2, 4, 6, 8, 12, 15): errors are the negated aligned lengths the split verification
          stores; alignment lengths on both sides of read_length - e and of read_length / 3; 0, 4, 5, 9, 10, 50, 1000, 2^20 candidates
          on the strand; num_second_best_mappings / diff below, at and above 1.

Left out, because the reference leaves the result undefined and x86 and gfx950 may then legitimately differ:
  * an alignment length of 0 (with a read length of 0 in the non-split form): a division by zero and log(0)
  * a read length of 0: repetitive_seed_length / 0
  * split tuples with num_second_best_mappings / diff + 1 == 0: the reference divides by it
  * anything whose double does not fit the integer type it is converted to (none of the lists reaches that: the largest value before
    a conversion is below 2^25); read lengths stay below 65536 in the non-split form, where the reference stores them into a uint16_t
"""
import collections
import math

import numpy as np

import mapq_model as mm

MAX_CASES = 3_000_000
NONE = 99  # second-error code: no second-best mapping (second_min_num_errors stays e + 1)
Group = collections.namedtuple("Group", "name kind e reads pairs")
_GROUPS = None


def breakpoints():
    """brk[v] = the smallest n >= 1 with (int)(4.343 * log(n + 1) + 0.499) >= v, for every v an int n reaches"""
    def f(n):
        return int(4.343 * math.log(n + 1) + 0.499)
    out = []
    v = 0
    while f(0x7fffffff) >= v:
        lo, hi = 1, 0x7fffffff
        while lo < hi:
            mid = (lo + hi) // 2
            if f(mid) >= v:
                hi = mid
            else:
                lo = mid + 1
        out.append(lo)
        v += 1
    return out


def nsec_values():
    """0 and b - 1, b, b + 1 for every breakpoint b"""
    s = {0}
    for b in breakpoints():
        s.update((b - 1, b, b + 1))
    return sorted(v for v in s if 0 <= v <= 0x7ffffffe)


def threshold_pairs():
    """the (errors, length) pairs with errors / length exactly 1/20, 3/100 or 1/1000, up to 15 errors: 15 + 5 + 15"""
    return [(k, 20 * k) for k in range(1, 16)] + [(3 * k, 100 * k) for k in range(1, 6)] + [(k, 1000 * k) for k in range(1, 16)]


def cross(*lists):
    g = np.meshgrid(*[np.asarray(l, np.int64) for l in lists], indexing="ij")
    return [a.ravel() for a in g]


def _second(err, code, e):
    return np.where(code == NONE, e + 1, err + code)


def _rep(rl, code):
    return np.choose(code, [0 * rl, 0 * rl + 1, rl // 3, rl - 1, rl, rl + 1, 2 * rl])


def _lenform(L, form):
    """(alignment_length, read_length) whose larger one is L: equal, alignment longer, read longer"""
    al = np.where(form == 2, np.maximum(L - 5, 1), L)
    rl = np.where(form == 1, np.maximum(L - 5, 1), L)
    return al, rl


def _pack_single(rows, e, name, kind=mm.SINGLE):
    """rows: list of dicts of equal-length int64 arrays (err al rl md second n_best n_second rep [ncand])"""
    cat = {k: np.concatenate([np.broadcast_to(np.asarray(r.get(k, 0), np.int64), r["err"].shape) for r in rows])
           for k in ("err", "al", "rl", "md", "second", "n_best", "n_second", "rep", "ncand")}
    n = len(cat["err"])
    reads = np.zeros((9, 2 * n), np.int32)
    for c, k in enumerate(("err", "al", "rl", None, "second", "n_best", "n_second", "rep", "ncand")):
        if k:
            reads[c, 0::2] = cat[k]
    reads[3, 0::2] = cat["err"]
    reads[2, 1::2] = 1  # the unused mate: a defined read all the same
    reads[1, 1::2] = 1
    pairs = np.zeros((6, n), np.int32)
    pairs[0] = cat["md"]
    return Group(name, kind, e, reads, pairs)


# ---------------------------------------------------------------- single
def _single_group(e, every_length_variants):
    NS = np.array(nsec_values(), np.int64)
    rows = []
    for md in (2, e):
        codes = list(range(-3, md + 3)) + [NONE]
        # the table's switch: lengths 45 .. 55, full cross of the short lists
        L, err, code, nb, ns, rc = cross(range(45, 56), range(16), codes, range(4), (0, 2), (0, 2))
        rows.append(dict(err=err, al=L, rl=L, md=md, second=_second(err, code, e), n_best=nb, n_second=ns, rep=_rep(L, rc)))
        # ... each long list on its own: the second-best counts, the repeat lengths with the three length forms
        L, ns, err, nb = cross(range(45, 56), NS, (0, 1, 5), (0, 1))
        rows.append(dict(err=err, al=L, rl=L, md=md, second=_second(err, 0 * err + NONE, e), n_best=nb, n_second=ns, rep=0))
        L, rc, err, form, code = cross(range(45, 56), range(7), range(16), range(3), (1, NONE))
        al, rl = _lenform(L, form)
        rows.append(dict(err=err, al=al, rl=rl, md=md, second=_second(err, code, e), n_best=1, n_second=0, rep=_rep(rl, rc)))
        # the identity thresholds with their neighbours
        tp = threshold_pairs()
        t, dl, rc, nb, code, form, ns = cross(range(len(tp)), (-1, 0, 1), range(1, 7), (0, 1), (1, 2, NONE), range(3), (0, 1))
        err = np.array([p[0] for p in tp], np.int64)[t]
        L = np.array([p[1] for p in tp], np.int64)[t] + dl
        al = np.where(form == 2, L - 3, L)  # the larger of the two is L
        rl = np.where(form == 1, L - 3, L)
        rows.append(dict(err=err, al=al, rl=rl, md=md, second=_second(err, code, e), n_best=nb, n_second=ns, rep=_rep(rl, rc)))
        # the breakpoints at ordinary read lengths
        ns, err, L, code, rc = cross(NS, (0, 2), (36, 50, 100, 151), (1, NONE), (0, 2))
        rows.append(dict(err=err, al=L, rl=L, md=md, second=_second(err, code, e), n_best=1, n_second=ns, rep=_rep(L, rc)))
    # every table index: the larger of (alignment length, read length) = a
    for v in range(every_length_variants):
        a = np.arange(1, 65536, dtype=np.int64)
        if v < 3:
            al, rl = a, [a, np.maximum(a - 1, 1), np.maximum(a // 2, 1)][v]
        else:
            al, rl = np.maximum(a - 1 - a % 7, 1), a
        md = np.where((a + v) % 2 == 0, 2, e)
        err = (a * 7 + v) % 16
        code = (a * 5 + v) % (md + 7) - 3
        code = np.where(code == md + 3, NONE, code)
        nb = np.array([1, 1, 0, 1, 2, 1, 3, 1], np.int64)[(a + v) % 8]
        ns = np.where(a % 5 == 0, NS[(a * 13 + v) % len(NS)], np.array([0, 0, 1, 0, 2, 0, 7], np.int64)[a % 7])
        rows.append(dict(err=err, al=al, rl=rl, md=md, second=_second(err, code, e), n_best=nb, n_second=ns,
                         rep=_rep(rl, (a * 3 + v) % 11 % 7)))
    return _pack_single(rows, e, "single_e%d" % e)


# ---------------------------------------------------------------- paired
def _pick(k, P):
    """two members of a pool of P per index, from the digits of a scrambled index"""
    h = (k * 2654435761 + 12345) % (1 << 32)
    return h % P, (h // P) % P


def _read_pool(e):
    """reads for the pairs: the single family's values at max_num_error_difference 2, the alignment as long as the read, longer and
    shorter; then (the last n_threshold reads) the identity thresholds with their neighbouring lengths, every one with a repeat
    length.  Returns (pool, n_threshold)."""
    L, err, form, code, nb, ns, rc, dmin = cross((36, 50, 100, 151), (0, 1, 2, 5, 8), (0, 1, 2), (-1, 0, 1, 2, 3, NONE), (1, 2), (0, 1, 5, 100),
                                                 (0, 2, 4), (0, 1))
    al = np.where(form == 1, L + 2, np.where(form == 2, L - 5, L))
    a = dict(err=err, al=al, rl=L, min_err=np.maximum(err - dmin, 0), second=_second(err, code, e), n_best=nb, n_second=ns, rep=_rep(L, rc))
    tp = threshold_pairs()
    t, dl, form, rc, code = cross(range(len(tp)), (-1, 0, 1), range(3), (2, 4), (1, NONE))
    err = np.array([p[0] for p in tp], np.int64)[t]
    L = np.array([p[1] for p in tp], np.int64)[t] + dl  # the larger of alignment length and read length
    al = np.where(form == 2, L - 3, L)
    rl = np.where(form == 1, L - 3, L)
    b = dict(err=err, al=al, rl=rl, min_err=err, second=_second(err, code, e), n_best=0 * err + 1, n_second=0 * err, rep=_rep(rl, rc))
    pool = {k: np.concatenate([a[k], b[k]]) for k in a}
    pool["ncand"] = 0 * pool["err"]
    return pool, len(err)


def _pack_pairs(pool, i1, i2, cols, e, name, kind, rep1=None, rep2=None):
    n = len(i1)
    reads = np.zeros((9, 2 * n), np.int32)
    for c, k in enumerate(("err", "al", "rl", "min_err", "second", "n_best", "n_second", "rep", "ncand")):
        reads[c, 0::2] = pool[k][i1]
        reads[c, 1::2] = pool[k][i2]
    if rep1 is not None:
        reads[7, 0::2] = rep1
        reads[7, 1::2] = rep2
    pairs = np.zeros((6, n), np.int32)
    for c, v in enumerate(cols):
        pairs[c] = v
    return Group(name, kind, e, reads, pairs)


def _paired_group(e):
    pool, n_thr = _read_pool(e)
    P = len(pool["err"])
    NS = np.array(nsec_values(), np.int64)
    parts = []
    # pair-level values crossed, 400 read pairs
    k, dmin, dsec, nb, ns, force = cross(range(400), range(5), (0, 1, 2, 3, 4, 5, 7, NONE), (0, 1, 2), (0, 1, 5, 40, 2000, 1000000), (-1, 0))
    parts.append((k, dmin, dsec, nb, ns, force, None))
    # the breakpoints: penalties below and above mapq_pe
    ns, d, k, nb = cross(NS, range(6), range(400, 440), (0, 1))
    dmin = np.array([0, 0, 0, 0, 1, 2], np.int64)[d]
    dsec = np.array([1, 2, 3, 0, 0, 5], np.int64)[d]
    parts.append((k, dmin, dsec, nb, ns, 0 * k - 1, None))
    # the repeat lengths' sum below, equal to and above the two read lengths
    k, rform, d, ns = cross(range(440, 840), range(7), range(4), (0, 1, 40))
    dmin = np.array([0, 0, 0, 1], np.int64)[d]
    dsec = np.array([1, 2, 3, 3], np.int64)[d]
    parts.append((k, dmin, dsec, 0 * k + 1, ns, 0 * k - 1, rform))
    # the pair's identity exactly at the thresholds and next to them: a threshold read with itself, and with an error-free mate
    t, mate, ns, dsec = cross(range(P - n_thr, P), (0, 1), (0, 1), (1, 2, 3))
    parts.append(((t, np.where(mate == 0, t, 0)), 0 * t, dsec, 0 * t + 1, ns, 0 * t - 1, None))
    out_i1, out_i2, cols, r1s, r2s = [], [], [[] for _ in range(6)], [], []
    for k, dmin, dsec, nb, ns, force, rform in parts:
        i1, i2 = k if isinstance(k, tuple) else _pick(k, P)  # two reads of the pool per index, or the two reads themselves
        m = pool["min_err"][i1] + pool["min_err"][i2]
        L1, L2 = pool["rl"][i1], pool["rl"][i2]
        if rform is None:
            r1, r2 = pool["rep"][i1], pool["rep"][i2]
        else:
            r1 = np.choose(rform, [L1 - 1, L1, L1 + 1, L1 // 3, 0 * L1 + 1, 0 * L1, 2 * L1])
            r2 = np.choose(rform, [L2, L2, L2, L2 // 3, 0 * L2, L2, 2 * L2])
        out_i1.append(i1); out_i2.append(i2); r1s.append(r1); r2s.append(r2)
        for c, v in enumerate((0 * i1 + 2, m + dmin, np.where(dsec == NONE, 2 * e + 1, m + dsec), nb, ns, force)):
            cols[c].append(v)
    return _pack_pairs(pool, np.concatenate(out_i1), np.concatenate(out_i2), [np.concatenate(c) for c in cols], e, "paired_e%d" % e, mm.PAIRED,
                       np.concatenate(r1s), np.concatenate(r2s))


# ---------------------------------------------------------------- split
def _split_rows(e, md, variants):
    offs = sorted({-2, -1, 0, 1, 2, e * 3 // 4, e * 3 // 4 + 1, md, md + 1}) + [NONE]
    L, ac, lc, off = cross((30, 51, 100, 150, 301), range(9), range(7), offs)
    al = np.choose(ac, [L - e - 1, L - e, L - e + 1, L // 3 - 1, L // 3, L // 3 + 1, L, 0 * L + 49, 0 * L + 50])
    aligned = np.choose(lc, [al + 2, al, al - 1, al * 97 // 100, al * 95 // 100, al * 999 // 1000, al // 2])
    keep = (al >= 1) & (aligned >= 1)
    L, al, aligned, off = (v[keep] for v in (L, al, aligned, off))
    L, al, aligned, off = (np.repeat(v, variants) for v in (L, al, aligned, off))
    idx = np.arange(len(L), dtype=np.int64)
    h = (idx * 2654435761 + 12345) % (1 << 32)  # the other arguments: digits of a scrambled index
    err = -aligned
    second = np.where(off == NONE, e + 1, err + off)
    diff = np.minimum(second, err + md) - err   # what the function's diff will be when at most one best mapping exists
    d = np.maximum(np.abs(diff), 1)
    nb = np.array([0, 1, 1, 1, 2], np.int64)[h % 5]; h = h // 5
    ns = np.choose(h % 8, [0 * d, 0 * d + 1, d - 1, d, d + 1, 2 * d, 5 * d, 0 * d + 1000]); h = h // 8
    rep = np.choose(h % 9, [0 * L, 0 * L + 1, al - 1, al, al + 1, L - 1, L, 2 * L, L // 3]); h = h // 9
    nc = np.array([0, 4, 5, 9, 10, 50, 1000, 1 << 20], np.int64)[h % 8]
    # the reference would divide by num_second_best_mappings / diff + 1 == 0: left out (for the uncapped second as well: more than
    # one best mapping keeps it)
    bad = np.zeros(len(L), bool)
    for df in (diff, second - err):
        bad |= (df < 0) & (ns // np.maximum(-df, 1) == 1)
    ok = ~bad
    return dict(err=err[ok], al=al[ok], rl=L[ok], md=md, second=second[ok], n_best=nb[ok], n_second=ns[ok], rep=np.maximum(rep, 0)[ok],
                ncand=nc[ok])


def _split_groups(e):
    rows = [_split_rows(e, 2, 16), _split_rows(e, e, 16)]
    single = _pack_single(rows, e, "split_e%d" % e, mm.SPLIT)
    pool = dict(rows[0])  # the pair form calls the single form with max_num_error_difference 2
    pool["min_err"] = pool["err"]
    P = len(pool["err"])
    k = np.arange(40000, dtype=np.int64)
    i1, i2 = _pick(k, P)
    pair = _pack_pairs(pool, i1, i2, [0 * k + 2, 0 * k, 0 * k, 0 * k + 1, 0 * k, 0 * k - 1], e, "split_pair_e%d" % e, mm.PAIRED_SPLIT)
    return [single, pair]


# the groups' names, in order, without building them (the tests' parameters)
GROUP_NAMES = tuple(["single_e%d" % e for e in (3, 8, 12, 15)] + ["paired_e8"] +
                    [n % e for e in (2, 4, 6, 8, 12, 15) for n in ("split_e%d", "split_pair_e%d")])


def groups():
    global _GROUPS
    if _GROUPS is None:
        g = [_single_group(e, 4 if e == 8 else 1) for e in (3, 8, 12, 15)]
        g += [_paired_group(e) for e in (8,)]
        for e in (2, 4, 6, 8, 12, 15):
            g += _split_groups(e)
        assert sum(x.pairs.shape[1] for x in g) <= MAX_CASES and tuple(x.name for x in g) == GROUP_NAMES
        for x in g:
            x.reads.setflags(write=False)
            x.pairs.setflags(write=False)
        _GROUPS = g
    return _GROUPS


_RESULTS = None


def model_results():
    """[(mapq uint8 [n], tags) per group]: the model on every case, computed once for all tests"""
    global _RESULTS
    if _RESULTS is None:
        _RESULTS = [mm.model(g.kind, g.e, g.reads, g.pairs) for g in groups()]
        for q, t in _RESULTS:
            q.setflags(write=False)
            t.setflags(write=False)
    return _RESULTS


def describe(group, i):
    """the arguments of case i of a group, for a failure message"""
    r = {c: (int(group.reads[k, 2 * i]), int(group.reads[k, 2 * i + 1])) for k, c in enumerate(mm.READ_COLS)}
    p = {c: int(group.pairs[k, i]) for k, c in enumerate(mm.PAIR_COLS)}
    return "%s case %d (kind %s, e %d): reads (read 1, read 2) %s, pair %s" % (group.name, i, mm.KIND_NAMES[group.kind], group.e, r, p)


def first_difference(group, tags, results):
    """None, or a message naming the first case on which the results differ: its arguments, every result, the model's branches"""
    bad = np.zeros(group.pairs.shape[1], bool)
    ref = next(iter(results.values()))
    for v in results.values():
        bad |= v != ref
    if not bad.any():
        return None
    i = int(np.flatnonzero(bad)[0])
    return "%d of %d cases differ; first: %s; results %s; branches %s" % (
        int(bad.sum()), len(bad), describe(group, i), {k: int(v[i]) for k, v in results.items()}, mm.names(tags, i))
