"""A plain model of the reference's MAPQ arithmetic: GetMAPQForSingleEndRead and GetMAPQForPairedEndRead
(mapping_generator.h:920-1192 of chromap v0.3.3), with and without split_alignment.  Written from those lines, statement by statement
and in their operation order, in numpy on float64 -- not from chromap_amd/csrc/cm_stages.h, which it checks (tests/test_mapq_cpu.py,
tests/test_gpu_mapq.py).

  * every log() is math.log (the values needed are few: 65 535 lengths, a few hundred counts; they are looked up per case)
  * a double converted to an integer is truncated; a value stored into the reference's uint8_t is reduced to 8 bits where the
    reference stores it (mapq_pe, the final casts)
  * the split tail's integer divisions truncate as C's do; num_candidates / 5 / diff is done in 32-bit unsigned arithmetic as the
    usual arithmetic conversions make it (num_candidates is a uint32_t)

The arguments are the two case matrices of cmgpu_debug_mapq (include/chromap_amd_debug.h; chromap_amd._capi.MAPQ_READ_COLS /
MAPQ_PAIR_COLS): reads int32 [9, 2 n], pairs int32 [6, n]; case i is pair i, reads 2 i and 2 i + 1.  model() returns the MAPQ byte of
every case and bit masks of the branches it took (TAGS; names(tags, i) spells case i's out, count(tags, name) counts a branch)."""
import math

import numpy as np

SINGLE, SPLIT, PAIRED, PAIRED_SPLIT = 0, 1, 2, 3
KIND_NAMES = ("single", "split", "paired", "paired_split")
READ_COLS = ("num_errors", "alignment_length", "read_length", "min_err", "second_err", "n_best", "n_second", "rep_len", "strand_ncand")
PAIR_COLS = ("max_diff", "min_sum", "second_sum", "n_best", "n_second", "force_mapq")

# ---- branch tags.  s.*: GetMAPQForSingleEndRead (read 1 of the case; r2.* the same for read 2 of a pair), x.*: its split_alignment
# parts, p.*: GetMAPQForPairedEndRead.  Every condition and every conditional expression of the three functions has a tag per
# outcome (s.al_longer / s.al_not_longer: the maximum of :927-930, which the split form does not take).
SINGLE_TAGS = ("al_longer", "al_not_longer", "nbest_gt1", "nbest_le1", "second_capped", "second_kept", "len_lt50", "len_ge50", "nsec_pos", "nsec_zero", "cut60", "cut0",
               "uncut", "rep_zero", "rep_full", "rep_part", "id_le95", "id_le97", "id_ge999", "id_mid")
SPLIT_TAGS = ("id_capped", "id_kept", "tail", "no_tail_len", "no_tail_same", "third_rule", "third_kept", "cand_sub", "cand_kept", "below0",
              "not_below0", "div", "no_div")
PAIRED_TAGS = ("nbest_le1", "nbest_gt1", "adj_second", "adj_unpaired", "raw_wrap", "raw_fits", "nsec_pos", "nsec_zero", "pen_wrap",
               "pen_fits", "cut60", "uncut", "rep_zero", "rep_full", "rep_part", "max1_read", "max1_al", "max2_read", "max2_al", "id_is_1", "id_is_2",
               "id_le95", "id_le97", "id_ge999", "id_mid",
               "mix1_own", "mix1_pe", "mix1_mix", "mix2_own", "mix2_pe", "mix2_mix", "x12_cut1", "x12_kept1", "x12_cut2", "x12_kept2",
               "min_is_1", "min_is_2", "force_applied", "force_not")
TAGS = {}
for _p, _l in (("s.", SINGLE_TAGS), ("x.", SPLIT_TAGS), ("r2.s.", SINGLE_TAGS), ("r2.x.", SPLIT_TAGS), ("p.", PAIRED_TAGS)):
    for _t in _l:
        TAGS[_p + _t] = (len(TAGS) // 62, 1 << (len(TAGS) % 62))  # (word, bit) of the [TAG_WORDS, n] int64 tag array
TAG_WORDS = (len(TAGS) + 61) // 62


def names(tags, i):
    """the branches case i took"""
    return [k for k, (w, b) in TAGS.items() if int(tags[w, i]) & b]


def count(tags, name):
    """how many cases took branch `name`"""
    w, b = TAGS[name]
    return int(np.count_nonzero(tags[w] & b))


# the branches each kind's cases must reach (tests/test_mapq_cpu.py)
def branches_of(kind):
    s = ["s." + t for t in SINGLE_TAGS if kind in (SINGLE, PAIRED) or not t.startswith("al_")]
    x = ["x." + t for t in SPLIT_TAGS]
    x12 = ["p." + t for t in ("x12_cut1", "x12_kept1", "x12_cut2", "x12_kept2", "min_is_1", "min_is_2")]
    if kind == SINGLE:
        return s
    if kind == SPLIT:
        return s + x
    if kind == PAIRED:
        return ["p." + t for t in PAIRED_TAGS] + s + ["r2." + t for t in s]
    return x12 + s + x + ["r2." + t for t in s + x]


_LOG = None
_COEF = None


def len_coef_table():
    """mapping_generator.h:924-925, 958-960 for every 16-bit alignment length: a < 50 ? 1.0 : (int)log(50) / log(a)"""
    global _COEF
    if _COEF is None:
        frac = int(math.log(50))
        _COEF = np.array([1.0 if a < 50 else frac / math.log(a) for a in range(65536)], np.float64)
    return _COEF


def nsec_penalty(n_second):
    """(int)(4.343 * log(num_second_best_mappings + 1) + 0.499), per element (:966-967, :1094-1097); 0 where it is not applied"""
    n_second = np.asarray(n_second, np.int64)
    u, inv = np.unique(n_second, return_inverse=True)
    pen = np.array([int(4.343 * math.log(int(v) + 1) + 0.499) if v > 0 else 0 for v in u], np.int64)
    return pen[inv]


def _trunc(x):
    return np.trunc(x).astype(np.int64)


def _cdiv(a, b):
    """C's integer division (truncation toward zero); b != 0"""
    q = np.abs(a) // np.abs(b)
    return np.where((a < 0) != (b < 0), -q, q)


def _set(tags, prefix, name, mask):
    w, b = TAGS[prefix + name]
    tags[w] |= np.where(mask, b, 0).astype(np.int64)


def _id_branches(tags, prefix, on, ident, frac, mapq):
    """:983-991 / :1135-1144: the four identity branches of the repeat block; mapq as float64-exact integers"""
    b95 = on & (ident <= 0.95)
    b97 = on & ~b95 & (ident <= 0.97)
    b999 = on & ~b95 & ~b97 & (ident >= 0.999)
    mid = on & ~b95 & ~b97 & ~b999
    _set(tags, prefix, "id_le95", b95); _set(tags, prefix, "id_le97", b97); _set(tags, prefix, "id_ge999", b999); _set(tags, prefix, "id_mid", mid)
    m = mapq.astype(np.float64)
    out = mapq.copy()
    out = np.where(b95, _trunc(m * (1 - np.sqrt(frac)) + 0.499), out)
    out = np.where(b97, _trunc(m * (1 - frac) + 0.499), out)
    out = np.where(b999, _trunc(m * (1 - frac * frac * frac * frac) + 0.499), out)
    out = np.where(mid, _trunc(m * (1 - frac * frac) + 0.499), out)
    return out


def single_end(split, e, err, al, rl, max_diff, second, n_best, n_second, rep, ncand, tags, prefix=""):
    """GetMAPQForSingleEndRead (:920-1022); returns the uint8_t it returns, as int64"""
    sp, xp = prefix + "s.", prefix + "x."
    err, rl, max_diff, second, n_best, n_second = (np.asarray(v, np.int64) for v in (err, rl, max_diff, second, n_best, n_second))
    al = np.asarray(al, np.int64) & 0xffff          # uint16_t alignment_length
    rep = np.asarray(rep, np.int64) & 0xffffffff    # uint32_t repetitive_seed_length_
    ncand = np.asarray(ncand, np.int64) & 0xffffffff
    if not split:                                   # :927-930
        longer = al > rl
        _set(tags, sp, "al_longer", longer); _set(tags, sp, "al_not_longer", ~longer)
        al = np.where(longer, al, rl & 0xffff)
    alf = al.astype(np.float64)
    ident = 1 - err.astype(np.float64) / alf        # :932
    if split:                                       # :934-937
        ident = (-err).astype(np.float64) / alf
        capped = ident > 1
        _set(tags, xp, "id_capped", capped); _set(tags, xp, "id_kept", ~capped)
        ident = np.where(capped, 1.0, ident)
    le1 = ~(n_best > 1)                             # :942, :953
    _set(tags, sp, "nbest_gt1", ~le1); _set(tags, sp, "nbest_le1", le1)
    cap = le1 & (second > err + max_diff)           # :954-956
    _set(tags, sp, "second_capped", cap); _set(tags, sp, "second_kept", le1 & ~cap)
    sec = np.where(cap, err + max_diff, second)
    _set(tags, sp, "len_lt50", le1 & (al < 50)); _set(tags, sp, "len_ge50", le1 & (al >= 50))
    tmp = len_coef_table()[al]                      # :958-960
    tmp = tmp * (ident * ident)                     # :961
    mapq = np.where(le1, _trunc(5 * 6.02 * (sec - err).astype(np.float64) * tmp * tmp + 0.499), 0)  # :962
    pos = n_second > 0                              # :965-968
    _set(tags, sp, "nsec_pos", pos); _set(tags, sp, "nsec_zero", ~pos)
    mapq = mapq - np.where(pos, nsec_penalty(np.where(pos, n_second, 0)), 0)
    hi, lo = mapq > 60, mapq < 0                    # :970-975
    _set(tags, sp, "cut60", hi); _set(tags, sp, "cut0", lo); _set(tags, sp, "uncut", ~hi & ~lo)
    mapq = np.clip(mapq, 0, 60)
    on = rep > 0                                    # :977-992
    full = on & (rep >= (rl & 0xffffffff))
    _set(tags, sp, "rep_zero", ~on); _set(tags, sp, "rep_full", full); _set(tags, sp, "rep_part", on & ~full)
    frac = np.where(full, 0.999, rep.astype(np.float64) / rl.astype(np.float64))
    mapq = _id_branches(tags, sp, on, ident, frac, mapq)
    if split:                                       # :994-1019
        short = al < rl - e
        tail = short & (sec != err)
        _set(tags, xp, "tail", tail); _set(tags, xp, "no_tail_len", ~short); _set(tags, xp, "no_tail_same", short & (sec == err))
        third = tail & (rep >= al) & (rep < (rl & 0xffffffff)) & (al < _cdiv(rl, np.int64(3)))
        _set(tags, xp, "third_rule", third); _set(tags, xp, "third_kept", tail & ~third)
        mapq = np.where(third, 0, mapq)
        diff = sec - err
        close = diff <= e * 3 // 4
        sub = tail & close & (ncand >= 5)
        _set(tags, xp, "cand_sub", sub); _set(tags, xp, "cand_kept", tail & ~sub)
        udiff = np.where(sub, diff & 0xffffffff, 1)  # the int diff converted to unsigned
        m32 = ((mapq & 0xffffffff) - (ncand // 5) // udiff) & 0xffffffff
        m32 = np.where(m32 >= 1 << 31, m32 - (1 << 32), m32)  # back into the int mapq
        mapq = np.where(sub, m32, mapq)
        neg = tail & (mapq < 0)
        _set(tags, xp, "below0", neg); _set(tags, xp, "not_below0", tail & ~neg)
        mapq = np.where(neg, 0, mapq)
        dv = tail & (n_second > 0) & close
        _set(tags, xp, "div", dv); _set(tags, xp, "no_div", tail & ~dv)
        divisor = np.where(dv, _cdiv(n_second, np.where(dv, diff, 1)) + 1, 1)
        if np.any(divisor == 0):
            raise ZeroDivisionError("num_second_best_mappings / diff + 1 == 0: the reference divides by zero")
        mapq = np.where(dv, _cdiv(mapq, divisor), mapq)
    return mapq & 0xff                              # :1021


def model(kind, e, reads, pairs):
    """(mapq uint8 [n], tags int64 [TAG_WORDS, n]) of the n cases"""
    reads = np.asarray(reads, np.int64)
    pairs = np.asarray(pairs, np.int64)
    n = pairs.shape[1]
    assert reads.shape == (9, 2 * n) and pairs.shape == (6, n)
    tags = np.zeros((TAG_WORDS, n), np.int64)
    R1 = {c: reads[k, 0::2] for k, c in enumerate(READ_COLS)}
    R2 = {c: reads[k, 1::2] for k, c in enumerate(READ_COLS)}
    P = {c: pairs[k] for k, c in enumerate(PAIR_COLS)}
    split = kind in (SPLIT, PAIRED_SPLIT)

    def se(R, max_diff, prefix):
        return single_end(split, e, R["num_errors"], R["alignment_length"], R["read_length"], max_diff, R["second_err"], R["n_best"],
                          R["n_second"], R["rep_len"], R["strand_ncand"], tags, prefix)

    if kind in (SINGLE, SPLIT):
        return se(R1, P["max_diff"], "").astype(np.uint8), tags
    mapq_pe = np.zeros(n, np.int64)                 # :1073
    if kind == PAIRED:
        min_unpaired = R1["min_err"] + R2["min_err"] + 3  # :1074-1075
        le1 = P["n_best"] <= 1                      # :1077
        _set(tags, "p.", "nbest_le1", le1); _set(tags, "p.", "nbest_gt1", ~le1)
        use2 = P["second_sum"] < min_unpaired       # :1078-1082
        _set(tags, "p.", "adj_second", le1 & use2); _set(tags, "p.", "adj_unpaired", le1 & ~use2)
        adj = np.where(use2, P["second_sum"], min_unpaired)
        raw = _trunc(5 * 6.02 * (adj - P["min_sum"]).astype(np.float64) / 1 + .499)  # :1024, :1084-1086: an int
        _set(tags, "p.", "raw_wrap", le1 & (raw != (raw & 0xff))); _set(tags, "p.", "raw_fits", le1 & (raw == (raw & 0xff)))
        pe = raw & 0xff                             # ... stored into the uint8_t
        pos = le1 & (P["n_second"] > 0)             # :1092-1098
        _set(tags, "p.", "nsec_pos", pos); _set(tags, "p.", "nsec_zero", le1 & ~pos)
        pen = np.where(pos, nsec_penalty(np.where(pos, P["n_second"], 0)), 0)
        _set(tags, "p.", "pen_wrap", pos & (pen > pe)); _set(tags, "p.", "pen_fits", pos & (pen <= pe))
        pe = (pe - pen) & 0xff                      # uint8_t -= int
        hi = pe > 60                                # :1100-1105 (an unsigned value is never < 0)
        _set(tags, "p.", "cut60", le1 & hi); _set(tags, "p.", "uncut", le1 & ~hi)
        pe = np.where(hi, 60, pe)
        rep = (R1["rep_len"] + R2["rep_len"]) & 0xffffffff  # :1111-1112
        rep = np.where(rep >= 1 << 31, rep - (1 << 32), rep)  # into the int
        on = le1 & (rep > 0)                        # :1114-1145
        total = (R1["read_length"] + R2["read_length"]).astype(np.float64)
        full = on & (rep.astype(np.float64) >= total)
        _set(tags, "p.", "rep_zero", le1 & ~on); _set(tags, "p.", "rep_full", full); _set(tags, "p.", "rep_part", on & ~full)
        frac = np.where(full, 0.999, rep.astype(np.float64) / total)
        al1, al2 = R1["alignment_length"] & 0xffff, R2["alignment_length"] & 0xffff
        rd1, rd2 = R1["read_length"] > al1, R2["read_length"] > al2  # :1121-1129
        _set(tags, "p.", "max1_read", on & rd1); _set(tags, "p.", "max1_al", on & ~rd1)
        _set(tags, "p.", "max2_read", on & rd2); _set(tags, "p.", "max2_al", on & ~rd2)
        id1 = 1 - R1["num_errors"].astype(np.float64) / np.where(rd1, R1["read_length"], al1).astype(np.float64)
        id2 = 1 - R2["num_errors"].astype(np.float64) / np.where(rd2, R2["read_length"], al2).astype(np.float64)
        first = id1 < id2                           # :1131-1133
        _set(tags, "p.", "id_is_1", on & first); _set(tags, "p.", "id_is_2", on & ~first)
        ident = np.where(first, id1, id2)
        pe = _id_branches(tags, "p.", on, ident, frac, pe) & 0xff
        mapq_pe = np.where(le1, pe, 0)
    two = np.full(n, 2, np.int64)
    mapq1 = se(R1, two, "")                         # :1148-1155
    mapq2 = se(R2, two, "r2.")
    if kind == PAIRED:                              # :1162-1169
        def mix(mq, which):
            own = mq > mapq_pe
            mixed = mq.astype(np.float64) + mapq_pe.astype(np.float64) * 0.65
            arm_pe = ~own & (mapq_pe.astype(np.float64) < mixed)
            _set(tags, "p.", which + "_own", own); _set(tags, "p.", which + "_pe", arm_pe); _set(tags, "p.", which + "_mix", ~own & ~arm_pe)
            return np.where(own, mq, np.where(arm_pe, mapq_pe, _trunc(mixed))) & 0xff
        mapq1 = mix(mapq1, "mix1")
        mapq2 = mix(mapq2, "mix2")
    mapq1 = _trunc(mapq1.astype(np.float64) * 1.2) & 0xff  # :1171-1179
    mapq2 = _trunc(mapq2.astype(np.float64) * 1.2) & 0xff
    _set(tags, "p.", "x12_cut1", mapq1 > 60); _set(tags, "p.", "x12_kept1", mapq1 <= 60)
    _set(tags, "p.", "x12_cut2", mapq2 > 60); _set(tags, "p.", "x12_kept2", mapq2 <= 60)
    mapq1 = np.minimum(mapq1, 60)
    mapq2 = np.minimum(mapq2, 60)
    first = mapq1 < mapq2                           # :1185
    _set(tags, "p.", "min_is_1", first); _set(tags, "p.", "min_is_2", ~first)
    mapq = np.where(first, mapq1, mapq2)
    if kind == PAIRED:                              # :1187-1189 (split alignment passes force_mapq = -1)
        f = (mapq < 60) & (P["force_mapq"] >= 0) & (P["force_mapq"] < mapq)
        _set(tags, "p.", "force_applied", f); _set(tags, "p.", "force_not", ~f)
        mapq = np.where(f, P["force_mapq"], mapq)
    return (mapq & 0xff).astype(np.uint8), tags
