"""Small adversarial datasets for oracle-vs-device fuzzing (no reference needed: the oracle is
pinned by tests/test_oracle_golden.py).  Heavy repeat content pushes the code through the
paths typical data rarely reaches: seed-frequency caps (F0/F1, second round), long hit lists
(heap sort), many candidates per strand (lane-grouped verification with threshold break),
mate rescue with many windows, multi-mappers (reservoir sampling), chromosome edges."""
import os

import numpy as np

import plain_align as pa

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.zeros(256, dtype=np.uint8)
for a, b in zip(b"ACGTN", b"TGCAN"):
    COMP[a] = b


def _gapped_read(rng, src, n, e, budget_p, len_p):
    """n bases of src under an edit script of tests/plain_align.py (substitutions, insertions and deletions of 1 .. e bases,
    three gaps in ten in the first or last 3 bases), with a budget of 1 .. e + 2 edits.  src is longer than n so that deletions
    do not shorten the read; where the chromosome ends first, the deletions are left out.  Returns (read, applied script)."""
    script = pa.edit_script(rng, n, e, pa.geometric(rng, budget_p, e + 2), 0.3, len_p)
    if len(src) < n + sum(ln for k, _, ln in script if k == "d"):
        script = [x for x in script if x[0] != "d"]
    return pa.apply_script(rng, src, n, script)


def make_case(seed, **kw):
    return _make_case(seed, **kw)[:3]


def make_case_with_truth(seed, **kw):
    """(chroms, r1, r2, truth); truth[i] = {"chr", "start", "end" (the fragment), "scripts": (script of r1[i], of r2[i]), "where": ((first base, one past the last,
    strand) of r1[i] on the chromosome, of r2[i])}: a script is the list of (kind, read position, length) edits that were applied, empty for a read without one"""
    return _make_case(seed, **kw)


def _make_case(seed, genome=120_000, n_chr=3, elem_len=400, copies=700, div=0.01, pairs=3000, L=50, tandem=True,
               gap_share=0.0, gap_e=0, gap_budget_p=1.0, gap_len_p=1.0, edge_share=0.05):
    """gap_share > 0 turns the gapped reads on (off, not one more number is drawn and the data is what it always was): that
    share of the reads carries an edit script for error threshold gap_e; gap_budget_p / gap_len_p: ratio between the
    probabilities of neighbouring budgets (1 .. e + 2) / gap lengths (1 .. e), 1 = uniform; three read-1 lengths in ten come from the
    word-boundary set (those of its members between 28 and L; the others keep the generator's own lengths); edge fragments lie anywhere within a read length of the chromosome end."""
    rng = np.random.default_rng(seed)
    gaps = gap_share > 0
    truth = []
    lens = [genome // n_chr] * n_chr
    chroms = [ACGT[rng.integers(0, 4, size=l)].copy() for l in lens]
    elem = ACGT[rng.integers(0, 4, size=elem_len)]
    for _ in range(copies):
        c = chroms[rng.integers(0, n_chr)]
        p = rng.integers(0, len(c) - elem_len)
        cp = elem.copy()
        m = rng.random(elem_len) < div
        cp[m] = ACGT[rng.integers(0, 4, size=int(m.sum()))]
        if rng.random() < 0.5:
            cp = COMP[cp[::-1]]
        c[p:p + elem_len] = cp
    if tandem:
        c = chroms[0]
        unit = ACGT[rng.integers(0, 4, size=23)]
        c[1000:1000 + 23 * 120] = np.tile(unit, 120)
        c[5000:5300] = ord("A")
        c[7000:7040] = ord("N")
    r1, r2 = [], []
    for i in range(pairs):
        ci = int(rng.integers(0, n_chr))
        c = chroms[ci]
        fl = int(rng.integers(35, 500))
        u = rng.random()
        if u < edge_share:
            st = 0 if rng.random() < 0.5 else len(c) - fl
            jit = int(rng.integers(-10, 10))
            if gaps:
                jit = int(rng.integers(0, L)) * (1 if st == 0 else -1)
            st = int(min(max(0, st + jit), len(c) - fl))
        else:
            st = int(rng.integers(0, len(c) - fl))
        frag = c[st:st + fl]
        a = frag[:L].copy()
        b = COMP[frag[::-1]][:L].copy()
        sa = sb = ()
        ia, ib = (st, st + len(a), 0), (st + fl - len(b), st + fl, 1)  # (first base, one past the last, strand) on the chromosome
        if gaps:
            slack = gap_e * (gap_e + 2) + 1
            if rng.random() < gap_share:
                a, sa = _gapped_read(rng, c[st:st + len(a) + slack], len(a), gap_e, gap_budget_p, gap_len_p)
            if rng.random() < gap_share:
                b, sb = _gapped_read(rng, COMP[c[max(0, st + fl - len(b) - slack):st + fl][::-1]], len(b), gap_e, gap_budget_p, gap_len_p)
        for x, sx in ((a, sa), (b, sb)):
            if sx:
                continue  # a scripted read has its substitutions in the script
            m = rng.random(len(x)) < 0.015
            x[m] = ACGT[rng.integers(0, 4, size=int(m.sum()))]
        if rng.random() < 0.03:
            a[rng.integers(0, len(a))] = ord("N")
        if rng.random() < 0.5:
            a, b = b, a
            sa, sb = sb, sa
            ia, ib = ib, ia
        l1 = int(rng.integers(28, L + 1)) if rng.random() < 0.1 else len(a)
        if gaps and rng.random() < 0.3:
            fit = [w for w in pa.WORD_LENGTHS if 28 <= w <= len(a)]
            if fit:
                l1 = fit[int(rng.integers(0, len(fit)))]
        if gaps:
            if ia[2] == 0:  # read 1 keeps its first l1 bases: the front of a + read, the far end of a - read
                ia = (ia[0], ia[0] + l1, 0)
            else:
                ia = (ia[1] - l1, ia[1], 1)
            truth.append({"chr": ci, "start": st, "end": st + fl, "scripts": (tuple(x for x in sa if x[1] < l1), tuple(sb)), "where": (ia, ib)})
        r1.append(a[:l1].tobytes())
        r2.append(b.tobytes())
    return chroms, r1, r2, truth


def write_case(d, seed, **kw):
    os.makedirs(d, exist_ok=True)
    chroms, r1, r2 = make_case(seed, **kw)
    fa = os.path.join(d, "f.fa")
    with open(fa, "wb") as f:
        for i, c in enumerate(chroms):
            f.write(b">c%d\n" % i + c.tobytes() + b"\n")

    def pack(rs):
        off = np.zeros(len(rs) + 1, np.uint32)
        off[1:] = np.cumsum([len(r) for r in rs])
        return np.frombuffer(b"".join(rs), np.uint8).copy(), off
    b1, o1 = pack(r1)
    b2, o2 = pack(r2)
    return fa, b1, o1, b2, o2


GAPS = {"gap_share": 0.7, "gap_budget_p": 0.5, "gap_len_p": 0.6, "edge_share": 0.05}

CONFIGS = [
    # (seed, preset, param overrides, generator overrides)
    (1, "atac", {"mapq_threshold": 0}, {}),
    (2, "chip", {"mapq_threshold": 0}, {"copies": 1200, "elem_len": 200}),
    (3, "atac", {"mapq_threshold": 0, "max_seed_freq0": 40, "max_seed_freq1": 90}, {"copies": 300}),
    (4, "hic", {"mapq_threshold": 0}, {"L": 100, "copies": 200}),
    (5, None, {"mapq_threshold": 0, "error_threshold": 5}, {"L": 70}),
    (6, "chip", {"mapq_threshold": 0, "min_num_seeds": 3, "max_insert_size": 300}, {"div": 0.0, "copies": 150}),
    # gap-rich reads (gap runs of 2 and more bases, gaps in a read's first and last bases, edit sums at the threshold, gapped reads at
    # chromosome ends); tests/test_fuzz_gaps.py keeps them so.  Appended: the slices [:2] and [:4] other tests take stay what they are.
    (7, "chip", {"mapq_threshold": 0, "error_threshold": 8}, {"L": 100, "gap_e": 8, **GAPS}),
    (8, "hic", {"mapq_threshold": 0}, {"L": 100, "gap_e": 4, **GAPS}),
    (9, None, {"mapq_threshold": 0, "error_threshold": 15}, {"L": 150, "gap_e": 15, **GAPS, "gap_budget_p": 0.8, "gap_len_p": 0.8}),
    (10, "atac", {"mapq_threshold": 0, "error_threshold": 1}, {"L": 36, "gap_e": 1, **GAPS}),
]
GAP_CONFIGS = CONFIGS[6:]


def write_wrap_case(d):
    """a repeat element that also stands at the very start of every chromosome, and reads that carry 15 foreign bases in front of the
    element's first 35: the + hit at position 0 has its diagonal before the sequence start (candidate position wraps below zero)"""
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(77)
    elem = ACGT[rng.integers(0, 4, 300)]
    chroms = [ACGT[rng.integers(0, 4, 40000)].copy() for _ in range(3)]
    for c in chroms:
        c[:300] = elem
        for _ in range(40):
            p = int(rng.integers(400, len(c) - 400))
            c[p:p + 300] = elem
    fa = os.path.join(d, "w.fa")
    with open(fa, "wb") as f:
        for i, c in enumerate(chroms):
            f.write(b">c%d\n" % i + c.tobytes() + b"\n")
    r1, r2 = [], []
    for i in range(300):
        a = np.concatenate([ACGT[rng.integers(0, 4, 15)], elem[:35]])
        b = COMP[chroms[i % 3][0:260][::-1]][:50]
        r1.append(a.tobytes())
        r2.append(b.tobytes())

    def pack(rs):
        off = np.zeros(len(rs) + 1, np.uint32)
        off[1:] = np.cumsum([len(r) for r in rs])
        return np.frombuffer(b"".join(rs), np.uint8).copy(), off
    b1, o1 = pack(r1)
    b2, o2 = pack(r2)
    return fa, b1, o1, b2, o2
