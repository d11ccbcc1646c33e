"""The MAPQ functions on their own, without a GPU: the plain model of the reference's arithmetic (tests/mapq_model.py), the product's
stage functions on the host (cm_mapq_single / _single_split / _paired / _paired_split of chromap_amd/csrc/cm_stages.h through
hostemu_mapq_batch) and the oracle's (ora_mapq_batch) on the cases of tests/mapq_cases.py; the cases' own coverage; the two host-built
tables of cm_mapq_tables.h against 60-digit arithmetic; the model against the MAPQ of real mapped records; and the cases under the
sanitizers in a stand-alone program.  No tolerance anywhere: any difference is a defect.  tests/test_gpu_mapq.py runs the same cases
through the device."""
import math
import subprocess

import numpy as np
import pytest

import datasets
import hostemu_valu_lib as hv
import mapq_cases as mc
import mapq_model as mm
import oracle_lib as ol

MIN_PER_BRANCH = 100
# GetMAPQForSingleEndRead's "mapq > 60" cannot be reached at max_num_error_difference 2, the value GetMAPQForPairedEndRead passes: the
# length coefficient and the identity are at most 1, so the value is at most (int)(5 * 6.02 * 2 + 0.499) = 60
UNREACHABLE = {mm.PAIRED: {"s.cut60", "r2.s.cut60"}, mm.PAIRED_SPLIT: {"s.cut60", "r2.s.cut60"}}


# ---------------------------------------------------------------- the three implementations
@pytest.mark.parametrize("name", mc.GROUP_NAMES)
def test_model_host_and_oracle_agree(name):
    gi = mc.GROUP_NAMES.index(name)
    g = mc.groups()[gi]
    q, tags = mc.model_results()[gi]
    results = {"model": q, "host": hv.mapq_batch(g.kind, g.e, g.reads, g.pairs), "oracle": ol.mapq_batch(g.kind, g.e, g.reads, g.pairs)}
    assert mc.first_difference(g, tags, results) is None, mc.first_difference(g, tags, results)


# ---------------------------------------------------------------- the cases themselves
def test_case_count_and_determinism():
    total = sum(g.pairs.shape[1] for g in mc.groups())
    print("cases: %d" % total)
    assert 0 < total <= mc.MAX_CASES
    saved, mc._GROUPS = mc._GROUPS, None
    try:
        again = mc.groups()
    finally:
        mc._GROUPS = saved
    for a, b in zip(saved, again):
        assert a.name == b.name and np.array_equal(a.reads, b.reads) and np.array_equal(a.pairs, b.pairs)


def test_every_branch_is_taken():
    for kind in (mm.SINGLE, mm.SPLIT, mm.PAIRED, mm.PAIRED_SPLIT):
        counts = {b: 0 for b in mm.branches_of(kind)}
        for g, (_, tags) in zip(mc.groups(), mc.model_results()):
            if g.kind == kind:
                for b in counts:
                    counts[b] += mm.count(tags, b)
        print("%s: %s" % (mm.KIND_NAMES[kind], counts))
        low = {b: c for b, c in counts.items() if c < MIN_PER_BRANCH and b not in UNREACHABLE.get(kind, ())}
        assert not low, "%s: branches with fewer than %d cases: %s" % (mm.KIND_NAMES[kind], MIN_PER_BRANCH, low)
        for b in UNREACHABLE.get(kind, ()):
            assert counts[b] == 0


def test_every_breakpoint_and_its_neighbours_occur():
    brk = mc.breakpoints()
    assert len(brk) == 94 and brk[-1] == 1778207635
    want = {v for b in brk for v in (b - 1, b, b + 1)}
    single = set()
    paired = set()
    for g in mc.groups():
        if g.kind == mm.SINGLE:
            single.update(np.unique(g.reads[6, 0::2]).tolist())
        if g.kind == mm.PAIRED:
            paired.update(np.unique(g.pairs[4]).tolist())
    assert want <= single and want <= paired


def test_all_identity_threshold_pairs_occur():
    tp = mc.threshold_pairs()
    assert len(tp) == len(set(tp)) == 35
    for err, length in tp:
        assert err <= 15 and (err * 20 == length or err * 100 == 3 * length or err * 1000 == length)
    have = set()
    for g in mc.groups():
        if g.kind == mm.SINGLE:
            L = np.maximum(g.reads[1, 0::2], g.reads[2, 0::2])
            rep = g.reads[7, 0::2] > 0  # the thresholds matter in the repeat block only
            have.update(zip(g.reads[0, 0::2][rep].tolist(), L[rep].tolist()))
    for err, length in tp:
        for d in (-1, 0, 1):
            assert (err, length + d) in have, (err, length + d)


def test_value_sets():
    values = {k: set() for k in range(4)}
    for g, (q, _) in zip(mc.groups(), mc.model_results()):
        values[g.kind].update(np.unique(q).tolist())
    for k in range(4):
        print("%s yields %s" % (mm.KIND_NAMES[k], sorted(values[k])))
    assert values[mm.SINGLE] == set(range(61))
    for k in (mm.SPLIT, mm.PAIRED, mm.PAIRED_SPLIT):
        assert {0, 60} <= values[k]


def test_left_out_cases_stay_out():
    for g in mc.groups():
        split = g.kind in (mm.SPLIT, mm.PAIRED_SPLIT)
        used = slice(0, None, 2) if g.kind in (mm.SINGLE, mm.SPLIT) else slice(None)
        al, rl = g.reads[1, used].astype(np.int64), g.reads[2, used].astype(np.int64)
        assert (rl >= 1).all() and (al >= 1).all() and (al <= 65535).all()
        if not split:
            assert (rl <= 65535).all()


# ---------------------------------------------------------------- the tables of cm_mapq_tables.h
def test_breakpoint_table_is_the_true_one():
    import mpmath
    mp = mpmath.mp
    mp.dps = 60
    a, b = mpmath.mpf(4.343), mpmath.mpf(0.499)  # the doubles the reference's constants are

    def f(n):
        return int(mpmath.floor(a * mpmath.log(n + 1) + b))
    _, brk = hv.mapq_tables()
    true = []
    margin = 1.0
    v = 0
    while f(0x7fffffff) >= v:
        n = max(1, int(mpmath.ceil(mpmath.exp((v - b) / a))) - 1)
        while n > 1 and f(n - 1) >= v:
            n -= 1
        while f(n) < v:
            n += 1
        true.append(n)
        for m in (n - 1, n):
            if m >= 1:
                x = a * mpmath.log(m + 1) + b
                margin = min(margin, float(abs(x - mpmath.nint(x)) / x))
        v += 1
    print("breakpoints: %d, closest relative approach to an integer %.3g" % (len(true), margin))
    assert brk.tolist() == true == mc.breakpoints()
    assert margin > 1e-13  # far above the error of a double log(): libm cannot move a breakpoint


def test_len_coef_table():
    import mpmath
    mpmath.mp.dps = 60
    coef, _ = hv.mapq_tables()
    assert coef.shape == (65536,)
    assert (coef[:50] == 1.0).all()
    want = np.array([3 / math.log(a) for a in range(50, 65536)])
    assert np.array_equal(coef[50:].view(np.uint64), want.view(np.uint64))  # bit for bit
    assert np.array_equal(coef.view(np.uint64), mm.len_coef_table().view(np.uint64))
    worst = 0.0
    for a in range(50, 65536):
        t = 3 / mpmath.log(a)
        worst = max(worst, float(abs(mpmath.mpf(float(coef[a])) - t) / mpmath.mpf(float(np.spacing(coef[a])))))
    print("len_coef: largest distance to the 60-digit value %.3f ulp" % worst)
    assert worst <= 2.0  # libm's log() under 1 ulp, the division half an ulp


# ---------------------------------------------------------------- the model on real runs
@pytest.mark.parametrize("case", ["p1_e12_chip_q0", "p1_e5_atac"])
def test_model_gives_the_mapq_of_mapped_records(case):
    meta = datasets.case_meta(case)
    fa, r1, r2 = datasets.case_inputs(case)
    preset, kw = datasets.flags_to_params(meta["chromap_flags"])
    kw["mapq_threshold"] = 0
    p = ol.params(preset, **kw)
    o = ol.Oracle(datasets.case_index(case), fa, p)
    try:
        b1, o1 = ol.read_fastx(r1)
        b2, o2 = ol.read_fastx(r2)
        rec, k, _, tr = o.map_pairs(b1, o1, b2, o2, trace=True)
        rec = np.frombuffer(rec, dtype=np.dtype([("read_id", "<u4"), ("rid", "<u4"), ("start", "<u4"), ("flen", "<u2"), ("mapq", "u1"),
                                                ("dir", "u1"), ("uniq", "u1"), ("dups", "u1"), ("pos_al", "<u2"), ("neg_al", "<u2")], align=True))[:k]
        t = np.frombuffer(tr, dtype=np.dtype([(n, "<u4") for n in ("len1", "len2", "n_mm1", "n_mm2", "n_cand1", "n_cand2", "n_draft1", "n_draft2")] +
                                             [(n, "<i4") for n in ("min_err1", "min_err2", "nbest1", "nbest2", "second1", "second2", "nsecond1",
                                                                   "nsecond2")] + [("rep1", "<u4"), ("rep2", "<u4")] +
                                             [(n, "<i4") for n in ("min_sum", "nbest", "second_sum", "nsecond", "force_mapq")]))
    finally:
        o.close()
    assert p.max_num_best_mappings == 1 and not p.split_alignment
    t = t[rec["read_id"]]
    sel = t["min_sum"] == t["min_err1"] + t["min_err2"]  # then the reported mappings are each read's best: their errors are known
    rec, t = rec[sel], t[sel]
    n = len(rec)
    print("%s: %d of %d records have min_sum == min_err1 + min_err2" % (case, n, k))
    assert n >= 0.95 * k
    reads = np.zeros((9, 2 * n), np.int32)
    plus1 = rec["dir"] == 1  # read 1 is the + strand read
    for m, s in ((0, "1"), (1, "2")):
        reads[0, m::2] = t["min_err" + s]
        reads[2, m::2] = t["len" + s]
        reads[3, m::2] = t["min_err" + s]
        reads[4, m::2] = t["second" + s]
        reads[5, m::2] = t["nbest" + s]
        reads[6, m::2] = t["nsecond" + s]
        reads[7, m::2] = t["rep" + s]
    reads[1, 0::2] = np.where(plus1, rec["pos_al"], rec["neg_al"])
    reads[1, 1::2] = np.where(plus1, rec["neg_al"], rec["pos_al"])
    pairs = np.stack([np.full(n, 2), t["min_sum"], t["second_sum"], t["nbest"], t["nsecond"], t["force_mapq"]]).astype(np.int32)
    q, tags = mm.model(mm.PAIRED, p.error_threshold, reads, pairs)
    g = mc.Group(case, mm.PAIRED, p.error_threshold, reads, pairs)
    msg = mc.first_difference(g, tags, {"model": q & 63, "record": rec["mapq"]})
    assert msg is None, msg


# ---------------------------------------------------------------- sanitizers
def test_cases_under_sanitizers(tmp_path):
    """every case through the host functions in a stand-alone program built with AddressSanitizer, UndefinedBehaviorSanitizer and the
    float-cast check: a clean run shows that the case set stays inside defined behaviour"""
    path = tmp_path / "mapq_cases.bin"
    with open(path, "wb") as f:
        f.write(np.int64(len(mc.groups())).tobytes())
        for g, (q, _) in zip(mc.groups(), mc.model_results()):
            f.write(np.array([g.kind, g.e, g.pairs.shape[1]], np.int64).tobytes())
            f.write(np.ascontiguousarray(g.reads).tobytes())
            f.write(np.ascontiguousarray(g.pairs).tobytes())
            f.write(q.tobytes())
    r = subprocess.run([hv.mapq_sanitizer_program(), str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    total = sum(g.pairs.shape[1] for g in mc.groups())
    assert r.returncode == 0 and "mapq: %d cases equal" % total in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]
