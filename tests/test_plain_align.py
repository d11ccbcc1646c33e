"""The alignment primitives -- oracle (oracle/chromap_oracle.c) and product (cm_stages.h through the host emulation) -- against
the plain DP tables of tests/plain_align.py on gap-rich windows: gap runs of up to e bases, gaps in the first and last three
bases, edit budgets around e, N / lower case / IUPAC bytes on both sides, every word-boundary read length, every window offset
modulo 32, e at both ends of the accepted range.  Every comparison is exact."""
import ctypes as C
import functools

import numpy as np
import pytest

import hostemu_lib as hl
import oracle_lib as ol
import plain_align as pa

ES = (1, 2, 4, 8, 12, 15)
N_PER = 112  # 15 lengths x 6 thresholds x 112 = 10 080 windows; > 3 x 32 so every offset modulo 32 occurs in every group
I32 = np.int32


@functools.lru_cache(maxsize=None)
def cases(e, L, clean):
    W, R = pa.gap_rich_cases(20260 + clean, e, L, N_PER, clean_text=bool(clean))
    W.setflags(write=False)
    R.setflags(write=False)
    return W, R


@functools.lru_cache(maxsize=None)
def plain_distance(e, L, clean):
    W, R = cases(e, L, clean)
    return pa.band_distance(e, W, R)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _emu():
    L = hl.lib()
    for name in ("hostemu_band_batch", "hostemu_traceback_batch", "hostemu_dropoff_batch", "hostemu_ksw_batch"):
        getattr(L, name).restype = None
    V, I, U = C.c_void_p, C.c_int, C.c_uint32
    L.hostemu_band_batch.argtypes = [I, I, U, U, V, V, I, I, V, V]
    L.hostemu_traceback_batch.argtypes = [I, I, U, U, V, V, I, V, V]
    L.hostemu_dropoff_batch.argtypes = [I, I, U, U, V, V, I, I, V, V, V]
    L.hostemu_ksw_batch.argtypes = [I, I, U, U, V, V, I, V, V, V, V, V]
    return L


def _oracle():
    L = ol.lib()
    L.ora_banded_align_dropoff.restype = C.c_int
    L.ora_banded_align_dropoff.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.ora_ksw_semi_global3.restype = C.c_int
    L.ora_ksw_semi_global3.argtypes = [C.c_int, C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int),
                                       C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return L


def _same(name, e, L, got, want, W, R):
    got = [np.asarray(g, np.int64) for g in got]
    want = [np.asarray(w, np.int64) for w in want]
    bad = np.zeros(len(W), bool)
    for g, w in zip(got, want):
        bad |= g != w
    if bad.any():
        c = int(np.argmax(bad))
        raise AssertionError("%s: e %d L %d: %d of %d cases differ; case %d: got %s, plain DP %s\nwindow %r\nread   %r" % (
            name, e, L, int(bad.sum()), len(W), c, [int(g[c]) for g in got], [int(w[c]) for w in want], W[c].tobytes(), R[c].tobytes()))


@pytest.mark.parametrize("e", ES)
def test_cases_are_gap_rich(e):
    """the generator does what the other tests rely on: per threshold, reads within the threshold that the band alone can
    align (the Hamming count at offset e is larger), distances of exactly e and e + 1, and early exits"""
    within = gapped = at_e = at_e1 = exits = 0
    for L in pa.WORD_LENGTHS:
        W, R = cases(e, L, 0)
        err, end = plain_distance(e, L, 0)
        ham = (pa.classes(W[:, e:e + L]) != pa.classes(R)).sum(axis=1)
        within += int((err <= e).sum())
        gapped += int(((err <= e) & (ham > err)).sum())
        at_e += int(((err == e) & (end >= 0)).sum())
        at_e1 += int(((err == e + 1) & (end >= 0)).sum())
        exits += int((end < 0).sum())
    total = N_PER * len(pa.WORD_LENGTHS)
    # a budget of 0 .. e + 3 edits, gaps of up to e bases: one script in e + 4 is empty, so at least that share stays within e
    assert within >= total // (2 * (e + 4)) and gapped >= 30, (within, gapped)
    assert at_e >= 20 and at_e1 >= 20 and exits >= 5, (at_e, at_e1, exits)


@pytest.mark.parametrize("e", ES)
def test_distance_oracle(e):
    Lo = _oracle()
    for L in pa.WORD_LENGTHS:
        W, R = cases(e, L, 0)
        got = np.zeros((2, len(W)), np.int64)
        for c in range(len(W)):
            ep = C.c_int(-1)
            got[0, c] = Lo.ora_banded_align(e, W[c].tobytes(), R[c].tobytes(), L, C.byref(ep))
            got[1, c] = ep.value
        _same("ora_banded_align", e, L, got, plain_distance(e, L, 0), W, R)


@pytest.mark.parametrize("planes", (0, 1), ids=("bytes", "planes"))
@pytest.mark.parametrize("strand", (0, 1))
@pytest.mark.parametrize("e", ES)
def test_distance_product(e, strand, planes):
    Le = _emu()
    for li, L in enumerate(pa.WORD_LENGTHS):
        W, R = cases(e, L, strand)
        err, end = np.zeros(len(W), I32), np.zeros(len(W), I32)
        Le.hostemu_band_batch(e, L, len(W), li, _ptr(W), _ptr(R), strand, planes, _ptr(err), _ptr(end))
        _same("cm_banded_align" + ("_planes" if planes else ""), e, L, (err, end), plain_distance(e, L, strand), W, R)


@pytest.mark.parametrize("e", ES)
def test_start_oracle_and_product(e):
    Lo, Le = _oracle(), _emu()
    for li, L in enumerate(pa.WORD_LENGTHS):
        for strand in (0, 1):
            W, R = cases(e, L, strand)
            err, _ = plain_distance(e, L, strand)
            keep = err <= e  # the traceback runs on accepted alignments only
            if not keep.any():
                continue
            Wk, Rk, ek = np.ascontiguousarray(W[keep]), np.ascontiguousarray(R[keep]), np.ascontiguousarray(err[keep], I32)
            want = pa.band_start(e, ek, Wk, Rk)
            if strand == 0:
                got = np.zeros(len(Wk), np.int64)
                for c in range(len(Wk)):
                    sp = C.c_int(-7)
                    Lo.ora_banded_traceback(e, int(ek[c]), Wk[c].tobytes(), Rk[c].tobytes(), L, C.byref(sp))
                    got[c] = sp.value
                _same("ora_banded_traceback", e, L, (got,), (want,), Wk, Rk)
            st = np.zeros(len(Wk), I32)
            Le.hostemu_traceback_batch(e, L, len(Wk), li, _ptr(Wk), _ptr(Rk), strand, _ptr(ek), _ptr(st))
            _same("cm_banded_traceback strand %d" % strand, e, L, (st,), (want,), Wk, Rk)


def plain_dropoff_shape(e, W, R, shape):
    """the four calls of the split-alignment verification in terms of plain_align.dropoff"""
    L = R.shape[1]
    allow = 20 - e if shape & 1 else 0
    if shape < 2:
        return pa.dropoff(e, W[:, allow:], R[:, allow:])
    Ls = L - allow
    return pa.dropoff(e, W[:, :Ls + 2 * e][:, ::-1], R[:, :Ls][:, ::-1])


@pytest.mark.parametrize("shape", (0, 1, 2, 3), ids=("fwd", "fwd_allow", "rev3", "rev3_allow"))
@pytest.mark.parametrize("e", ES)
def test_dropoff(e, shape):
    Lo, Le = _oracle(), _emu()
    allow = 20 - e if shape & 1 else 0
    for li, L in enumerate(pa.WORD_LENGTHS):
        if L < 25 or allow + 2 >= L:  # split alignment takes reads of 30 bases and more
            continue
        strand = 1 if shape >= 2 else 0
        W, R = cases(e, L, strand)
        want = plain_dropoff_shape(e, W, R, shape)
        got = np.zeros((3, len(W)), np.int64)
        for c in range(len(W)):
            ep, ln = C.c_int(-1), C.c_int(-1)
            if shape < 2:
                got[0, c] = Lo.ora_banded_align_dropoff(e, W[c, allow:].tobytes(), R[c, allow:].tobytes(), L - allow, 0, C.byref(ep), C.byref(ln))
            else:
                got[0, c] = Lo.ora_banded_align_dropoff(e, W[c].tobytes(), R[c].tobytes(), L - allow, 1, C.byref(ep), C.byref(ln))
            got[1, c], got[2, c] = ep.value, ln.value
        _same("oracle drop-off shape %d" % shape, e, L, got, want, W, R)
        for planes in (0, 1):
            out = [np.zeros(len(W), I32) for _ in range(3)]
            Le.hostemu_dropoff_batch(e, L, len(W), li, _ptr(W), _ptr(R), shape, planes, *[_ptr(o) for o in out])
            _same("cm_banded_align_dropoff%s shape %d" % ("_planes" if planes else "", shape), e, L, out, want, W, R)


@pytest.mark.parametrize("e", ES)
def test_affine(e):
    Lo, Le = _oracle(), _emu()
    w = 2 * e + 1
    for li, L in enumerate(pa.WORD_LENGTHS):
        for strand in (0, 1):
            W, R = cases(e, L, strand)
            want = pa.affine_best(W, R, w)
            n = len(W)
            if strand == 0:
                got = np.zeros((2, n), np.int64)
                for c in range(n):
                    cg = np.zeros(ol.SAM_CIGAR_CAP, np.uint32)
                    nc, st, en = C.c_int(0), C.c_int(-1), C.c_int(-1)
                    got[0, c] = Lo.ora_ksw_semi_global3(L + 2 * e, W[c].tobytes(), L, R[c].tobytes(), w, _ptr(cg), ol.SAM_CIGAR_CAP, C.byref(nc),
                                                        C.byref(st), C.byref(en))
                    got[1, c] = en.value
                    # (at most e + 3 edits: the CIGAR stays far below the 64 operations at which the oracle returns -1 instead)
                    assert nc.value < ol.SAM_CIGAR_CAP
                    sc, _, _ = pa.replay(cg[:nc.value], W[c, st.value:en.value], R[c])
                    assert sc == want[0][c], ("oracle CIGAR replay", e, L, c, sc, int(want[0][c]))
                _same("ora_ksw_semi_global3", e, L, got, want, W, R)
            sc, st, en, nc = (np.zeros(n, I32) for _ in range(4))
            cg = np.zeros((n, ol.SAM_CIGAR_CAP), np.uint32)
            Le.hostemu_ksw_batch(e, L, n, li, _ptr(W), _ptr(R), strand, _ptr(sc), _ptr(st), _ptr(en), _ptr(cg), _ptr(nc))
            assert (nc < ol.SAM_CIGAR_CAP).all()  # no CIGAR near the 64 operations at which the score is withheld
            _same("cm_ksw_sg3 strand %d" % strand, e, L, (sc, en), want, W, R)
            for c in range(n):
                s, _, _ = pa.replay(cg[c, :nc[c]], W[c, st[c]:en[c]], R[c])
                assert s == want[0][c], ("product CIGAR replay", e, L, strand, int(c), s, int(want[0][c]))
