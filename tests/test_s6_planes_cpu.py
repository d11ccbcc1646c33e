"""S6's leading mismatch count on bit planes (chromap_amd/csrc/cm_stages.h: cm_hamming_diag_planes, which cm_ref_start_end takes for
reads of at most 64 bases made of upper-case A/C/G/T only) compiled for the host (tests/hostemu/hostemu_s6_planes.cpp):
  count     against cm_hamming_diag on the bytes the planes were packed from, case by case with exact equality: read lengths around the
            32- and 64-bit borders, windows in two and in three reference records, both strands, 0 / 1 / 3 / L substitutions with the
            first and the last base among them, reference windows with lower-case letters, with N, and over a chromosome's end;
  dispatch  cm_ref_start_end with the option on and off: reads with N, with a lower-case base and of 65 bases carry flag 0 and stay on
            bytes; plain reads, with a deletion and at both chromosome ends too, give the same span either way;
and the same cases in a stand-alone program under AddressSanitizer / UndefinedBehaviorSanitizer."""
import ctypes as C
import subprocess

import pytest

from hostemu_s6_planes_lib import lib, sanitizer_program

LENGTHS = (17, 31, 32, 33, 50, 63, 64)
SHIFTS = (0, 1, 17, 31)          # g & 31: a window of L bases lies in three records when shift + L > 64
MIS = {0: "none", 1: "first", 2: "last", 3: "first+middle+last", 4: "all"}
REF = {0: "upper", 1: "lower-case", 2: "N", 3: "chromosome end", 4: "lower-case+N+end"}


def count_case(L, sh, strand, mis, ref_kind, extra, seed=1):
    out = (C.c_int32 * 5)(-1, -1, -1, -1, -1)
    assert lib().hostemu_s6p_case(L, sh, strand, mis, ref_kind, extra, seed, out) == 0
    return list(out)


@pytest.mark.parametrize("strand", (0, 1))
@pytest.mark.parametrize("sh", SHIFTS)
@pytest.mark.parametrize("L", LENGTHS)
def test_plane_count_equals_byte_count(L, sh, strand):
    three_records = 0
    for mis in MIS:
        for ref_kind in REF:
            for extra in (0, 5):
                if L + extra > 64:
                    continue
                by, p1, p2, built, plain = count_case(L, sh, strand, mis, ref_kind, extra)
                what = (L, sh, strand, MIS[mis], REF[ref_kind], extra)
                assert plain == 1, what
                assert p2 == by, what   # two words per read plane
                assert p1 == by, what   # one word per read plane (batches of reads of up to 32 bases)
                assert by == built, what  # ... and both are the mismatches the case was built with
                want_min = {0: 0, 1: 1, 2: 1, 3: 3, 4: L}[mis]
                assert by >= want_min and (ref_kind != 0 or by == want_min), what
                three_records += sh + L > 64
    assert three_records == (len(MIS) * len(REF) * (2 if L + 5 <= 64 else 1) if sh + L > 64 else 0)


def test_sweep_covers_two_and_three_records():
    assert any(sh + L <= 64 for L in LENGTHS for sh in SHIFTS) and any(sh + L > 64 for L in LENGTHS for sh in SHIFTS)
    assert any(sh + L > 64 and L <= 50 for L in LENGTHS for sh in SHIFTS)  # the third record for a headline read too


DISPATCH = {0: "plain, substitutions", 1: "plain, a deletion", 2: "an N", 3: "a lower-case base", 4: "65 bases",
            5: "plain, chromosome end", 6: "plain, chromosome start"}


@pytest.mark.parametrize("strand", (0, 1))
@pytest.mark.parametrize("kind", sorted(DISPATCH))
def test_ref_start_end_dispatch(kind, strand):
    for seed in (1, 2, 3):
        out = (C.c_uint32 * 9)()
        assert lib().hostemu_s6p_dispatch(kind, strand, seed, out) == 0
        on, off, flag, nerr, pos = tuple(out[0:3]), tuple(out[3:6]), out[6], out[7], out[8]
        assert flag == (0 if kind in (2, 3, 4) else 1), DISPATCH[kind]
        assert on == off, (DISPATCH[kind], strand, seed)
        assert nerr > 0  # (no early return: the count runs)
        assert off[0] == 0 and off[1] == pos, (DISPATCH[kind], strand, seed, off, pos)  # the start that was planted


def test_whole_sweep_in_one_call():
    bad = (C.c_int32 * 6)()
    n = lib().hostemu_s6p_sweep(1, bad)
    assert n > 0, (n, list(bad))
    assert n == sum(1 for L in LENGTHS for _ in SHIFTS for _ in (0, 1) for _ in MIS for _ in REF for x in (0, 5) if L + x <= 64) + 2 * len(DISPATCH)


def test_cases_under_address_and_undefined_sanitizers():
    r = subprocess.run([sanitizer_program()], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "cases equal" in r.stdout, r.stdout[-4000:]
