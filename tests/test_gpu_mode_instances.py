"""The per-mode instances of the S4-S6 kernels (cm_stages.h: CmModePe / CmModeAny) against the instances that carry every mode:
each case is mapped with cmgpu_set_option("generic_kernels") 0 and 1, and the record bytes and every Stats field must be equal.
A 2 Mbp synthetic genome and 20 000 pairs per case.  The paired-end instances serve a batch that is neither single-end nor
split-aligned; the single-end and split cases are guards (both settings run the generic instances there), and so is --SAM for S6,
which has kernels of its own."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 20000
PLAIN = (2_000_000, 4, 99)
REPEATS = (2_000_000, 4, 4242, (8, 40, 1500, 0.005))  # planted repeat families: pairs with several best pairings


def _both(g, run):
    """run() maps the batch and returns (records, stats dict) -- with the per-mode instances, then with the generic ones"""
    out = []
    for generic in (0, 1):
        g.set_option("generic_kernels", generic)
        assert g.get_option("generic_kernels") == generic
        out.append(run())
    g.set_option("generic_kernels", 0)
    (rec0, st0), (rec1, st1) = out
    for key in st1:
        assert st0[key] == st1[key], key
    assert rec0 == rec1
    return rec0, st0


def _resident(g, n):
    from chromap_amd import Stats

    def run():
        st = Stats()
        k = g.map_resident(st)
        rec, k2 = g.download_records(n * max(1, int(g.params.max_num_best_mappings)))
        assert k2 == k
        return bytes(rec)[:k * 24], st.as_dict()
    return run


def test_atac_with_dead_pairs():
    """every fifth pair has a mate below min_read_length: S5a's early return for dead pairs writes what cm_s5_verify wrote"""
    from chromap_amd import ChromapGPU
    g = ChromapGPU(synthetic=PLAIN, preset="atac")
    g.generate_resident(N, read_length=50, frag_min=30, frag_max=500, sub_rate=0.01, seed=51)
    b1, o1, b2, o2 = g.download_batch(N)
    short = int(g.params.min_read_length) - 10
    assert short > 0
    len1 = np.diff(o1.astype(np.int64))
    len1[::5] = np.minimum(len1[::5], short)
    keep = np.concatenate([np.arange(int(o1[i]), int(o1[i]) + int(len1[i])) for i in range(N)])
    n1 = np.zeros(N + 1, np.uint32)
    n1[1:] = np.cumsum(len1)
    g.upload(b1[keep], n1, b2, o2)
    rec, st = _both(g, _resident(g, N))
    # the short reads' pairs are gone, the others map
    ids = np.frombuffer(rec, np.uint32).reshape(-1, 6)[:, 0]
    assert len(ids) > 0.7 * N and not np.any(ids % 5 == 0)
    g.close()


def test_atac_multi_mappers_fill_the_s6c_list():
    """mapq_threshold=0 on planted repeats: the list S6c works through holds multi-mapped pairs, several of one wave"""
    from chromap_amd import ChromapGPU
    g = ChromapGPU(synthetic=REPEATS, preset="atac", mapq_threshold=0)
    g.generate_resident(N, read_length=50, frag_min=30, frag_max=600, sub_rate=0.01, seed=11, indel_rate=0.002)
    rec, st = _both(g, _resident(g, N))
    print("multi-mappers: %d of %d pairs" % (st["num_multi_mappers"], N))
    assert st["num_multi_mappers"] > N // 64  # more listed pairs than S6a has waves: some wave appends two or more
    g.close()


def test_atac_without_multi_mappers():
    """no pair has a second best pairing: the list is empty (its kernel is not even launched once the launch set has aged)"""
    from chromap_amd import ChromapGPU
    g = ChromapGPU(synthetic=PLAIN, preset="atac")
    g.generate_resident(N, read_length=50, frag_min=30, frag_max=500, sub_rate=0.01, seed=52)
    rec, st = _both(g, _resident(g, N))
    assert st["num_multi_mappers"] == 0 and st["num_mapped_reads"] > 1.6 * N
    g.close()


def test_hic_preset():
    """split alignment: the generic instances whatever the option says"""
    from chromap_amd import ChromapGPU
    g = ChromapGPU(synthetic=PLAIN, preset="hic")
    g.generate_resident(N, read_length=100, sub_rate=0.01, indel_rate=0.001, seed=5, hic=0.35)
    rec, st = _both(g, _resident(g, N))
    assert len(rec) > 0.7 * N * 24
    g.close()


def _single(g, b, off):
    from chromap_amd import Stats

    def run():
        g.stats = Stats()  # (map_single adds to the mapper's own counters)
        rec, k = g.map_single(b, off)
        return bytes(rec)[:k * 24], g.stats.as_dict()
    return run


@pytest.mark.parametrize("preset", ["atac", "hic"], ids=["single_end", "single_end_split"])
def test_single_end(preset):
    """single-end reads, without and with split alignment (guards: the generic instances on both settings)"""
    from chromap_amd import ChromapGPU
    g = ChromapGPU(synthetic=REPEATS, preset=preset)
    g.generate_resident(N, read_length=60, frag_min=80, frag_max=500, sub_rate=0.01, seed=53)
    b1, o1, _, _ = g.download_batch(N)
    rec, st = _both(g, _single(g, b1, o1))
    assert len(rec) > 0.7 * N * 24
    g.close()


def test_sam_output():
    """--SAM has S6 kernels of its own (guard; S4 and S5 are the paired-end instances): records, CIGARs and MD strings"""
    from chromap_amd import ChromapGPU, Stats, _capi
    g = ChromapGPU(synthetic=REPEATS, preset="atac", output_format=_capi.FORMAT_SAM)
    g.generate_resident(N, read_length=50, frag_min=30, frag_max=600, sub_rate=0.01, seed=12, indel_rate=0.002)

    def run():
        st = Stats()
        k = g.map_resident(st)
        rec, k2 = g.download_records(N * max(1, int(g.params.max_num_best_mappings)))
        assert k2 == k
        sam, cigar, md, _, _ = g.download_sam()
        return bytes(rec)[:k * 24] + bytes(sam) + cigar.tobytes() + md.tobytes(), st.as_dict()
    rec, st = _both(g, run)
    assert st["num_mapped_reads"] > 1.4 * N
    g.close()
