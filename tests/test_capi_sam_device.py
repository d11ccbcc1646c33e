"""The C ABI of SAM output through the device ingest (include/chromap_amd.h: read store, SAM record store, SAM text on the
device): the built library exports every entry point, and each refuses a NULL context with CMGPU_EINVAL.  No GPU needed."""
import ctypes as C

from chromap_amd import _capi

EINVAL = -1  # CMGPU_EINVAL
NEW = ("cmgpu_fastq_keep_reads", "cmgpu_reads_clear", "cmgpu_reads_info", "cmgpu_download_reads", "cmgpu_sam_store_append_resident",
       "cmgpu_sam_store_clear", "cmgpu_sam_store_info", "cmgpu_store_format_sam", "cmgpu_write_sam_header")


def test_new_symbols_are_exported_and_declared():
    L = _capi.lib()
    for s in NEW:
        assert s in _capi.SYMBOLS, s
        assert hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s


def test_null_context_is_einval():
    L = _capi.lib()
    n, nb, b32 = C.c_uint64(7), C.c_uint64(7), C.c_uint32(7)
    off = (C.c_uint64 * 2)()
    p = _capi.default_params()
    names = (C.c_char_p * 1)(b"chr1")
    lens = (C.c_uint32 * 1)(100)
    assert L.cmgpu_fastq_keep_reads(None, 1) == EINVAL
    assert L.cmgpu_reads_clear(None) == EINVAL
    assert L.cmgpu_reads_info(None, 0, C.byref(n), C.byref(nb), C.byref(nb), C.byref(b32)) == EINVAL
    assert L.cmgpu_download_reads(None, 0, None, 0, C.cast(off, C.c_void_p), None, None, 0, C.cast(off, C.c_void_p)) == EINVAL
    assert L.cmgpu_sam_store_append_resident(None, C.byref(n)) == EINVAL
    assert L.cmgpu_sam_store_clear(None) == EINVAL
    assert L.cmgpu_sam_store_info(None, C.byref(n), C.byref(nb)) == EINVAL
    assert L.cmgpu_store_format_sam(None, names, C.cast(lens, C.c_void_p), 1, C.byref(p), 0, C.byref(n), C.byref(nb)) == EINVAL
    assert n.value == 7 and nb.value == 7  # (nothing was written)


def test_sam_header_is_written_on_the_host(tmp_path):
    """cmgpu_write_sam_header has no context: NULL arguments are EINVAL, and the @SQ lines are the host writer's"""
    L = _capi.lib()
    names = (C.c_char_p * 2)(b"chr1", b"chrUn_x")
    lens = (C.c_uint32 * 2)(1000, 4000000000)
    out = str(tmp_path / "h.sam")
    assert L.cmgpu_write_sam_header(None, C.cast(lens, C.c_void_p), 2, out.encode()) == EINVAL
    assert L.cmgpu_write_sam_header(names, None, 2, out.encode()) == EINVAL
    assert L.cmgpu_write_sam_header(names, C.cast(lens, C.c_void_p), 2, None) == EINVAL
    assert L.cmgpu_write_sam_header(names, C.cast(lens, C.c_void_p), 2, out.encode()) == 0
    assert open(out, "rb").read() == b"@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:chrUn_x\tLN:4000000000\n"
