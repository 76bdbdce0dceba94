"""CPU: the block writer (mscomp_amd_writer_*) is exported, declared in the header and named in api.EXPORTS, and refuses bad arguments
before it touches a device -- the ladder of tests/test_reader_abi.py, which mscomp_amd_writer_create follows check for check."""
import ctypes as C

import abi_rig as R

NAMES = ("mscomp_amd_writer_create", "mscomp_amd_writer_destroy", "mscomp_amd_writer_write", "mscomp_amd_writer_counts")


def test_writer_symbols_are_exported_and_declared():
    import ms_compress_amd as m
    lib = m.load_library()
    hdr = R.check_declared(lib, NAMES)
    assert "typedef struct mscomp_amd_writer mscomp_amd_writer;" in hdr
    assert m.BlockWriter is not None and callable(m.blocks_write)


def test_writer_argument_errors_without_gpu():
    import ms_compress_amd as m
    lib = m.load_library()
    create = lib.mscomp_amd_writer_create
    ctx = C.c_void_p(8)                                           # never dereferenced: every check below comes before the context is used

    def refused(*args):
        wr = C.c_void_p(123)
        st = create(*args, C.byref(wr))
        assert not wr.value                                       # the object pointer is cleared on failure
        return st
    for f in (2, 3, 4):                                           # a null context
        assert refused(None, f, 4096, 4, 64, 8, 16, 0) == m.MSCOMP_ARG_ERROR
    for bad in (0, 1, 5, 99):                                     # a bad format
        assert refused(ctx, bad, 4096, 4, 64, 8, 16, 0) == m.MSCOMP_ARG_ERROR
    for bs in (0, 4095, 6144, 2048, 1048576, 0x80000000):         # block_size: a power of two from 4096 to 524288
        assert refused(ctx, 2, bs, 4, 64, 8, 16, 0) == m.MSCOMP_ARG_ERROR
    for flags in (1, 2, 0x80000000):                              # flags must be 0
        assert refused(ctx, 3, 65536, 4, 64, 8, 16, flags) == m.MSCOMP_ARG_ERROR
    big = 0x7FFFFFF1
    assert refused(ctx, 2, 4096, big, 64, 8, 16, 0) == m.MSCOMP_ARG_ERROR          # each of the four counts
    assert refused(ctx, 2, 4096, 4, big, 8, 16, 0) == m.MSCOMP_ARG_ERROR
    assert refused(ctx, 2, 4096, 4, 64, big, 16, 0) == m.MSCOMP_ARG_ERROR
    assert refused(ctx, 2, 4096, 4, 64, 8, big, 0) == m.MSCOMP_ARG_ERROR
    assert refused(ctx, 2, 4096, 4, 1 << 40, 8, 16, 0) == m.MSCOMP_ARG_ERROR
    for f in (2, 3, 4):                                           # a cache beyond what a dev plan addresses
        assert refused(ctx, f, 524288, 4, 64, 8, 0x7FFFFFF0, 0) == m.MSCOMP_MEM_ERROR
    assert create(None, 2, 4096, 4, 64, 8, 16, 0, None) == m.MSCOMP_ARG_ERROR       # a null object pointer
    assert create(ctx, 2, 4096, 4, 64, 8, 16, 0, None) == m.MSCOMP_ARG_ERROR


def test_writer_null_object():
    import ms_compress_amd as m
    lib = m.load_library()
    lib.mscomp_amd_writer_destroy(None)                           # a no-op
    p = C.c_void_p(8)
    assert lib.mscomp_amd_writer_write(None, p, 16, p, p, p, None, p, p, p, p, 16, p, None, p, p, p) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_writer_write(None, p, 16, p, p, p, p, p, p, p, p, 16, p, p, p, p, p) == m.MSCOMP_ARG_ERROR
    out = (C.c_uint32 * 3)()
    assert lib.mscomp_amd_writer_counts(None, out) == -1
