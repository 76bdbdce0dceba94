"""CPU: the block container (mscomp_amd_blocks_*) is exported, declared in the header and named in api.EXPORTS, and refuses bad arguments
before it touches a device."""
import ctypes as C

import abi_rig as R

NAMES = ("mscomp_amd_blocks_create", "mscomp_amd_blocks_destroy", "mscomp_amd_blocks_bound", "mscomp_amd_blocks_compress", "mscomp_amd_blocks_decompress")


def test_blocks_symbols_are_exported_and_declared():
    import ms_compress_amd as m
    lib = m.load_library()
    hdr = R.check_declared(lib, NAMES)
    assert "typedef struct mscomp_amd_blocks mscomp_amd_blocks;" in hdr
    assert m.BlockContainer is not None and callable(m.blocks_compress) and callable(m.blocks_decompress)


def test_blocks_argument_errors_without_gpu():
    import ms_compress_amd as m
    lib = m.load_library()
    create = lib.mscomp_amd_blocks_create
    ctx = C.c_void_p(8)                                           # never dereferenced: every check below comes before the context is used

    def refused(*args):
        bk = C.c_void_p(123)
        st = create(*args, C.byref(bk))
        assert not bk.value                                       # the object pointer is cleared on failure
        return st
    for f in (2, 3, 4):                                           # a null context
        assert refused(None, f, 4096, 4, 1 << 20, 0) == m.MSCOMP_ARG_ERROR
    for bad in (0, 1, 5, 99):                                     # a bad format
        assert refused(ctx, bad, 4096, 4, 1 << 20, 0) == m.MSCOMP_ARG_ERROR
    for bs in (0, 4095, 6144, 2048, 1048576, 0x80000000):         # block_size: a power of two from 4096 to 524288
        assert refused(ctx, 2, bs, 4, 1 << 20, 0) == m.MSCOMP_ARG_ERROR
    for flags in (1, 2, 0x80000000):                              # flags must be 0
        assert refused(ctx, 3, 65536, 4, 1 << 20, flags) == m.MSCOMP_ARG_ERROR
    assert refused(ctx, 2, 4096, 0x7FFFFFF1, 1 << 20, 0) == m.MSCOMP_ARG_ERROR   # too many resources
    assert refused(ctx, 2, 4096, 16, 1 << 62, 0) == m.MSCOMP_MEM_ERROR          # more blocks than the tables can address
    assert create(None, 2, 4096, 4, 1 << 20, 0, None) == m.MSCOMP_ARG_ERROR      # a null object pointer
    assert create(ctx, 2, 4096, 4, 1 << 20, 0, None) == m.MSCOMP_ARG_ERROR


def test_blocks_null_object():
    import ms_compress_amd as m
    lib = m.load_library()
    lib.mscomp_amd_blocks_destroy(None)                           # a no-op
    assert lib.mscomp_amd_blocks_bound(None) == 0
    p = C.c_void_p(8)
    assert lib.mscomp_amd_blocks_compress(None, p, p, p, p, 16, p, p, p) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_blocks_decompress(None, p, 16, p, p, p, None, p, p, p, p, p) == m.MSCOMP_ARG_ERROR
