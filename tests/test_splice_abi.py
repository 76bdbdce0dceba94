"""CPU: the splicer's three symbols are exported, declared in the header and named in api.EXPORTS, and refuse bad arguments before they
touch a device -- in the manner of tests/test_resize_abi.py."""
import ctypes as C

import abi_rig as R

NAMES = ("mscomp_amd_splicer_create", "mscomp_amd_splicer_destroy", "mscomp_amd_splicer_splice")


def test_splice_symbols_are_exported_and_declared():
    import ms_compress_amd as m
    lib = m.load_library()
    hdr = R.check_declared(lib, NAMES)
    assert "#define MSCOMP_AMD_SPLICE_SRC_MAX 4u" in hdr and "mscomp_amd_blocks_view" in hdr and m.MSCOMP_AMD_SPLICE_SRC_MAX == 4
    assert callable(m.BlockSplicer.splice) and callable(m.blocks_splice)
    assert C.sizeof(m.BlocksView) == 64                           # eight words, as the header lays them out


def test_create_argument_errors_without_gpu():
    import ms_compress_amd as m
    lib = m.load_library()
    create = lib.mscomp_amd_splicer_create
    ctx = C.c_void_p(8)                                           # never dereferenced: every check below comes before the context is used

    def refused(*args):
        obj = C.c_void_p(123)
        return create(*args, C.byref(obj)) == m.MSCOMP_ARG_ERROR and not obj.value
    assert refused(None, 4096, 1, 4, 64, 0)                       # a null context
    assert create(ctx, 4096, 1, 4, 64, 0, None) == m.MSCOMP_ARG_ERROR               # a null out pointer
    for bs in (0, 4095, 6144, 2048, 1048576, 0x80000000):         # block_size: a power of two from 4096 to 524288
        assert refused(ctx, bs, 1, 4, 64, 0), bs
    for n_src in (0, 5, 0xFFFFFFFF):                              # 1 .. MSCOMP_AMD_SPLICE_SRC_MAX sources
        assert refused(ctx, 4096, n_src, 4, 64, 0), n_src
    assert refused(ctx, 65536, 2, 4, 64, 1)                       # no flags
    big = 0x7FFFFFF1
    assert refused(ctx, 4096, 4, big, 64, 0) and refused(ctx, 4096, 4, 4, big, 0) and refused(ctx, 524288, 1, 4, 1 << 40, 0)


def test_splice_null_object():
    import ms_compress_amd as m
    lib = m.load_library()
    p = C.c_void_p(8)                                             # never dereferenced: the splicer is null
    views = (m.BlocksView * 1)()
    assert lib.mscomp_amd_splicer_splice(None, views, p, p, 16, p, p, p, p, p) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_splicer_splice(None, views, p, p, 16, p, p, None, p, p) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_splicer_splice(None, None, None, None, 0, None, None, None, None, None) == m.MSCOMP_ARG_ERROR
    lib.mscomp_amd_splicer_destroy(None)                          # a null splicer is nothing to destroy
