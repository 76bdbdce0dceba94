"""CPU: the deduper's three symbols are exported, declared in the header with their prototypes and named in api.EXPORTS, and refuse bad
arguments before they touch a device -- in the manner of tests/test_splice_abi.py. (The refusals of a call that need a deduper, and with it
a device, are in tests/test_gpu_dedup.py.)"""
import ctypes as C

import abi_rig as R

NAMES = ("mscomp_amd_deduper_create", "mscomp_amd_deduper_destroy", "mscomp_amd_deduper_dedup")
PROTOTYPES = (
    "MSCompStatus mscomp_amd_deduper_create(mscomp_amd_ctx* ctx, uint32_t block_size, uint32_t n_src, size_t n_res_total, "
    "uint64_t n_blocks_total, uint32_t flags, mscomp_amd_deduper** dd);",
    "void mscomp_amd_deduper_destroy(mscomp_amd_deduper* dd);",
    "MSCompStatus mscomp_amd_deduper_dedup(mscomp_amd_deduper* dd, const mscomp_amd_blocks_view* src, uint64_t* d_rep, uint64_t* d_new_index, "
    "uint64_t* d_pick, uint64_t* d_count, int32_t* d_status);",
)


def test_dedup_symbols_are_exported_and_declared():
    import ms_compress_amd as m
    lib = m.load_library()
    hdr = R.check_declared(lib, NAMES, PROTOTYPES)
    assert "typedef struct mscomp_amd_deduper mscomp_amd_deduper;" in hdr
    assert hdr.index("mscomp_amd_splicer_splice(") < hdr.index("mscomp_amd_deduper_create(") < hdr.index("mscomp_amd_res_crc_dev(")   # behind the splicer's section
    assert callable(m.BlockDeduper.dedup) and callable(m.blocks_dedup)


def test_create_argument_errors_without_gpu():
    import ms_compress_amd as m
    lib = m.load_library()
    create = lib.mscomp_amd_deduper_create
    ctx = C.c_void_p(8)                                           # never dereferenced: every check below comes before the context is used

    def refused(*args):
        obj = C.c_void_p(123)
        return create(*args, C.byref(obj)) == m.MSCOMP_ARG_ERROR and not obj.value
    assert refused(None, 4096, 1, 4, 64, 0)                       # a null context
    assert create(ctx, 4096, 1, 4, 64, 0, None) == m.MSCOMP_ARG_ERROR               # a null out pointer
    for bs in (0, 4095, 6144, 2048, 1048576, 0x80000000):         # block_size: a power of two from 4096 to 524288
        assert refused(ctx, bs, 1, 4, 64, 0), bs
    for n_src in (0, m.MSCOMP_AMD_SPLICE_SRC_MAX + 1, 0xFFFFFFFF):   # 1 .. MSCOMP_AMD_SPLICE_SRC_MAX sources
        assert refused(ctx, 4096, n_src, 4, 64, 0), n_src
    assert refused(ctx, 65536, 2, 4, 64, 1)                       # no flags
    big = 0x7FFFFFF1
    assert refused(ctx, 4096, 4, big, 64, 0) and refused(ctx, 4096, 4, 4, big, 0) and refused(ctx, 524288, 1, 4, 1 << 40, 0)


def test_dedup_null_object():
    import ms_compress_amd as m
    lib = m.load_library()
    p = C.c_void_p(8)                                             # never dereferenced: the deduper is null
    views = (m.BlocksView * 1)()
    assert lib.mscomp_amd_deduper_dedup(None, views, p, p, p, p, p) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_deduper_dedup(None, None, None, None, None, None, None) == m.MSCOMP_ARG_ERROR
    lib.mscomp_amd_deduper_destroy(None)                          # a null deduper is nothing to destroy
