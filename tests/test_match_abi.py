"""CPU: the two symbols of the deduper's match call are exported, declared in the header with their prototypes and named in api.EXPORTS,
and refuse bad arguments before they touch a device -- in the manner of tests/test_diff_abi.py. (The refusals of a call that need a
deduper, and with it a device, are in tests/test_gpu_match.py.)"""
import ctypes as C

import abi_rig as R

NAMES = ("mscomp_amd_deduper_create_match", "mscomp_amd_deduper_match")
PROTOTYPES = (
    "MSCompStatus mscomp_amd_deduper_create_match(mscomp_amd_ctx* ctx, uint32_t block_size, uint32_t n_src, size_t n_res_total, "
    "uint64_t n_blocks_total, uint64_t n_blocks_new, uint32_t flags, mscomp_amd_deduper** dd);",
    "MSCompStatus mscomp_amd_deduper_match(mscomp_amd_deduper* dd, const mscomp_amd_blocks_view* store, const mscomp_amd_blocks_view* next, "
    "uint64_t* d_delta_ext_first, uint64_t* d_delta_ext, uint64_t* d_patch_ext_first, uint64_t* d_patch_ext, uint64_t* d_class, "
    "uint64_t* d_count, int32_t* d_status);",
)


def test_match_symbols_are_exported_and_declared():
    import ms_compress_amd as m
    lib = m.load_library()
    hdr = R.check_declared(lib, NAMES, PROTOTYPES)
    # behind diff's section, in front of the transcoder's
    assert hdr.index("mscomp_amd_deduper_diff(") < hdr.index("mscomp_amd_deduper_create_match(") < hdr.index("mscomp_amd_deduper_match(")
    assert hdr.index("mscomp_amd_deduper_match(mscomp_amd_deduper* dd") < hdr.index("typedef struct mscomp_amd_transcoder")
    section = hdr[hdr.index("/* Match:"): hdr.index("MSCompStatus mscomp_amd_deduper_create_match(")]
    for part in ("Creation:", "Scratch:", "Sources:", "Notation:", "Rules:", "Consequence:", "Checksums:", "Execution:", "Left out:"):
        assert part in section, part
    assert "#define MSCOMP_AMD_SCRATCH_DEDUPER 6" in hdr and "MSCOMP_AMD_SCRATCH_MATCH" not in hdr       # no new scratch kind
    assert callable(m.BlockDeduper.for_match) and callable(m.BlockDeduper.match)
    assert callable(m.blocks_match) and callable(m.blocks_match_delta) and callable(m.blocks_match_patch) and callable(m.blocks_single_instance)


def test_create_match_argument_errors_without_gpu():
    import ms_compress_amd as m
    lib = m.load_library()
    create = lib.mscomp_amd_deduper_create_match
    ctx = C.c_void_p(8)                                           # never dereferenced: every check below comes before the context is used

    def refused(*args):
        obj = C.c_void_p(123)
        return create(*args, C.byref(obj)) == m.MSCOMP_ARG_ERROR and not obj.value
    assert refused(None, 4096, 1, 4, 64, 32, 0)                   # a null context
    assert create(ctx, 4096, 1, 4, 64, 32, 0, None) == m.MSCOMP_ARG_ERROR           # a null out pointer
    for bs in (0, 4095, 6144, 2048, 1048576, 0x80000000):         # block_size: a power of two from 4096 to 524288
        assert refused(ctx, bs, 1, 4, 64, 32, 0), bs
    assert refused(ctx, 65536, 1, 4, 64, 32, 1)                   # no flags
    for n_src in (4, 5, 0xFFFFFFFF):                              # at most three stores (none is legal: that needs a device)
        assert refused(ctx, 4096, n_src, 4, 64, 32, 0), n_src
    big = 0x7FFFFFF1
    assert refused(ctx, 4096, 0, big, 64, 32, 0) and refused(ctx, 4096, 3, 4, big, 32, 0) and refused(ctx, 524288, 1, 4, 1 << 40, 32, 0)
    assert refused(ctx, 4096, 1, 4, 64, 65, 0) and refused(ctx, 4096, 1, 4, 0, 1, 0)     # the new rows are among all rows


def test_match_null_object():
    import ms_compress_amd as m
    lib = m.load_library()
    p = C.c_void_p(8)                                             # never dereferenced: the deduper is null
    views = (m.BlocksView * 2)()
    assert lib.mscomp_amd_deduper_match(None, views, C.byref(views[1]), p, p, p, p, p, p, p) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_deduper_match(None, None, None, None, None, None, None, None, None, None) == m.MSCOMP_ARG_ERROR
