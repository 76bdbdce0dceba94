"""CPU: the two symbols of the deduper's diff call are exported, declared in the header with their prototypes and named in api.EXPORTS,
and refuse bad arguments before they touch a device -- in the manner of tests/test_dedup_abi.py. (The refusals of a call that need a
deduper, and with it a device, are in tests/test_gpu_diff.py.)"""
import ctypes as C

import abi_rig as R

NAMES = ("mscomp_amd_deduper_create_diff", "mscomp_amd_deduper_diff")
PROTOTYPES = (
    "MSCompStatus mscomp_amd_deduper_create_diff(mscomp_amd_ctx* ctx, uint32_t block_size, size_t n_pair, uint64_t n_blocks_new, "
    "uint32_t flags, mscomp_amd_deduper** dd);",
    "MSCompStatus mscomp_amd_deduper_diff(mscomp_amd_deduper* dd, const mscomp_amd_blocks_view* base, const mscomp_amd_blocks_view* next, "
    "const uint64_t* d_pair, uint64_t* d_delta_ext_first, uint64_t* d_delta_ext, uint64_t* d_patch_ext_first, uint64_t* d_patch_ext, "
    "uint64_t* d_changed, uint64_t* d_count, int32_t* d_status);",
)


def test_diff_symbols_are_exported_and_declared():
    import ms_compress_amd as m
    lib = m.load_library()
    hdr = R.check_declared(lib, NAMES, PROTOTYPES)
    assert "#define MSCOMP_AMD_DIFF_NO_BASE 0xFFFFFFFFFFFFFFFFull" in hdr and m.MSCOMP_AMD_DIFF_NO_BASE == 0xFFFFFFFFFFFFFFFF
    assert hdr.index("mscomp_amd_deduper_dedup(") < hdr.index("mscomp_amd_deduper_create_diff(") < hdr.index("mscomp_amd_res_crc_dev(")   # behind the deduper's section
    for part in ("Creation:", "Scratch:", "Sources:", "Notation:", "Rules:", "Consequence:", "Checksums:", "Execution:", "Left out:"):
        assert part in hdr[hdr.index("/* Diff:"): hdr.index("#define MSCOMP_AMD_DIFF_NO_BASE")], part
    assert "#define MSCOMP_AMD_SCRATCH_DEDUPER 6" in hdr and "MSCOMP_AMD_SCRATCH_DIFF" not in hdr        # no new scratch kind
    assert callable(m.BlockDeduper.for_diff) and callable(m.BlockDeduper.diff)
    assert callable(m.blocks_diff) and callable(m.blocks_delta) and callable(m.blocks_patch)


def test_create_diff_argument_errors_without_gpu():
    import ms_compress_amd as m
    lib = m.load_library()
    create = lib.mscomp_amd_deduper_create_diff
    ctx = C.c_void_p(8)                                           # never dereferenced: every check below comes before the context is used

    def refused(*args):
        obj = C.c_void_p(123)
        return create(*args, C.byref(obj)) == m.MSCOMP_ARG_ERROR and not obj.value
    assert refused(None, 4096, 4, 64, 0)                          # a null context
    assert create(ctx, 4096, 4, 64, 0, None) == m.MSCOMP_ARG_ERROR                  # a null out pointer
    for bs in (0, 4095, 6144, 2048, 1048576, 0x80000000):         # block_size: a power of two from 4096 to 524288
        assert refused(ctx, bs, 4, 64, 0), bs
    assert refused(ctx, 65536, 4, 64, 1)                          # no flags
    big = 0x7FFFFFF1
    assert refused(ctx, 4096, big, 64, 0) and refused(ctx, 4096, 4, big, 0) and refused(ctx, 524288, 4, 1 << 40, 0)


def test_diff_null_object():
    import ms_compress_amd as m
    lib = m.load_library()
    p = C.c_void_p(8)                                             # never dereferenced: the deduper is null
    views = (m.BlocksView * 2)()
    assert lib.mscomp_amd_deduper_diff(None, C.byref(views[0]), C.byref(views[1]), p, p, p, p, p, p, p, p) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_deduper_diff(None, None, None, None, None, None, None, None, None, None, None) == m.MSCOMP_ARG_ERROR
