"""CPU: the four symbols of the block transcoder are exported, declared in the header with their prototypes and named in api.EXPORTS, and
refuse bad arguments before they touch a device -- in the manner of tests/test_diff_abi.py. (The refusals of a call that need a
transcoder, and with it a device, are in tests/test_gpu_transcode.py.)"""
import ctypes as C

import abi_rig as R

NAMES = ("mscomp_amd_transcoder_create", "mscomp_amd_transcoder_destroy", "mscomp_amd_transcoder_transcode", "mscomp_amd_transcoder_counts")
PROTOTYPES = (
    "MSCompStatus mscomp_amd_transcoder_create(mscomp_amd_ctx* ctx, MSCompFormat format, uint32_t block_size, MSCompFormat new_format, "
    "uint32_t new_block_size, size_t n_res, uint64_t n_blocks_table, uint64_t n_blocks_new, uint64_t groups_max, uint32_t flags, "
    "mscomp_amd_transcoder** tc);",
    "void mscomp_amd_transcoder_destroy(mscomp_amd_transcoder* tc);",
    "MSCompStatus mscomp_amd_transcoder_transcode(mscomp_amd_transcoder* tc, const uint8_t* d_packed, uint64_t packed_len, "
    "const uint64_t* d_block_first, const uint64_t* d_block_off, const uint64_t* d_res_len, const uint32_t* d_block_crc, "
    "uint8_t* d_new_packed, uint64_t new_cap, uint64_t* d_new_block_first, uint64_t* d_new_block_off, uint32_t* d_new_block_crc, "
    "int32_t* d_status);",
    "int mscomp_amd_transcoder_counts(mscomp_amd_transcoder* tc, uint32_t out[3]);",
)
LZNT1, XPRESS, XHUFF = 2, 3, 4


def test_transcoder_symbols_are_exported_and_declared():
    import ms_compress_amd as m
    lib = m.load_library()
    hdr = R.check_declared(lib, NAMES, PROTOTYPES)
    assert hdr.index("mscomp_amd_deduper_diff(") < hdr.index("mscomp_amd_transcoder_create(") < hdr.index("mscomp_amd_res_crc_dev(")   # behind the deduper's section
    doc = hdr[hdr.index("/* Block transcoders:"): hdr.index("typedef struct mscomp_amd_transcoder")]
    for part in ("Creation:", "Contract:", "Rules:", "Counts:", "Execution:", "What carrying trusts"):
        assert part in doc, part
    assert "MSCOMP_AMD_SCRATCH_TRANSCODER" not in hdr                            # no scratch kind, no context buffer
    assert callable(m.BlockTranscoder.transcode) and callable(m.BlockTranscoder.counts) and callable(m.blocks_transcode)


def test_create_argument_errors_without_gpu():
    import ms_compress_amd as m
    lib = m.load_library()
    create = lib.mscomp_amd_transcoder_create
    ctx = C.c_void_p(8)                                           # never dereferenced: every check below comes before the context is used

    def status(*args):
        obj = C.c_void_p(123)
        st = create(*args, C.byref(obj))
        assert not obj.value                                      # *tc is cleared on every failure
        return st
    ok = (LZNT1, 4096, LZNT1, 65536, 4, 64, 8, 8, 0)
    assert status(None, *ok) == m.MSCOMP_ARG_ERROR                # a null context
    assert create(ctx, *ok, None) == m.MSCOMP_ARG_ERROR           # a null out pointer
    for bs in (0, 4095, 6144, 2048, 1048576, 0x80000000):         # either block size: a power of two from 4096 to 524288
        assert status(ctx, LZNT1, bs, LZNT1, 65536, 4, 64, 8, 8, 0) == m.MSCOMP_ARG_ERROR, bs
        assert status(ctx, LZNT1, 4096, LZNT1, bs, 4, 64, 8, 8, 0) == m.MSCOMP_ARG_ERROR, bs
    for fmt in (0, 1, 5, -1):                                     # either format: one of the three codecs
        assert status(ctx, fmt, 4096, LZNT1, 65536, 4, 64, 8, 8, 0) == m.MSCOMP_ARG_ERROR, fmt
        assert status(ctx, LZNT1, 4096, fmt, 65536, 4, 64, 8, 8, 0) == m.MSCOMP_ARG_ERROR, fmt
    assert status(ctx, LZNT1, 4096, LZNT1, 65536, 4, 64, 8, 8, 1) == m.MSCOMP_ARG_ERROR          # no flags
    big = 0x7FFFFFF1
    for at in range(4):                                           # n_res, n_blocks_table, n_blocks_new, groups_max
        counts = [4, 64, 8, 8]
        counts[at] = big
        assert status(ctx, LZNT1, 4096, LZNT1, 65536, *counts, 0) == m.MSCOMP_ARG_ERROR, at
    for fmt in (LZNT1, XPRESS, XHUFF):                            # nothing to change: that is a splice
        assert status(ctx, fmt, 32768, fmt, 32768, 4, 64, 64, 8, 0) == m.MSCOMP_ARG_ERROR
    # the units of the inner plans: groups_max G / B1 of them are more than a dev plan takes
    assert status(ctx, LZNT1, 4096, LZNT1, 524288, 4, 64, 8, 0x7FFFFFF0, 0) == m.MSCOMP_MEM_ERROR
    assert status(ctx, XPRESS, 524288, LZNT1, 4096, 4, 64, 8, 0x7FFFFFF0, 0) == m.MSCOMP_MEM_ERROR


def test_transcoder_null_object():
    import ms_compress_amd as m
    lib = m.load_library()
    p = C.c_void_p(8)                                             # never dereferenced: the transcoder is null
    assert lib.mscomp_amd_transcoder_transcode(None, p, 0, p, p, p, p, p, 0, p, p, p, p) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_transcoder_transcode(None, None, 0, None, None, None, None, None, 0, None, None, None, None) == m.MSCOMP_ARG_ERROR
    out = (C.c_uint32 * 3)()
    assert lib.mscomp_amd_transcoder_counts(None, out) == -1
    lib.mscomp_amd_transcoder_destroy(None)                       # a no-op
