"""CPU: the four symbols of the block syncer are exported, declared in the header with their prototypes and named in api.EXPORTS, and
refuse bad arguments before they touch a device -- in the manner of tests/test_match_abi.py. (The refusals of a call that need a syncer,
and with it a device, are in tests/test_gpu_sync.py.)"""
import ctypes as C
import re

import abi_rig as R

NAMES = ("mscomp_amd_syncer_create", "mscomp_amd_syncer_destroy", "mscomp_amd_syncer_sync", "mscomp_amd_syncer_counts")
PROTOTYPES = (
    "MSCompStatus mscomp_amd_syncer_create(mscomp_amd_ctx* ctx, MSCompFormat format, uint32_t block_size, size_t n_res, uint64_t n_blocks_table, "
    "size_t n_units, uint64_t in_total_max, uint64_t n_cand_max, uint32_t flags, mscomp_amd_syncer** sy);",
    "void mscomp_amd_syncer_destroy(mscomp_amd_syncer* sy);",
    "MSCompStatus mscomp_amd_syncer_sync(mscomp_amd_syncer* sy, const mscomp_amd_blocks_view* store, const uint8_t* d_in, const uint64_t* d_in_off, "
    "const uint64_t* d_in_len, uint64_t* d_hit_first, uint64_t* d_req, uint64_t* d_req_off, uint64_t* d_lit_first, uint64_t* d_lit, "
    "uint64_t* d_count, int32_t* d_res_status, int32_t* d_status);",
    "int mscomp_amd_syncer_counts(mscomp_amd_syncer* sy, uint32_t out[3]);",
)


def test_sync_symbols_are_exported_and_declared():
    import ms_compress_amd as m
    lib = m.load_library()
    hdr = R.check_declared(lib, NAMES, PROTOTYPES)
    # behind the transcoder's section, in front of the resource checksums
    assert hdr.index("mscomp_amd_transcoder_counts(") < hdr.index("mscomp_amd_syncer_create(") < hdr.index("mscomp_amd_res_crc_dev(mscomp_amd_ctx* ctx")
    section = hdr[hdr.index("/* Sync:"): hdr.index("MSCompStatus mscomp_amd_syncer_create(")]
    for part in ("Creation:", "Scratch:", "Sources:", "Rules:", "Consequence:", "Counts:", "Execution:", "Left out:"):
        assert part in section, part
    assert "MSCOMP_AMD_SCRATCH_SYNCER" not in hdr                                 # no new scratch kind
    tile = int(re.search(r"#define\s+MSCOMP_AMD_SYNC_TILE\s+(\d+)u", hdr).group(1))
    assert tile == m.MSCOMP_AMD_SYNC_TILE and tile <= 4096 and 4096 % tile == 0   # the seams the tests aim at; a tile never exceeds a block
    assert callable(m.BlockSyncer.sync) and callable(m.BlockSyncer.counts)
    assert callable(m.blocks_sync) and callable(m.blocks_sync_delta) and callable(m.blocks_sync_patch)


def test_create_argument_errors_in_order_without_gpu():
    import ms_compress_amd as m
    lib = m.load_library()
    create = lib.mscomp_amd_syncer_create
    ctx = C.c_void_p(8)                                           # never dereferenced: every check below comes before the context is used

    def status(*args):
        obj = C.c_void_p(123)
        st = create(*args, C.byref(obj))
        assert not obj.value                                      # cleared on every failure
        return st
    ok = (3, 4096, 4, 64, 2, 1 << 20, 32, 0)                      # format, block_size, n_res, n_blocks_table, n_units, in_total_max, n_cand_max, flags
    assert status(None, *ok) == m.MSCOMP_ARG_ERROR                # a null context
    assert create(ctx, *ok, None) == m.MSCOMP_ARG_ERROR           # a null out pointer
    for fmt in (0, 1, 5):
        assert status(ctx, fmt, *ok[1:]) == m.MSCOMP_ARG_ERROR, fmt
    for bs in (0, 4095, 6144, 2048, 1048576, 0x80000000):         # block_size: a power of two from 4096 to 524288
        assert status(ctx, 3, bs, *ok[2:]) == m.MSCOMP_ARG_ERROR, bs
    assert status(ctx, *ok[:7], 1) == m.MSCOMP_ARG_ERROR          # no flags
    big = 0x7FFFFFF1
    for at in (2, 3, 4, 6):                                       # n_res, n_blocks_table, n_units, n_cand_max
        assert status(ctx, *ok[:at], big, *ok[at + 1:]) == m.MSCOMP_ARG_ERROR, at
    # MSCOMP_MEM_ERROR only behind every argument check, and still before the context is used
    assert status(ctx, *ok[:5], 1 << 50, *ok[6:]) == m.MSCOMP_MEM_ERROR
    assert status(ctx, *ok[:5], 0x7FFFFFF0 * 4096, *ok[6:]) == m.MSCOMP_MEM_ERROR          # the tiles are numbered in 32 bits
    assert status(ctx, 3, 524288, 4, 64, 2, 1 << 20, 0x7FFFFFF0, 0) == m.MSCOMP_MEM_ERROR   # a cache no dev plan addresses
    assert status(ctx, *ok[:5], 1 << 50, 32, 1) == m.MSCOMP_ARG_ERROR                      # an argument error wins over a memory error
    assert status(ctx, 3, 4095, 4, 64, 2, 1 << 50, 0x7FFFFFF0, 0) == m.MSCOMP_ARG_ERROR


def test_sync_null_object():
    import ms_compress_amd as m
    lib = m.load_library()
    p = C.c_void_p(8)                                             # never dereferenced: the syncer is null
    view = m.BlocksView()
    assert lib.mscomp_amd_syncer_sync(None, C.byref(view), p, p, p, p, p, p, p, p, p, p, p) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_syncer_sync(None, None, None, None, None, None, None, None, None, None, None, None, None) == m.MSCOMP_ARG_ERROR
    out = (C.c_uint32 * 3)()
    assert lib.mscomp_amd_syncer_counts(None, out) == -1
    lib.mscomp_amd_syncer_destroy(None)                           # a no-op
