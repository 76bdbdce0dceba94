"""CPU: the six symbols of the block digests -- the digester's four and the digest syncer's two -- are exported, declared in the header
with their prototypes and named in api.EXPORTS, and both creates refuse bad arguments before they touch a device -- in the manner of
tests/test_sync_abi.py. (The refusals of a call that need an object, and with it a device, are in tests/test_gpu_digest.py.)"""
import ctypes as C
import re

import abi_rig as R

NAMES = ("mscomp_amd_digester_create", "mscomp_amd_digester_destroy", "mscomp_amd_digester_blocks", "mscomp_amd_digester_check",
         "mscomp_amd_syncer_create_digest", "mscomp_amd_syncer_sync_digest")
PROTOTYPES = (
    "MSCompStatus mscomp_amd_digester_create(mscomp_amd_ctx* ctx, uint32_t block_size, size_t n_res, uint64_t in_total_max, uint32_t flags, "
    "mscomp_amd_digester** dg);",
    "void mscomp_amd_digester_destroy(mscomp_amd_digester* dg);",
    "MSCompStatus mscomp_amd_digester_blocks(mscomp_amd_digester* dg, const uint8_t* d_data, const uint64_t* d_res_off, const uint64_t* d_res_len, "
    "uint32_t* d_block_digest, int32_t* d_status);",
    "MSCompStatus mscomp_amd_digester_check(mscomp_amd_digester* dg, const uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_res_len, "
    "const uint64_t* d_block_first, const uint64_t* d_range, const uint32_t* d_block_digest, uint64_t* d_out_len, int32_t* d_status);",
    "MSCompStatus mscomp_amd_syncer_create_digest(mscomp_amd_ctx* ctx, uint32_t block_size, size_t n_res, uint64_t n_blocks_table, "
    "size_t n_units, uint64_t in_total_max, uint64_t n_cand_max, uint32_t flags, mscomp_amd_syncer** sy);",
    "MSCompStatus mscomp_amd_syncer_sync_digest(mscomp_amd_syncer* sy, const mscomp_amd_blocks_view* store, const uint32_t* d_block_digest, "
    "const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len, uint64_t* d_hit_first, uint64_t* d_req, uint64_t* d_req_off, "
    "uint64_t* d_lit_first, uint64_t* d_lit, uint64_t* d_count, int32_t* d_res_status, int32_t* d_status);",
)


def test_digest_symbols_are_exported_and_declared():
    import ms_compress_amd as m
    lib = m.load_library()
    hdr = R.check_declared(lib, NAMES, PROTOTYPES)
    # behind the syncer's section, in front of the resource checksums
    assert hdr.index("mscomp_amd_syncer_counts(") < hdr.index("/* Digests:") < hdr.index("mscomp_amd_digester_create(") < hdr.index("/* Resource checksums")
    section = hdr[hdr.index("/* Digests:"): hdr.index("MSCompStatus mscomp_amd_digester_create(")]
    for part in ("Creation:", "Scratch:", "Sources:", "Rules:", "Consequence:", "Execution:", "Left out:"):
        assert part in section, part
    for word in ("BLAKE2s", "RFC 7693", "16 block_size / 1024 + 56", "16 block_size / 1024 + 32", "never dereferenced", "keyed digests"):
        assert word in section, word
    assert "MSCOMP_AMD_SCRATCH_DIGESTER" not in hdr                               # no new scratch kind
    leaf = int(re.search(r"#define\s+MSCOMP_AMD_DIGEST_LEAF\s+(\d+)u", hdr).group(1))
    assert leaf == m.MSCOMP_AMD_DIGEST_LEAF == 1024
    # the view's layout is ABI: the digest column travels as an argument of its own
    assert [f for f, _ in m.BlocksView._fields_] == ["d_packed", "packed_len", "d_block_first", "d_block_off", "d_res_len", "d_block_crc", "n_res", "n_blocks_table"]
    assert callable(m.BlockDigester.blocks) and callable(m.BlockDigester.check) and callable(m.blocks_digest)
    assert callable(m.BlockSyncer.for_digest) and callable(m.BlockSyncer.sync_digest)


def _status(create, *args):
    obj = C.c_void_p(123)
    st = create(*args, C.byref(obj))
    assert not obj.value                                          # cleared on every failure
    return st


def test_digester_create_argument_errors_in_order_without_gpu():
    import ms_compress_amd as m
    create = m.load_library().mscomp_amd_digester_create
    ctx = C.c_void_p(8)                                           # never dereferenced: every check below comes before the context is used
    ok = (4096, 4, 1 << 20, 0)                                    # block_size, n_res, in_total_max, flags
    assert _status(create, None, *ok) == m.MSCOMP_ARG_ERROR       # a null context
    assert create(ctx, *ok, None) == m.MSCOMP_ARG_ERROR           # a null out pointer
    for bs in (0, 4095, 6144, 2048, 1048576, 0x80000000):         # block_size: a power of two from 4096 to 524288
        assert _status(create, ctx, bs, *ok[1:]) == m.MSCOMP_ARG_ERROR, bs
    assert _status(create, ctx, *ok[:3], 1) == m.MSCOMP_ARG_ERROR   # no flags
    assert _status(create, ctx, 4096, 0x7FFFFFF1, 1 << 20, 0) == m.MSCOMP_ARG_ERROR
    # MSCOMP_MEM_ERROR only behind every argument check, and still before the context is used
    assert _status(create, ctx, 4096, 4, 1 << 50, 0) == m.MSCOMP_MEM_ERROR
    assert _status(create, ctx, 4096, 4, 0x7FFFFFF0 * 4096, 0) == m.MSCOMP_MEM_ERROR       # n_blocks_max = n_res + in_total_max / B
    assert _status(create, ctx, 524288, 0x7FFFFFF0, 524288, 0) == m.MSCOMP_MEM_ERROR
    assert _status(create, ctx, 4096, 4, 1 << 50, 1) == m.MSCOMP_ARG_ERROR                 # an argument error wins over a memory error
    assert _status(create, ctx, 4095, 4, 1 << 50, 0) == m.MSCOMP_ARG_ERROR


def test_digest_syncer_create_argument_errors_in_order_without_gpu():
    import ms_compress_amd as m
    create = m.load_library().mscomp_amd_syncer_create_digest
    ctx = C.c_void_p(8)
    ok = (4096, 4, 64, 2, 1 << 20, 32, 0)                         # block_size, n_res, n_blocks_table, n_units, in_total_max, n_cand_max, flags
    assert _status(create, None, *ok) == m.MSCOMP_ARG_ERROR
    assert create(ctx, *ok, None) == m.MSCOMP_ARG_ERROR
    for bs in (0, 4095, 6144, 2048, 1048576, 0x80000000):
        assert _status(create, ctx, bs, *ok[1:]) == m.MSCOMP_ARG_ERROR, bs
    assert _status(create, ctx, *ok[:6], 1) == m.MSCOMP_ARG_ERROR
    big = 0x7FFFFFF1
    for at in (1, 2, 3, 5):                                       # n_res, n_blocks_table, n_units, n_cand_max
        assert _status(create, ctx, *ok[:at], big, *ok[at + 1:]) == m.MSCOMP_ARG_ERROR, at
    assert _status(create, ctx, *ok[:4], 1 << 50, *ok[5:]) == m.MSCOMP_MEM_ERROR
    assert _status(create, ctx, *ok[:4], 0x7FFFFFF0 * 4096, *ok[5:]) == m.MSCOMP_MEM_ERROR   # the tiles are numbered in 32 bits
    assert _status(create, ctx, *ok[:4], 1 << 50, 32, 1) == m.MSCOMP_ARG_ERROR             # an argument error wins over a memory error
    assert _status(create, ctx, 4095, 4, 64, 2, 1 << 50, 32, 0) == m.MSCOMP_ARG_ERROR


def test_null_objects():
    import ms_compress_amd as m
    lib = m.load_library()
    p = C.c_void_p(8)                                             # never dereferenced: the object is null
    view = m.BlocksView()
    assert lib.mscomp_amd_digester_blocks(None, p, p, p, p, p) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_digester_check(None, p, p, p, p, p, p, p, p) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_syncer_sync_digest(None, C.byref(view), p, p, p, p, p, p, p, p, p, p, p, p) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_syncer_sync_digest(None, None, None, None, None, None, None, None, None, None, None, None, None, None) == m.MSCOMP_ARG_ERROR
    lib.mscomp_amd_digester_destroy(None)                         # a no-op
