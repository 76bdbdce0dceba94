"""CPU: the three symbols of salvage and repair are exported, declared in the header with their prototypes and named in api.EXPORTS, the
five verdicts are in the header and in the package, and the calls refuse bad arguments before they touch a device -- in the manner of
tests/test_diff_abi.py. (The refusals that need a container or a deduper, and with it a device, are in tests/test_gpu_repair.py.)"""
import ctypes as C
import re

import abi_rig as R

NAMES = ("mscomp_amd_blocks_salvage", "mscomp_amd_deduper_create_repair", "mscomp_amd_deduper_repair")
PROTOTYPES = (
    "MSCompStatus mscomp_amd_blocks_salvage(mscomp_amd_blocks* bk, const uint8_t* d_packed, uint64_t packed_len, "
    "const uint64_t* d_block_first, const uint64_t* d_block_off, const uint64_t* d_res_len, const uint32_t* d_block_crc, const uint32_t* d_only, "
    "uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap, uint64_t* d_out_len, uint32_t* d_bad, uint32_t* d_verdict, "
    "uint64_t* d_count, int32_t* d_status);",
    "MSCompStatus mscomp_amd_deduper_create_repair(mscomp_amd_ctx* ctx, uint32_t block_size, uint32_t n_src, size_t n_res, "
    "uint64_t n_blocks_new, uint32_t flags, mscomp_amd_deduper** dd);",
    "MSCompStatus mscomp_amd_deduper_repair(mscomp_amd_deduper* dd, const mscomp_amd_blocks_view* src, const uint32_t* const* d_verdict, "
    "uint64_t* d_ext_first, uint64_t* d_ext, uint64_t* d_fixed, uint64_t* d_lost, uint64_t* d_count, int32_t* d_status);",
)
VERDICTS = (("GOOD", 0), ("TABLE", 1), ("DECODE", 2), ("CRC", 3), ("SKIPPED", 4))
PARTS = ("Creation:", "Scratch:", "Sources:", "Notation:", "Rules:", "Consequence:", "Checksums:", "Execution:", "Left out:")


def test_repair_symbols_are_exported_and_declared():
    import ms_compress_amd as m
    lib = m.load_library()
    hdr = R.check_declared(lib, NAMES, PROTOTYPES)
    for name, value in VERDICTS:
        assert re.search(r"#define MSCOMP_AMD_BLOCK_%s +%du\b" % (name, value), hdr), name
        assert getattr(m, "MSCOMP_AMD_BLOCK_" + name) == value
    assert hdr.index("mscomp_amd_blocks_check(") < hdr.index("mscomp_amd_blocks_salvage(") < hdr.index("mscomp_amd_reader_create(")   # the container's fifth call
    assert hdr.index("mscomp_amd_deduper_match(") < hdr.index("mscomp_amd_deduper_create_repair(") < hdr.index("mscomp_amd_res_crc_dev(")   # behind the deduper's third
    salvage = hdr[hdr.index("/* Salvage:"): hdr.index("#define MSCOMP_AMD_BLOCK_GOOD")]
    repair = hdr[hdr.index("/* Repair:"): hdr.index("MSCompStatus mscomp_amd_deduper_create_repair(")]
    for part in PARTS:
        assert part in salvage and part in repair, part
    for left in ("damaged CRC word from damaged data", "byte-granular salvage", "block_first", "fusing salvage, repair and splice", "more than three mirrors"):
        assert left in repair[repair.index("Left out:"):], left
    assert "#define MSCOMP_AMD_SCRATCH_DEDUPER 6" in hdr and "MSCOMP_AMD_SCRATCH_REPAIR" not in hdr and "MSCOMP_AMD_SCRATCH_SALVAGE" not in hdr
    assert len(re.findall(r"#define MSCOMP_AMD_SCRATCH_[A-Z]+ +\d+", hdr)) == 7                      # no new scratch kind
    assert "68 bytes of tables per possible block + 28 per resource" in hdr                           # salvage reserves nothing more
    assert callable(m.BlockContainer.salvage) and callable(m.BlockDeduper.for_repair) and callable(m.BlockDeduper.repair)
    assert callable(m.blocks_salvage) and callable(m.blocks_repair)


def test_create_repair_argument_errors_without_gpu():
    import ms_compress_amd as m
    lib = m.load_library()
    create = lib.mscomp_amd_deduper_create_repair
    ctx = C.c_void_p(8)                                           # never dereferenced: every check below comes before the context is used

    def refused(*args):
        obj = C.c_void_p(123)
        return create(*args, C.byref(obj)) == m.MSCOMP_ARG_ERROR and not obj.value
    assert refused(None, 4096, 2, 4, 64, 0)                       # a null context
    assert create(ctx, 4096, 2, 4, 64, 0, None) == m.MSCOMP_ARG_ERROR               # a null out pointer
    for bs in (0, 4095, 6144, 2048, 1048576, 0x80000000):         # block_size: a power of two from 4096 to 524288
        assert refused(ctx, bs, 2, 4, 64, 0), bs
    for n_src in (0, 5, 0xFFFFFFFF):                              # one primary and at most three mirrors
        assert refused(ctx, 4096, n_src, 4, 64, 0), n_src
    assert refused(ctx, 65536, 2, 4, 64, 1)                       # no flags
    big = 0x7FFFFFF1
    assert refused(ctx, 4096, 2, big, 64, 0) and refused(ctx, 4096, 2, 4, big, 0) and refused(ctx, 524288, 4, 4, 1 << 40, 0)


def test_repair_null_objects():
    import ms_compress_amd as m
    lib = m.load_library()
    p = C.c_void_p(8)                                             # never dereferenced: the object is null
    views = (m.BlocksView * 2)()
    q = (C.c_void_p * 2)(8, 8)
    assert lib.mscomp_amd_deduper_repair(None, views, q, p, p, p, p, p, p) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_deduper_repair(None, None, None, None, None, None, None, None, None) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_blocks_salvage(None, p, 64, p, p, p, p, p, p, p, p, p, p, p, p, p) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_blocks_salvage(None, None, 0, *([None] * 13)) == m.MSCOMP_ARG_ERROR
