"""CPU: the five symbols of the parity object are exported, declared in the header with their prototypes and named in api.EXPORTS, the two
defines are in the header and in the package, the section has its parts and stands in its place, and the calls refuse bad arguments before
they touch a device -- in the manner of tests/test_repair_abi.py. (The refusals that need an object, and with it a device, are in
tests/test_gpu_parity_rows.py.)"""
import ctypes as C
import re

import abi_rig as R

NAMES = ("mscomp_amd_parity_create", "mscomp_amd_parity_destroy", "mscomp_amd_parity_bound", "mscomp_amd_parity_build", "mscomp_amd_parity_rebuild")
PROTOTYPES = (
    "MSCompStatus mscomp_amd_parity_create(mscomp_amd_ctx* ctx, uint32_t block_size, uint64_t n_blocks_table, uint32_t k, uint32_t m, "
    "uint32_t flags, mscomp_amd_parity** pr);",
    "void mscomp_amd_parity_destroy(mscomp_amd_parity* pr);",
    "int mscomp_amd_parity_bound(const mscomp_amd_parity* pr, uint64_t out[2]);",
    "MSCompStatus mscomp_amd_parity_build(mscomp_amd_parity* pr, const mscomp_amd_blocks_view* src, uint8_t* d_par, uint64_t par_cap, "
    "uint64_t* d_par_off, uint32_t* d_par_crc, uint32_t* d_row_len, uint64_t* d_par_head, int32_t* d_status);",
    "MSCompStatus mscomp_amd_parity_rebuild(mscomp_amd_parity* pr, const mscomp_amd_blocks_view* src, const uint32_t* d_verdict, "
    "const uint8_t* d_par, uint64_t par_len, const uint64_t* d_par_off, const uint32_t* d_par_crc, const uint32_t* d_row_len, "
    "const uint64_t* d_par_head, uint8_t* d_fix_packed, uint64_t fix_cap, uint64_t* d_fix_block_off, uint32_t* d_fix_verdict, "
    "uint64_t* d_count, int32_t* d_status);",
)
PARTS = ("Creation:", "Scratch:", "Sources:", "Notation:", "Rules:", "Consequence:", "Checksums:", "Execution:", "Left out:")
LEFT_OUT = ("d_par_off, d_par_crc, d_row_len, d_par_head", "d_block_first / d_res_len", "damaged CRC word from damaged data", "m > 3",
            "updating parity in place", "parity over the data instead of the stored form", "fusing salvage, rebuild, repair and splice")


def test_parity_symbols_are_exported_and_declared():
    import ms_compress_amd as m
    lib = m.load_library()
    hdr, flat = R.check_declared(lib, NAMES, PROTOTYPES), R.flat_header()
    for name, value in (("K_MAX", 255), ("M_MAX", 3)):
        assert re.search(r"#define MSCOMP_AMD_PARITY_%s +%du\b" % (name, value), hdr), name
        assert getattr(m, "MSCOMP_AMD_PARITY_" + name) == value
    assert "typedef struct mscomp_amd_parity mscomp_amd_parity;" in flat
    # the section's place: behind the digest syncer's call, in front of the resource checksums
    assert hdr.index("mscomp_amd_syncer_sync_digest(") < hdr.index("/* Parity:") < hdr.index("mscomp_amd_parity_create(") < hdr.index("/* Resource checksums")
    assert hdr.index("mscomp_amd_parity_rebuild(") < hdr.index("mscomp_amd_res_crc_dev(")
    section = hdr[hdr.index("/* Parity:"): hdr.index("#define MSCOMP_AMD_PARITY_K_MAX")]
    at = 0
    for part in PARTS:                                            # every part, in the order of every other section
        assert part in section[at:], part
        at = section.index(part, at)
    section = re.sub(r"\s*\n \*\s*", " ", section)                # (without its line breaks)
    left = section[section.index("Left out:"):]
    for phrase in LEFT_OUT:
        assert phrase in left, phrase
    for phrase in ("0x11D", "INTERLEAVED", "SPARSE MIRROR", "BYTE FOR BYTE", "28 bytes per parity row", "12 per row", "24 per group"):
        assert phrase in section, phrase
    assert len(re.findall(r"#define MSCOMP_AMD_SCRATCH_[A-Z]+ +\d+", hdr)) == 7 and "MSCOMP_AMD_SCRATCH_PARITY" not in hdr   # no new scratch kind
    for name in ("bound", "build", "rebuild", "fix_view"):
        assert callable(getattr(m.BlockParity, name)), name
    assert callable(m.blocks_parity) and callable(m.blocks_rebuild)


def test_create_parity_argument_errors_without_gpu():
    import ms_compress_amd as m
    lib = m.load_library()
    create = lib.mscomp_amd_parity_create
    ctx = C.c_void_p(8)                                           # never dereferenced: every check below comes before the context is used

    def answer(*args):
        obj = C.c_void_p(123)
        st = create(*args, C.byref(obj))
        assert not obj.value                                      # *pr is cleared whatever the refusal
        return st
    refused = lambda *args: answer(*args) == m.MSCOMP_ARG_ERROR
    assert refused(None, 4096, 64, 4, 2, 0)                       # a null context
    assert create(ctx, 4096, 64, 4, 2, 0, None) == m.MSCOMP_ARG_ERROR               # a null out pointer
    for bs in (0, 4095, 6144, 2048, 1048576, 0x80000000):         # block_size: a power of two from 4096 to 524288
        assert refused(ctx, bs, 64, 4, 2, 0), bs
    for k in (0, 256, 0xFFFFFFFF):
        assert refused(ctx, 4096, 64, k, 2, 0), k
    for mm in (0, 4, 0xFFFFFFFF):
        assert refused(ctx, 4096, 64, 4, mm, 0), mm
    assert refused(ctx, 65536, 64, 4, 2, 1)                       # no flags
    assert refused(ctx, 4096, 0x7FFFFFF1, 4, 2, 0) and refused(ctx, 4096, 1 << 40, 255, 1, 0)
    assert answer(ctx, 4096, 0x7FFFFFF0, 1, 3, 0) == m.MSCOMP_MEM_ERROR             # more parity rows than the CRC kernels count: before the context is used


def test_parity_null_objects():
    import ms_compress_amd as m
    lib = m.load_library()
    p = C.c_void_p(8)                                             # never dereferenced: the object is null
    views = (m.BlocksView * 1)()
    out = (C.c_uint64 * 2)(7, 7)
    assert lib.mscomp_amd_parity_build(None, views, p, 64, p, p, p, p, p) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_parity_build(None, None, None, 0, None, None, None, None, None) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_parity_rebuild(None, views, p, p, 64, p, p, p, p, p, 64, p, p, p, p) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_parity_rebuild(None, None, None, None, 0, None, None, None, None, None, 0, None, None, None, None) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_parity_bound(None, out) == -1 and list(out) == [7, 7]
    lib.mscomp_amd_parity_destroy(None)                           # as every destroy: nothing to do
