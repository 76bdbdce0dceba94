"""The C ABI of libmscomp_amd.so as Python sees it: the constants of the two headers, SIGNATURES (every export, once), the two ctypes
structures, and load_library(), which opens the library and binds every export to its signature. tests/test_binding.py holds this file to
include/mscomp_amd.h. Nothing here touches a device or imports torch at import time, and nothing that calls an export belongs here."""
import ctypes as C
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MSCOMP_AMD_LIB") or os.path.join(HERE, "libmscomp_amd.so")   # (MSCOMP_AMD_LIB: a development build of the same library, e.g. with a *_PROFILE macro)

# enum values identical to /root/reference/include/mscomp/general.h:65-85
MSCOMP_NONE, MSCOMP_RESERVED, MSCOMP_LZNT1, MSCOMP_XPRESS, MSCOMP_XPRESS_HUFF = 0, 1, 2, 3, 4
MSCOMP_OK, MSCOMP_ERRNO, MSCOMP_ARG_ERROR, MSCOMP_DATA_ERROR, MSCOMP_MEM_ERROR, MSCOMP_BUF_ERROR = 0, -1, -2, -3, -4, -5
FORMATS = {"lznt1": MSCOMP_LZNT1, "xpress": MSCOMP_XPRESS, "xpress_huff": MSCOMP_XPRESS_HUFF}
CHUNK = {MSCOMP_LZNT1: 4096, MSCOMP_XPRESS: 65536, MSCOMP_XPRESS_HUFF: 65536}

# The C ABI, once: every function include/mscomp_amd.h declares, in its order, as "return type:argument types" in the codes of _CODES
# below (a number repeats the letter before it: "v4" is "vvvv"). tests/test_binding.py holds every entry to the header's prototype.
SIGNATURES = {
    "ms_compress":                              "i:ivzvZ",
    "ms_max_compressed_size":                   "z:iz",
    "lznt1_compress":                           "i:vzvZ",
    "lznt1_max_compressed_size":                "z:z",
    "xpress_compress":                          "i:vzvZ",
    "xpress_max_compressed_size":               "z:z",
    "xpress_huff_compress":                     "i:vzvZ",
    "xpress_huff_max_compressed_size":          "z:z",
    "ms_decompress":                            "i:ivzvZ",
    "lznt1_decompress":                         "i:vzvZ",
    "xpress_decompress":                        "i:vzvZ",
    "xpress_huff_decompress":                   "i:vzvZ",
    "ms_deflate_init":                          "i:iv",
    "ms_deflate":                               "i:vi",
    "ms_deflate_end":                           "i:v",
    "lznt1_deflate_init":                       "i:v",
    "lznt1_deflate":                            "i:vi",
    "lznt1_deflate_end":                        "i:v",
    "xpress_deflate_init":                      "i:v",
    "xpress_deflate":                           "i:vi",
    "xpress_deflate_end":                       "i:v",
    "xpress_inflate_init":                      "i:v",
    "xpress_inflate":                           "i:v",
    "xpress_inflate_end":                       "i:v",
    "ms_inflate_init":                          "i:iv",
    "ms_inflate":                               "i:v",
    "ms_inflate_end":                           "i:v",
    "lznt1_inflate_init":                       "i:v",
    "lznt1_inflate":                            "i:v",
    "lznt1_inflate_end":                        "i:v",
    "mscomp_amd_ctx_create":                    "i:ivH",
    "mscomp_amd_ctx_destroy":                   "-:v",
    "mscomp_amd_plan_create":                   "i:vizv4H",
    "mscomp_amd_plan_destroy":                  "-:v",
    "mscomp_amd_plan_execute":                  "i:v5",
    "mscomp_amd_compress_units_host":           "i:iivzv6",
    "mscomp_amd_decompress_units_host":         "i:iivzv6",
    "mscomp_amd_host_pool_release":             "-:",
    "mscomp_amd_compress_batch":                "i:vizv8",
    "mscomp_amd_plan_create_decompress":        "i:vizv4H",
    "mscomp_amd_decompress_batch":              "i:vizv8",
    "mscomp_amd_plan_create_size":              "i:vizvvvH",
    "mscomp_amd_plan_execute_size":             "i:v5",
    "mscomp_amd_decompressed_size_batch":       "i:vizv7",
    "mscomp_amd_plan_create_decompress_dev":    "i:vizqqH",
    "mscomp_amd_plan_execute_dev":              "i:v9",
    "mscomp_amd_layout_dev":                    "i:vzvqv",
    "mscomp_amd_plan_create_size_dev":          "i:vizqH",
    "mscomp_amd_plan_execute_size_dev":         "i:v8",
    "mscomp_amd_plan_create_decompress_dev_ex": "i:vizqquH",
    "mscomp_amd_plan_create_size_dev_ex":       "i:vizquH",
    "mscomp_amd_plan_create_compress_dev":      "i:vizqqH",
    "mscomp_amd_plan_layout_dev":               "i:vizvqvv",
    "mscomp_amd_plan_layout":                   "q:izvqvv",
    "mscomp_amd_compact_batch":                 "i:vzv6",
    "mscomp_amd_compact_dev":                   "i:vzvvvqvqv",
    "mscomp_amd_plan_create_crc_dev":           "i:vzqH",
    "mscomp_amd_plan_execute_crc_dev":          "i:v6",
    "mscomp_amd_blocks_create":                 "i:viuzquH",
    "mscomp_amd_blocks_destroy":                "-:v",
    "mscomp_amd_blocks_bound":                  "q:v",
    "mscomp_amd_blocks_compress":               "i:v5qvvv",
    "mscomp_amd_blocks_decompress":             "i:vvqv9",
    "mscomp_amd_blocks_crc":                    "i:v7",
    "mscomp_amd_blocks_check":                  "i:v9",
    "mscomp_amd_blocks_salvage":                "i:vvqv13",
    "mscomp_amd_reader_create":                 "i:viuzqzquH",
    "mscomp_amd_reader_destroy":                "-:v",
    "mscomp_amd_reader_read":                   "i:vvqv10",
    "mscomp_amd_reader_counts":                 "i:vU",
    "mscomp_amd_writer_create":                 "i:viuzqzquH",
    "mscomp_amd_writer_destroy":                "-:v",
    "mscomp_amd_writer_write":                  "i:vvqv8qv5",
    "mscomp_amd_writer_counts":                 "i:vU",
    "mscomp_amd_writer_resize":                 "i:vvqv6qv5",
    "mscomp_amd_splicer_create":                "i:vuuzquH",
    "mscomp_amd_splicer_destroy":               "-:v",
    "mscomp_amd_splicer_splice":                "i:vBvvqv5",
    "mscomp_amd_splicer_create_extents":        "i:vuuzzquH",
    "mscomp_amd_splicer_splice_extents":        "i:vBvvvqv5",
    "mscomp_amd_deduper_create":                "i:vuuzquH",
    "mscomp_amd_deduper_destroy":               "-:v",
    "mscomp_amd_deduper_dedup":                 "i:vBv5",
    "mscomp_amd_deduper_create_diff":           "i:vuzquH",
    "mscomp_amd_deduper_diff":                  "i:vBBv8",
    "mscomp_amd_deduper_create_match":          "i:vuuzqquH",
    "mscomp_amd_deduper_match":                 "i:vBBv7",
    "mscomp_amd_deduper_create_repair":         "i:vuuzquH",
    "mscomp_amd_deduper_repair":                "i:vBHv6",
    "mscomp_amd_transcoder_create":             "i:viuiuzqqquH",
    "mscomp_amd_transcoder_destroy":            "-:v",
    "mscomp_amd_transcoder_transcode":          "i:vvqv5qv4",
    "mscomp_amd_transcoder_counts":             "i:vU",
    "mscomp_amd_syncer_create":                 "i:viuzqzqquH",
    "mscomp_amd_syncer_destroy":                "-:v",
    "mscomp_amd_syncer_sync":                   "i:vBv11",
    "mscomp_amd_syncer_counts":                 "i:vU",
    "mscomp_amd_digester_create":               "i:vuzquH",
    "mscomp_amd_digester_destroy":              "-:v",
    "mscomp_amd_digester_blocks":               "i:v6",
    "mscomp_amd_digester_check":                "i:v9",
    "mscomp_amd_syncer_create_digest":          "i:vuzqzqquH",
    "mscomp_amd_syncer_sync_digest":            "i:vBv12",
    "mscomp_amd_parity_create":                 "i:vuquuuH",
    "mscomp_amd_parity_destroy":                "-:v",
    "mscomp_amd_parity_bound":                  "i:vQ",
    "mscomp_amd_parity_build":                  "i:vBvqv5",
    "mscomp_amd_parity_rebuild":                "i:vBvvqv5qv4",
    "mscomp_amd_res_crc_dev":                   "i:vuzqv5",
    "mscomp_amd_profile_enable":                "-:vi",
    "mscomp_amd_profile_read":                  "i:v4i",
    "mscomp_amd_debug_xpress_matches":          "i:vvzuivv",
    "mscomp_amd_debug_huff_lengths":            "i:vvzv",
    "mscomp_amd_debug_huff_lengths_slow":       "i:vvzv",
    "mscomp_amd_debug_hooks_enabled":           "i:",
    "mscomp_amd_debug_set_xpress_emit":         "-:i",
    "mscomp_amd_set_lznt1_sa_dict":             "-:i",
    "mscomp_amd_get_lznt1_sa_dict":             "i:",
    "mscomp_amd_ctx_set_lznt1_sa_dict":         "i:vi",
    "mscomp_amd_debug_set_xpress_decoder":      "-:i",
    "mscomp_amd_debug_lzg_open":                "i:vqv",
    "mscomp_amd_debug_set_finder":              "-:i",
    "mscomp_amd_debug_set_one_shot":            "-:i",
    "mscomp_amd_debug_set_lznt1":               "-:i",
    "mscomp_amd_debug_set_place_blocks":        "-:i",
    "mscomp_amd_debug_lzd_walked":              "u:v",
    "mscomp_amd_debug_decode_modes":            "i:vvz",
    "mscomp_amd_debug_plan_paths":              "i:vU",
    "mscomp_amd_debug_scratch_names":           "i:Si",
    "mscomp_amd_debug_scratch_poison":          "i:ivii",
    "mscomp_amd_debug_scratch_report":          "i:iviRi",
    "mscomp_amd_debug_lds_lane_order":          "u:vu4",
    "mscomp_amd_debug_alignbyte":               "u:vu",
    "mscomp_amd_debug_set_serial_atomics":      "-:i",
    "mscomp_amd_version":                       "s:",
}
EXPORTS = list(SIGNATURES)  # every symbol include/mscomp_amd.h declares (tests check the library exports all of them)
MSCOMP_AMD_SPLICE_SRC_MAX = 4
MSCOMP_AMD_SPLICE_ROW_TILE = 1024                              # rows of the new table per workgroup of splice_extents' row passes
MSCOMP_AMD_SYNC_TILE = 4096                                    # positions per wave of a syncer's scan: its seams
MSCOMP_AMD_DIGEST_LEAF = 1024                                  # bytes per leaf of a block digest's tree
MSCOMP_AMD_PARITY_K_MAX, MSCOMP_AMD_PARITY_M_MAX = 255, 3           # members and parity rows per group of a BlockParity
MSCOMP_AMD_DEV_LARGE_UNITS = 1
MSCOMP_AMD_DIFF_NO_BASE = (1 << 64) - 1                        # the base resource of a diff pair whose new resource has none
# the verdict of a row (BlockContainer.salvage): good; refused by its table entries; did not decode; decoded to other bytes; not judged
MSCOMP_AMD_BLOCK_GOOD, MSCOMP_AMD_BLOCK_TABLE, MSCOMP_AMD_BLOCK_DECODE, MSCOMP_AMD_BLOCK_CRC, MSCOMP_AMD_BLOCK_SKIPPED = 0, 1, 2, 3, 4


class ScratchRec(C.Structure):
    """mscomp_amd_scratch_rec: one buffer of a scratch report"""
    _fields_ = [("name", C.c_char_p), ("asked", C.c_uint64), ("cap", C.c_uint64), ("changed", C.c_uint64)]


class BlocksView(C.Structure):
    """mscomp_amd_blocks_view: one source container of a splice, as device addresses"""
    _fields_ = [("d_packed", C.c_void_p), ("packed_len", C.c_uint64), ("d_block_first", C.c_void_p), ("d_block_off", C.c_void_p),
                ("d_res_len", C.c_void_p), ("d_block_crc", C.c_void_p), ("n_res", C.c_uint64), ("n_blocks_table", C.c_uint64)]


# the type codes of SIGNATURES: scalars (int and the enums; size_t; uint64_t; uint32_t), void and const char* as return types, an untyped
# pointer (lower case), and the typed pointers a caller passes a ctypes array, structure or byref() for (upper case)
_CODES = {"i": C.c_int, "z": C.c_size_t, "q": C.c_uint64, "u": C.c_uint32, "-": None, "s": C.c_char_p, "v": C.c_void_p,
          "H": C.POINTER(C.c_void_p), "B": C.POINTER(BlocksView), "R": C.POINTER(ScratchRec), "U": C.POINTER(C.c_uint32),
          "Q": C.POINTER(C.c_uint64), "S": C.POINTER(C.c_char_p), "Z": C.POINTER(C.c_size_t)}


def signature(name):
    """(restype, argtypes) of an export, as ctypes classes, from SIGNATURES"""
    ret, _, args = SIGNATURES[name].partition(":")
    return _CODES[ret], [_CODES[c] for c, n in re.findall(r"(\D)(\d*)", args) for _ in range(int(n or 1))]


class MSCompError(RuntimeError):
    def __init__(self, status, what=""):
        super().__init__("mscomp status %d %s" % (status, what))
        self.status = status


_lib = None


def load_library():
    """Load libmscomp_amd.so. Fails loudly when the HIP extension has not been built (no fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
    try:                      # PyTorch bundles its own libamdhip64; this library links /opt/rocm's. Both live in one process, and the
        import torch  # noqa: F401   device is only visible to both when torch's runtime was loaded first (seen on the MI355X box).
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name in SIGNATURES:
        if hasattr(lib, name):                 # (build() and tests/test_abi.py report a symbol the library lacks; calling it raises)
            f = getattr(lib, name)
            f.restype, f.argtypes = signature(name)
    _lib = lib
    return lib
