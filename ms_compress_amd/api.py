"""Host-side binding of libmscomp_amd.so (the C-ABI declared in include/mscomp_amd.h).

Mirrors the reference's own ctypes fixture (/root/reference/test/compressors.py:187-251: ``OpenSrc.Compress`` ->
``ms_compress``; default output buffer, status codes) so that the parity tests read like the reference's tests,
and adds the batch interface (device-resident units) the GPU path needs.

PyTorch is plumbing only: device memory (``torch.empty(..., device="cuda")``), the current HIP stream and
``torch.distributed``. There is NO CPU encoder behind these functions: if the HIP extension is missing or no
GPU is visible they raise.
"""
import contextlib
import ctypes as C
import os
import re
import weakref

import numpy as np

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


def max_compressed_size(fmt, n):
    """ms_max_compressed_size (/root/reference/src/mscomp.cpp:96-100)."""
    return load_library().ms_max_compressed_size(int(fmt), int(n))


def compress(fmt, data, out_capacity=None):
    """One-shot ``ms_compress`` with HOST buffers (the reference contract, mscomp.h:59): returns the compressed
    bytes or raises MSCompError(status). Default capacity follows compressors.py:248 / ms_max_compressed_size."""
    lib = load_library()
    data = bytes(data)
    cap = max_compressed_size(fmt, len(data)) if out_capacity is None else int(out_capacity)
    out = C.create_string_buffer(cap + 2)
    n = C.c_size_t(cap)
    st = lib.ms_compress(int(fmt), data, len(data), out, C.byref(n))
    if st != MSCOMP_OK:
        raise MSCompError(st, "ms_compress(format=%d, in_len=%d, capacity=%d)" % (fmt, len(data), cap))
    return out.raw[: n.value]


def decompress(fmt, data, out_capacity):
    """One-shot ``ms_decompress`` with HOST buffers (mscomp.h:79): ``out_capacity`` is what the caller passes in *out_len.
    Returns the decompressed bytes or raises MSCompError(status)."""
    lib = load_library()
    data = bytes(data)
    cap = int(out_capacity)
    out = C.create_string_buffer(cap + 1)
    n = C.c_size_t(cap)
    st = lib.ms_decompress(int(fmt), data, len(data), out, C.byref(n))
    if st != MSCOMP_OK:
        raise MSCompError(st, "ms_decompress(format=%d, in_len=%d, capacity=%d)" % (fmt, len(data), cap))
    return out.raw[: n.value]


def pack_offsets(lengths, align=16):
    """Start offsets (n entries, uint64) of units of the given byte lengths packed back to back with every start
    aligned, and the total size. """
    off = np.zeros(len(lengths), dtype=np.uint64)
    pos = 0
    for i, n in enumerate(lengths):
        off[i] = pos
        pos += (int(n) + align - 1) // align * align
    return off, pos


class Context:
    """mscomp_amd_ctx: one per (device, stream). Uses torch's current device/stream by default."""

    def __init__(self, device=None, stream=None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible: ms_compress_amd has no CPU fallback")
        self.lib = load_library()
        self.device = torch.cuda.current_device() if device is None else int(device)
        with torch.cuda.device(self.device):
            s = torch.cuda.current_stream() if stream is None else stream
        self.stream = s
        self._h = C.c_void_p()
        self._handles = weakref.WeakSet()                  # the plans and block objects that live in this context (_Handle)
        _run(self, "mscomp_amd_ctx_create", self.device, C.c_void_p(s.cuda_stream), C.byref(self._h))

    def close(self):
        """Destroys the context, and first whatever still lives in it: an object's destroy call reads its context."""
        if self._h:
            for h in list(self._handles):
                h.close()
            self.lib.mscomp_amd_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_lznt1_sa_dict(self, on):
        """LZNT1 dictionary flavour of the plans this context creates from now on: True / False, None = the process default."""
        _run(self, "mscomp_amd_ctx_set_lznt1_sa_dict", self._h, -1 if on is None else int(bool(on)))

    def profile_enable(self, on=True):
        self.lib.mscomp_amd_profile_enable(self._h, 1 if on else 0)

    def profile_read(self):
        """{kernel name: (total ms, launches)} since the last read (synchronizes the stream)."""
        cap = 64
        names = (C.c_char_p * cap)()
        ms = (C.c_double * cap)()
        cnt = (C.c_uint64 * cap)()
        n = self.lib.mscomp_amd_profile_read(self._h, names, ms, cnt, cap)
        return {names[i].decode(): (ms[i], cnt[i]) for i in range(n)}


def _run(ctx, export, *args):
    """Calls ``export`` of the context's library with ``args`` in the prototype's order: a torch tensor goes as its data pointer, None as
    NULL, ints and ctypes values as they are. Raises MSCompError(status, export) unless the status is MSCOMP_OK."""
    st = getattr(ctx.lib, export)(*[C.c_void_p(a.data_ptr()) if hasattr(a, "data_ptr") else a for a in args])
    if st != MSCOMP_OK:
        raise MSCompError(st, export)


@contextlib.contextmanager
def _call(ctx, enter=True):
    """The frame of a host convenience: ``ctx`` or, for None, a Context of its own that is closed on the way out; the context's device and
    stream are torch's current ones inside (not with ``enter`` False: a wrapper whose inner calls enter them). Yields (ctx, torch device)."""
    import torch
    own = ctx is None
    ctx = ctx or Context()
    dev = torch.device("cuda", ctx.device)
    try:
        if enter:
            with torch.cuda.device(ctx.device), torch.cuda.stream(ctx.stream):
                yield ctx, dev
        else:
            yield ctx, dev
    finally:
        if own:
            ctx.close()


def _three_counts(obj, export):
    """the three uint32 counters ``export`` reads from the object ``obj`` (the call synchronizes the stream)"""
    out = (C.c_uint32 * 3)()
    _run(obj.ctx, export, obj._h, out)         # (these answer 0 or MSCOMP_ERRNO)
    return (int(out[0]), int(out[1]), int(out[2]))


def _byte_bounds(d_packed=None, packed_len=None, d_new_packed=None, new_cap=None):
    """(packed_len, new_cap) as a call passes them on: each defaults to all of its tensor (0 without one), and a new_cap beyond
    d_new_packed is refused."""
    plen = (0 if d_packed is None else d_packed.numel()) if packed_len is None else int(packed_len)
    cap = (0 if d_new_packed is None else d_new_packed.numel()) if new_cap is None else int(new_cap)
    if d_new_packed is not None and cap > d_new_packed.numel():
        raise ValueError("new_cap exceeds d_new_packed")
    return plen, cap


class _Handle:
    """An object of the library that lives in a context: ``ctx``, the handle ``_h`` and the export that destroys it."""
    _destroy = "mscomp_amd_plan_destroy"

    def __init__(self, ctx):
        self.ctx, self._h = ctx, C.c_void_p()
        ctx._handles.add(self)

    def _make(self, export, *args):
        """the create call ``export(ctx, *args, &handle)``"""
        _run(self.ctx, export, self.ctx._h, *args, C.byref(self._h))

    def _run(self, export, *args):
        """the call ``export(handle, *args)``: _run above"""
        _run(self.ctx, export, self._h, *args)

    def close(self):
        if self._h:
            getattr(self.ctx.lib, self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Plan(_Handle):
    """mscomp_amd_plan: the unit layout of one batch (offset tables uploaded once, scratch sized once)."""

    def __init__(self, ctx, fmt, in_off, in_len, out_off, out_cap, decompress=False):
        _Handle.__init__(self, ctx)
        self.fmt = int(fmt)
        arrs = [np.ascontiguousarray(a, dtype=np.uint64) for a in (in_off, in_len, out_off, out_cap)]
        assert all(a.ndim == 1 and a.shape == arrs[0].shape for a in arrs)
        self.in_off, self.in_len, self.out_off, self.out_cap = arrs
        self.n_units = len(self.in_off)
        self._make("mscomp_amd_plan_create_decompress" if decompress else "mscomp_amd_plan_create", self.fmt, self.n_units, *[a.ctypes.data for a in arrs])

    def execute(self, d_in, d_out, d_out_len, d_status):
        """Enqueue on the ctx stream. Arguments are torch CUDA tensors (uint8, uint8, int64/uint64[n], int32[n])."""
        self._run("mscomp_amd_plan_execute", d_in, d_out, d_out_len, d_status)


class SizePlan(_Handle):
    """A decompressed-size plan (mscomp_amd_plan_create_size): for every unit the status and length a decompress plan with
    out_cap = limit would report, and the smallest capacity that decodes (``need``). ``limit`` None = no limit (2^64 - 1)."""

    def __init__(self, ctx, fmt, in_off, in_len, limit=None):
        _Handle.__init__(self, ctx)
        self.fmt = int(fmt)
        self.in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        self.in_len = np.ascontiguousarray(in_len, dtype=np.uint64)
        assert self.in_off.ndim == 1 and self.in_off.shape == self.in_len.shape
        self.limit = None if limit is None else np.ascontiguousarray(limit, dtype=np.uint64)
        assert self.limit is None or self.limit.shape == self.in_off.shape
        self.n_units = len(self.in_off)
        self._make("mscomp_amd_plan_create_size", self.fmt, self.n_units, self.in_off.ctypes.data, self.in_len.ctypes.data,
                   None if self.limit is None else self.limit.ctypes.data)

    def execute(self, d_in, d_out_len, d_need, d_status):
        """Enqueue on the ctx stream. Arguments are torch CUDA tensors (uint8, int64/uint64[n], int64/uint64[n], int32[n])."""
        self._run("mscomp_amd_plan_execute_size", d_in, d_out_len, d_need, d_status)


class DevPlan(_Handle):
    """A decompress plan with device tables (mscomp_amd_plan_create_decompress_dev): made once for n_units units whose in_len sum to at most
    in_total_max and whose out_cap sum to at most out_total_max, then executed with unit tables that live on the device.
    ``large_units`` (MSCOMP_AMD_DEV_LARGE_UNITS): the plan also builds the tables of a host plan's paths for large units on the device
    (segment walk, all-CU byte stage, candidate token scratch), at the price of their scratch and launches in every execution."""

    def __init__(self, ctx, fmt, n_units, in_total_max, out_total_max, large_units=False):
        _Handle.__init__(self, ctx)
        self.fmt, self.n_units = int(fmt), int(n_units)
        self.in_total_max, self.out_total_max = int(in_total_max), int(out_total_max)
        self.large_units = bool(large_units)
        if self.large_units:
            self._make("mscomp_amd_plan_create_decompress_dev_ex", self.fmt, self.n_units, self.in_total_max, self.out_total_max, MSCOMP_AMD_DEV_LARGE_UNITS)
        else:
            self._make("mscomp_amd_plan_create_decompress_dev", self.fmt, self.n_units, self.in_total_max, self.out_total_max)

    def execute(self, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_out_len, d_status):
        """Enqueue on the ctx stream (nothing is synchronized or read back). Arguments are torch CUDA tensors: uint8 input and output, int64 /
        uint64 tables of n_units entries (offsets, lengths, capacities; results d_out_len), int32 d_status."""
        self._run("mscomp_amd_plan_execute_dev", d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_out_len, d_status)


class CompressDevPlan(DevPlan):
    """A compress plan with device tables (mscomp_amd_plan_create_compress_dev): made once for n_units units of at most in_unit_max bytes each
    whose in_len sum to at most in_total_max, then executed (``execute``, as DevPlan's) with unit tables that live on the device."""

    def __init__(self, ctx, fmt, n_units, in_total_max, in_unit_max):
        _Handle.__init__(self, ctx)
        self.fmt, self.n_units = int(fmt), int(n_units)
        self.in_total_max, self.in_unit_max = int(in_total_max), int(in_unit_max)
        self._make("mscomp_amd_plan_create_compress_dev", self.fmt, self.n_units, self.in_total_max, self.in_unit_max)


class SizeDevPlan(DevPlan):
    """A size plan with device tables (mscomp_amd_plan_create_size_dev): made once for n_units units whose in_len sum to at most in_total_max,
    then executed with unit tables (offsets, lengths, optional limits) that live on the device. ``large_units``: as DevPlan's (Xpress
    streams of 512 KiB or more are sized by segments)."""

    def __init__(self, ctx, fmt, n_units, in_total_max, large_units=False):
        _Handle.__init__(self, ctx)
        self.fmt, self.n_units = int(fmt), int(n_units)
        self.in_total_max = int(in_total_max)
        self.large_units = bool(large_units)
        if self.large_units:
            self._make("mscomp_amd_plan_create_size_dev_ex", self.fmt, self.n_units, self.in_total_max, MSCOMP_AMD_DEV_LARGE_UNITS)
        else:
            self._make("mscomp_amd_plan_create_size_dev", self.fmt, self.n_units, self.in_total_max)

    def execute(self, d_in, d_in_off, d_in_len, d_out_len, d_need, d_status, d_limit=None):
        """Enqueue on the ctx stream (nothing is synchronized or read back). Arguments are torch CUDA tensors: uint8 input, int64 / uint64
        tables of n_units entries (offsets, lengths, d_limit or None = no limit; results d_out_len, d_need), int32 d_status."""
        self._run("mscomp_amd_plan_execute_size_dev", d_in, d_in_off, d_in_len, d_limit, d_out_len, d_need, d_status)


class CrcDevPlan(DevPlan):
    """A CRC-32 plan with device tables (mscomp_amd_plan_create_crc_dev): made once for n_units units whose lengths sum to at most
    in_total_max, then executed with unit tables that live on the device. The value is zlib's crc32."""

    def __init__(self, ctx, n_units, in_total_max):
        _Handle.__init__(self, ctx)
        self.n_units, self.in_total_max = int(n_units), int(in_total_max)
        self._make("mscomp_amd_plan_create_crc_dev", self.n_units, self.in_total_max)

    def execute(self, d_in, d_in_off, d_in_len, d_crc, d_status):
        """Enqueue on the ctx stream (nothing is synchronized or read back). Arguments are torch CUDA tensors: uint8 input, int64 / uint64
        offsets and lengths of n_units entries, int32 d_crc (the 32 bits of each CRC) and int32 d_status."""
        self._run("mscomp_amd_plan_execute_crc_dev", d_in, d_in_off, d_in_len, d_crc, d_status)


class BlockContainer(_Handle):
    """A block container (mscomp_amd_blocks_create): resources cut into blocks of ``block_size`` bytes (a power of two, 4096 .. 524288), every
    block compressed on its own or stored raw when it does not shrink, the stored blocks packed back to back behind an offset table. Made
    once for ``n_res`` resources whose lengths sum to at most ``in_total_max``; ``n_blocks_max`` = n_res + in_total_max // block_size bounds
    the blocks of a batch. All scratch is reserved here: two inner dev plans, 64 bytes of tables per possible block, and a staging area of
    1 byte per byte of in_total_max + 16 per resource. Both calls enqueue kernels on the ctx stream and nothing else (nothing is
    synchronized or read back; legal inside a capture of that stream). Arguments are torch CUDA tensors: uint8 data, int64 / uint64 tables,
    int32 statuses."""
    _destroy = "mscomp_amd_blocks_destroy"

    def __init__(self, ctx, fmt, block_size, n_res, in_total_max):
        _Handle.__init__(self, ctx)
        self.fmt, self.block_size = int(fmt), int(block_size)
        self.n_res, self.in_total_max = int(n_res), int(in_total_max)
        self._make("mscomp_amd_blocks_create", self.fmt, self.block_size, self.n_res, self.in_total_max, 0)
        self.n_blocks_max = int(ctx.lib.mscomp_amd_blocks_bound(self._h))

    def compress(self, d_in, d_res_off, d_res_len, d_packed, d_block_first, d_block_off, d_status, packed_cap=None):
        """Resource r = d_res_len[r] bytes at d_in + d_res_off[r] (n_res entries each). Writes d_block_first (n_res + 1: the running count
        of blocks), d_block_off (n_blocks_max + 1: the running sum of the stored lengths, the entries behind the last block repeating the
        total), the stored blocks to d_packed[0 .. total) and d_status (n_res). Nothing is written at or behind ``packed_cap`` (default:
        all of d_packed); a block that would end beyond it is left out and its resource gets MSCOMP_BUF_ERROR."""
        cap = d_packed.numel() if packed_cap is None else int(packed_cap)
        if cap > d_packed.numel():
            raise ValueError("packed_cap exceeds d_packed")
        self._run("mscomp_amd_blocks_compress", d_in, d_res_off, d_res_len, d_packed, cap, d_block_first, d_block_off, d_status)

    def decompress(self, d_packed, d_block_first, d_block_off, d_res_len, d_out, d_out_off, d_out_cap, d_out_len, d_status, d_range=None,
                   packed_len=None):
        """Decodes, per resource, the blocks of ``d_range`` (2 x n_res: first block, count; both clipped; None = every block) to
        d_out + d_out_off[r], at most d_out_cap[r] bytes. d_status[r] is MSCOMP_OK with d_out_len[r] = the bytes the range stands for,
        MSCOMP_ARG_ERROR (beyond the creation bounds), MSCOMP_DATA_ERROR (a damaged table or payload) or MSCOMP_BUF_ERROR (capacity), with
        d_out_len[r] = 0. ``packed_len``: the valid bytes of d_packed (default: all of it)."""
        plen = d_packed.numel() if packed_len is None else int(packed_len)
        self._run("mscomp_amd_blocks_decompress", d_packed, plen, d_block_first, d_block_off, d_res_len, d_range, d_out, d_out_off, d_out_cap, d_out_len,
                  d_status)

    def crc(self, d_data, d_res_off, d_res_len, d_block_crc, d_status, d_res_crc=None):
        """CRC-32 of the uncompressed blocks of the resources (as compress takes them): d_block_crc (int32, n_blocks_max; entry j belongs to the
        block compress puts at d_block_off[j], the entries behind the last block are 0), d_res_crc (optional, int32, n_res: the CRC-32 of
        every whole resource, from the same pass) and d_status (n_res: MSCOMP_OK, or MSCOMP_ARG_ERROR as compress gives it)."""
        self._run("mscomp_amd_blocks_crc", d_data, d_res_off, d_res_len, d_block_crc, d_res_crc, d_status)

    def check(self, d_out, d_out_off, d_res_len, d_block_first, d_block_crc, d_out_len, d_status, d_range=None):
        """After decompress, with its tables and results: every block of the (clipped) range of every resource that is MSCOMP_OK in d_status
        is read back from d_out and held to d_block_crc; a mismatch turns the resource into MSCOMP_DATA_ERROR with d_out_len = 0."""
        self._run("mscomp_amd_blocks_check", d_out, d_out_off, d_res_len, d_block_first, d_range, d_block_crc, d_out_len, d_status)

    def salvage(self, d_packed, d_block_first, d_block_off, d_res_len, d_out, d_out_off, d_out_cap, d_out_len, d_bad, d_verdict, d_count, d_status,
                d_block_crc=None, d_only=None, packed_len=None):
        """Decodes every block that can be decoded and says which could not: d_verdict (int32, n_blocks_max) holds MSCOMP_AMD_BLOCK_GOOD,
        _TABLE, _DECODE, _CRC (only with ``d_block_crc``) or _SKIPPED per row of the table. A resource that decompress's checks 1-3 refuse
        keeps that status with d_out_len = 0 and d_bad = 0 and is neither read nor written; every other resource has d_out_len[r] = its
        length whatever its rows say, its good rows' data in place, ZEROS in its judged bad rows, d_bad[r] (int32, n_res) = their number
        and d_status[r] MSCOMP_OK without one, MSCOMP_DATA_ERROR otherwise. ``d_only`` (int32, n_blocks_max; the d_verdict of a copy of the
        same shape): rows it marks GOOD are not judged, not read and not written. d_count (int64, 4) = rows judged, rows bad, bytes
        zero-filled, resources with a bad row."""
        plen = d_packed.numel() if packed_len is None else int(packed_len)
        self._run("mscomp_amd_blocks_salvage", d_packed, plen, d_block_first, d_block_off, d_res_len, d_block_crc, d_only, d_out, d_out_off, d_out_cap,
                  d_out_len, d_bad, d_verdict, d_count, d_status)


def blocks_compress(fmt, buffers, block_size, ctx=None):
    """The block container of a list of byte strings (one resource each), built on the GPU. Returns numpy arrays (packed uint8, block_first
    uint64 of n + 1, block_off uint64 of nb + 1, statuses int32): block j of resource r is
    packed[block_off[block_first[r] + j] : block_off[block_first[r] + j + 1]], the bytes of ms_compress for that block when they are
    shorter than the block, the block itself otherwise."""
    import torch
    n = len(buffers)
    with _call(ctx) as (ctx, dev):
        d_in, d_off, d_len, lens = _upload_unit_tables(buffers, dev)
        total = int(sum(lens))
        bk = BlockContainer(ctx, fmt, block_size, n, total)
        d_packed = torch.zeros(total + 16, dtype=torch.uint8, device=dev)
        d_first = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_boff = torch.zeros(bk.n_blocks_max + 1, dtype=torch.int64, device=dev)
        d_st = torch.zeros(max(1, n), dtype=torch.int32, device=dev)
        bk.compress(d_in, d_off, d_len, d_packed, d_first, d_boff, d_st, packed_cap=total)
        ctx.stream.synchronize()
        first = d_first.cpu().numpy().view(np.uint64).copy()
        nb = int(first[n])
        boff = d_boff.cpu().numpy().view(np.uint64)[: nb + 1].copy()
        packed = d_packed.cpu().numpy()[: int(boff[nb])].copy()
        st = d_st.cpu().numpy()[:n].copy()
        bk.close()
    return packed, first, boff, st


def crc32_units(units, ctx=None):
    """zlib's crc32 of every byte string of a list, computed on the GPU (CrcDevPlan). Returns a numpy uint32 array."""
    import torch
    n = len(units)
    with _call(ctx) as (ctx, dev):
        d_in, d_off, d_len, lens = _upload_unit_tables(units, dev)
        d_crc = torch.zeros(max(1, n), dtype=torch.int32, device=dev)
        d_st = torch.zeros(max(1, n), dtype=torch.int32, device=dev)
        plan = CrcDevPlan(ctx, n, int(sum(lens)))
        plan.execute(d_in, d_off, d_len, d_crc, d_st)
        ctx.stream.synchronize()
        out, st = d_crc.cpu().numpy().view(np.uint32)[:n].copy(), d_st.cpu().numpy()[:n]
        plan.close()
    if st.any():
        raise MSCompError(int(st[st != 0][0]), "mscomp_amd_plan_execute_crc_dev")
    return out


def blocks_crc(fmt, buffers, block_size, ctx=None):
    """The checksums a block container keeps beside a list of byte strings (one resource each), computed on the GPU. Returns numpy uint32
    arrays (block_crc of nb entries, in the block order of blocks_compress; res_crc of n): zlib's crc32 of every block and of every resource."""
    import torch
    n = len(buffers)
    with _call(ctx) as (ctx, dev):
        d_in, d_off, d_len, lens = _upload_unit_tables(buffers, dev)
        bk = BlockContainer(ctx, fmt, block_size, n, int(sum(lens)))
        d_bcrc = torch.zeros(max(1, bk.n_blocks_max), dtype=torch.int32, device=dev)
        d_rcrc = torch.zeros(max(1, n), dtype=torch.int32, device=dev)
        d_st = torch.zeros(max(1, n), dtype=torch.int32, device=dev)
        bk.crc(d_in, d_off, d_len, d_bcrc, d_st, d_res_crc=d_rcrc)
        ctx.stream.synchronize()
        nb = sum((x + block_size - 1) // block_size for x in lens)
        out = d_bcrc.cpu().numpy().view(np.uint32)[:nb].copy(), d_rcrc.cpu().numpy().view(np.uint32)[:n].copy()
        bk.close()
    return out


def blocks_decompress(fmt, packed, block_first, block_off, lengths, block_size, ranges=None, ctx=None, block_crc=None):
    """Decode resources of a block container on the GPU: ``lengths`` are the resources' original lengths, ``ranges`` (optional) one
    (first block, count) pair per resource, clipped to its blocks; default: whole resources. ``block_crc`` (optional, as blocks_crc returns
    it): the decoded blocks are held to these checksums, and a resource with a mismatch gets MSCOMP_DATA_ERROR. Returns (list of bytes, or
    None where the status is not MSCOMP_OK; list of status)."""
    import torch
    n = len(lengths)
    lens = [int(x) for x in lengths]
    total = int(sum(lens))
    out_off, out_total = pack_offsets(lens)
    with _call(ctx) as (ctx, dev):
        bk = BlockContainer(ctx, fmt, block_size, n, total)
        packed, d_packed = _dev_packed(packed, dev)
        d_first, d_boff = _dev_u64(block_first, n + 1, dev), _dev_u64(block_off, bk.n_blocks_max + 1, dev)
        d_len, d_ooff, d_ocap = _dev_u64(lens, 1, dev), _dev_u64(out_off, 1, dev), _dev_u64(lens, 1, dev)
        d_range = None if ranges is None else _dev_u64(np.asarray(ranges, dtype=np.uint64), 2, dev)
        d_out = torch.zeros(out_total + 16, dtype=torch.uint8, device=dev)
        d_olen = torch.zeros(max(1, n), dtype=torch.int64, device=dev)
        d_st = torch.zeros(max(1, n), dtype=torch.int32, device=dev)
        bk.decompress(d_packed, d_first, d_boff, d_len, d_out, d_ooff, d_ocap, d_olen, d_st, d_range=d_range, packed_len=len(packed))
        if block_crc is not None:
            bk.check(d_out, d_ooff, d_len, d_first, _dev_block_crc(block_crc, bk.n_blocks_max, dev), d_olen, d_st, d_range=d_range)
        ctx.stream.synchronize()
        h_out, h_len, h_st = d_out.cpu().numpy(), d_olen.cpu().numpy(), d_st.cpu().numpy()
        bk.close()
    res = [bytes(h_out[int(out_off[i]): int(out_off[i]) + int(h_len[i])]) if h_st[i] == MSCOMP_OK else None for i in range(n)]
    return res, [int(x) for x in h_st[:n]]


def blocks_salvage(fmt, packed, block_first, block_off, lengths, block_size, ctx=None, block_crc=None, only=None):
    """Salvage a block container on the GPU (BlockContainer.salvage): every block that can be decoded is, and the others are named.
    ``block_crc`` (optional, as blocks_crc returns it) holds the decoded blocks to their checksums; ``only`` (optional: the verdicts of a
    copy of the same shape) leaves out the rows it marks MSCOMP_AMD_BLOCK_GOOD. Returns (buffers: bytes of the resource's length with
    zeros in the bad rows and in the rows left out, or None for a resource refused as a whole; verdicts: a numpy uint32 array with one
    entry per row of block_off; bad: list; statuses: list; counts: list of 4)."""
    import torch
    n = len(lengths)
    lens = [int(x) for x in lengths]
    total = int(sum(lens))
    out_off, out_total = pack_offsets(lens)
    with _call(ctx) as (ctx, dev):
        bk = BlockContainer(ctx, fmt, block_size, n, total)
        nbm = bk.n_blocks_max
        packed, d_packed = _dev_packed(packed, dev)
        d_first, d_boff = _dev_u64(block_first, n + 1, dev), _dev_u64(block_off, nbm + 1, dev)
        d_len, d_ooff, d_ocap = _dev_u64(lens, 1, dev), _dev_u64(out_off, 1, dev), _dev_u64(lens, 1, dev)
        d_crc = None if block_crc is None else _dev_block_crc(block_crc, nbm, dev)
        d_only = None
        if only is not None:                                       # (rows behind the mask's own are judged)
            h_only = np.full(max(1, nbm), MSCOMP_AMD_BLOCK_SKIPPED, dtype=np.uint32)
            k = min(len(only), nbm)
            h_only[:k] = np.asarray(only, dtype=np.uint32)[:k]
            d_only = torch.from_numpy(h_only.view(np.int32).copy()).to(dev)
        d_out = torch.zeros(out_total + 16, dtype=torch.uint8, device=dev)
        d_olen, d_cnt = torch.zeros(max(1, n), dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
        d_bad, d_st = torch.zeros(max(1, n), dtype=torch.int32, device=dev), torch.zeros(max(1, n), dtype=torch.int32, device=dev)
        d_ver = torch.full((max(1, nbm),), MSCOMP_AMD_BLOCK_SKIPPED, dtype=torch.int32, device=dev)
        bk.salvage(d_packed, d_first, d_boff, d_len, d_out, d_ooff, d_ocap, d_olen, d_bad, d_ver, d_cnt, d_st, d_block_crc=d_crc, d_only=d_only,
                   packed_len=len(packed))
        ctx.stream.synchronize()
        h_out, h_len, h_st, h_bad = d_out.cpu().numpy(), d_olen.cpu().numpy(), d_st.cpu().numpy(), d_bad.cpu().numpy()
        rows = max(0, len(np.asarray(block_off).reshape(-1)) - 1)
        ver = np.full(rows, MSCOMP_AMD_BLOCK_SKIPPED, dtype=np.uint32)
        ver[: min(rows, nbm)] = d_ver.cpu().numpy().view(np.uint32)[: min(rows, nbm)]
        counts = [int(x) for x in d_cnt.cpu().numpy()]
        bk.close()
    accepted = lambda i: h_st[i] == MSCOMP_OK or (h_st[i] == MSCOMP_DATA_ERROR and h_bad[i] > 0)
    res = [bytes(h_out[int(out_off[i]): int(out_off[i]) + int(h_len[i])]) if accepted(i) else None for i in range(n)]
    return res, ver, [int(x) for x in h_bad[:n]], [int(x) for x in h_st[:n]], counts


class _BlockAccess(_Handle):
    """What BlockReader and BlockWriter share: the arguments they are made with; ``_counts`` names the export their counts() read."""

    def __init__(self, ctx, fmt, block_size, n_res, n_blocks_table, n_req, blocks_max):
        _Handle.__init__(self, ctx)
        self.fmt, self.block_size = int(fmt), int(block_size)
        self.n_res, self.n_blocks_table, self.n_req, self.blocks_max = int(n_res), int(n_blocks_table), int(n_req), int(blocks_max)
        self._make(self._create, self.fmt, self.block_size, self.n_res, self.n_blocks_table, self.n_req, self.blocks_max, 0)


class BlockReader(_BlockAccess):
    """A block reader (mscomp_amd_reader_create): batched byte-range reads from a block container, by its tables alone. Made once for
    ``n_req`` requests per call that together cover at most ``blocks_max`` blocks (counted per request, before any sharing); the tables are
    those of a container of ``n_res`` resources whose d_block_off has ``n_blocks_table`` + 1 entries. All scratch is reserved here: a cache
    of blocks_max blocks, one inner dev plan, 88 bytes of tables per unit of blocks_max, 44 per request and 4 per block-table entry. read()
    enqueues kernels on the ctx stream and nothing else (legal inside a capture of that stream). Arguments are torch CUDA tensors: uint8
    data, int64 / uint64 tables, int32 statuses and checksums."""
    _create, _destroy, _counts = "mscomp_amd_reader_create", "mscomp_amd_reader_destroy", "mscomp_amd_reader_counts"

    def read(self, d_packed, d_block_first, d_block_off, d_res_len, d_req, d_out, d_out_off, d_out_cap, d_out_len, d_status, d_block_crc=None,
             packed_len=None):
        """Request q = (resource, offset, length) = d_req[3 q .. 3 q + 2], clipped to the resource as pread does. d_status[q] is MSCOMP_OK
        with d_out_len[q] = the clipped length and exactly those bytes at d_out + d_out_off[q]; or MSCOMP_ARG_ERROR (no such resource, or
        over the budget of blocks_max), MSCOMP_BUF_ERROR (more than d_out_cap[q]) or MSCOMP_DATA_ERROR (a damaged table or block; with
        ``d_block_crc``, as BlockContainer.crc wrote it, a block whose CRC-32 differs) with d_out_len[q] = 0 and nothing written.
        ``packed_len``: the valid bytes of d_packed (default: all of it)."""
        plen, _ = _byte_bounds(d_packed, packed_len)
        self._run("mscomp_amd_reader_read", d_packed, plen, d_block_first, d_block_off, d_res_len, d_block_crc, d_req, d_out, d_out_off, d_out_cap,
                  d_out_len, d_status)

    def counts(self):
        """(units, distinct blocks, blocks decoded rather than raw) of the last read(); synchronizes the stream."""
        return _three_counts(self, self._counts)


def blocks_read(fmt, packed, block_first, block_off, lengths, block_size, requests, ctx=None, block_crc=None):
    """Read byte ranges of a block container on the GPU: ``requests`` is a list of (resource, offset, length), each clipped to its resource
    as pread does; ``lengths`` are the resources' original lengths. ``block_crc`` (optional, as blocks_crc returns it): every block read is
    held to its checksum. Returns (list of bytes, or None where the status is not MSCOMP_OK; list of status)."""
    import torch
    n, nq = len(lengths), len(requests)
    lens = [int(x) for x in lengths]
    B = int(block_size)
    M64 = (1 << 64) - 1
    reqs = [(int(r) & M64, int(o) & M64, int(ln) & M64) for r, o, ln in requests]
    wants, blocks = _covering_blocks(reqs, lens, B)            # (the capacities, and the budget)
    out_off, out_total = pack_offsets(wants)
    nbt = max(0, len(np.asarray(block_off).reshape(-1)) - 1)
    with _call(ctx) as (ctx, dev):
        rd = BlockReader(ctx, fmt, B, n, nbt, nq, blocks)
        packed, d_packed = _dev_packed(packed, dev)
        d_first, d_boff, d_len = _dev_u64(block_first, n + 1, dev), _dev_u64(block_off, nbt + 1, dev), _dev_u64(lens, 1, dev)
        d_req = _dev_u64(np.array(reqs, dtype=np.uint64), 3, dev)
        d_ooff, d_ocap = _dev_u64(out_off, 1, dev), _dev_u64(wants, 1, dev)
        d_crc = None if block_crc is None else _dev_block_crc(block_crc, nbt, dev)
        d_out = torch.zeros(out_total + 16, dtype=torch.uint8, device=dev)
        d_olen = torch.zeros(max(1, nq), dtype=torch.int64, device=dev)
        d_st = torch.zeros(max(1, nq), dtype=torch.int32, device=dev)
        rd.read(d_packed, d_first, d_boff, d_len, d_req, d_out, d_ooff, d_ocap, d_olen, d_st, d_block_crc=d_crc, packed_len=len(packed))
        ctx.stream.synchronize()
        h_out, h_len, h_st = d_out.cpu().numpy(), d_olen.cpu().numpy(), d_st.cpu().numpy()
        rd.close()
    res = [bytes(h_out[int(out_off[i]): int(out_off[i]) + int(h_len[i])]) if h_st[i] == MSCOMP_OK else None for i in range(nq)]
    return res, [int(x) for x in h_st[:nq]]


class BlockWriter(_BlockAccess):
    """A block writer (mscomp_amd_writer_create): batched byte-range writes into a block container, out of place. Made once for ``n_req``
    requests per call that together cover at most ``blocks_max`` blocks (counted per request, before any sharing), against the tables of
    a container of ``n_res`` resources whose d_block_off has ``n_blocks_table`` + 1 entries. All scratch is reserved here: a cache and a
    staging area of blocks_max blocks each, two inner dev plans, 96 bytes of tables per unit of blocks_max, 44 per request, 8 per
    block-table entry and 12 per resource. write() and resize() enqueue kernels on the ctx stream and nothing else (legal inside a capture
    of that stream); for resize() blocks_max bounds the blocks whose data changes: per resource the block the new end falls into, and the
    blocks that did not exist. Arguments are torch CUDA tensors: uint8 data, int64 / uint64 tables, int32 statuses and checksums."""
    _create, _destroy, _counts = "mscomp_amd_writer_create", "mscomp_amd_writer_destroy", "mscomp_amd_writer_counts"

    def write(self, d_packed, d_block_first, d_block_off, d_res_len, d_req, d_src, d_src_off, d_new_packed, d_new_block_off, d_written, d_status,
              d_res_status, d_block_crc=None, d_new_block_crc=None, packed_len=None, new_cap=None):
        """Request q = (resource, offset, length) = d_req[3 q .. 3 q + 2], clipped to the resource as the reader clips it; its bytes are read
        at d_src + d_src_off[q]. The old container (d_packed, d_block_off, d_block_crc) is only read; the new one is written to
        d_new_packed (nothing at or behind ``new_cap``, default: all of it), d_new_block_off and d_new_block_crc (given exactly when
        d_block_crc is). d_status[q] is MSCOMP_OK with d_written[q] = the clipped length, or MSCOMP_ARG_ERROR (no such resource, or over
        the budget of blocks_max) or MSCOMP_DATA_ERROR (a damaged table or block) with d_written[q] = 0 and no byte of the request
        applied. d_res_status[r] is MSCOMP_BUF_ERROR when a block of the resource did not fit below new_cap. A touched block is decoded,
        patched in request order and encoded again; every other block keeps its stored bytes."""
        plen, cap = _byte_bounds(d_packed, packed_len, d_new_packed, new_cap)
        self._run("mscomp_amd_writer_write", d_packed, plen, d_block_first, d_block_off, d_res_len, d_block_crc, d_req, d_src, d_src_off, d_new_packed, cap,
                  d_new_block_off, d_new_block_crc, d_written, d_status, d_res_status)

    def resize(self, d_packed, d_block_first, d_block_off, d_res_len, d_want_len, d_new_packed, d_new_block_first, d_new_block_off, d_new_res_len,
               d_res_status, d_block_crc=None, d_new_block_crc=None, packed_len=None, new_cap=None):
        """Every resource r cut or zero-extended to d_want_len[r] bytes (mscomp_amd_writer_resize), out of place as write(): the new
        container goes to d_new_packed (nothing at or behind ``new_cap``, default: all of it), d_new_block_first (n_res + 1),
        d_new_block_off (n_blocks_table + 1), d_new_block_crc (given exactly when d_block_crc is) and d_new_res_len (n_res).
        d_res_status[r] is MSCOMP_OK, or MSCOMP_DATA_ERROR (a wrong block count, or an unreadable block where the length changes inside
        it) or MSCOMP_ARG_ERROR (over the budget of blocks_max changed and fresh blocks) with the resource carried as it was, or
        MSCOMP_BUF_ERROR (a block did not fit below new_cap); all MSCOMP_ARG_ERROR with zeroed tables when the new table needs more than
        n_blocks_table rows. Only the block the new end falls into is decoded; it and the fresh blocks are encoded."""
        plen, cap = _byte_bounds(d_packed, packed_len, d_new_packed, new_cap)
        self._run("mscomp_amd_writer_resize", d_packed, plen, d_block_first, d_block_off, d_res_len, d_block_crc, d_want_len, d_new_packed, cap,
                  d_new_block_first, d_new_block_off, d_new_block_crc, d_new_res_len, d_res_status)

    def counts(self):
        """(units, distinct blocks touched, blocks encoded again) of the last write(), or (units, changed blocks decoded, blocks encoded) of
        the last resize(); synchronizes the stream."""
        return _three_counts(self, self._counts)


def blocks_write(fmt, packed, block_first, block_off, lengths, block_size, writes, ctx=None, block_crc=None):
    """Write byte ranges into a block container on the GPU: ``writes`` is a list of (resource, offset, bytes), each clipped to its resource
    (a write never changes a resource's length); ``lengths`` are the resources' original lengths; ``block_crc`` (optional, as blocks_crc
    returns it): every block touched is held to its checksum first, and the new container gets checksums too. Returns numpy arrays and
    lists (new_packed uint8, new_block_off uint64, new_block_crc uint32 or None, written, statuses, res_statuses): the new container
    shares block_first and lengths with the old one."""
    import torch
    n, nq = len(lengths), len(writes)
    lens = [int(x) for x in lengths]
    B = int(block_size)
    M64 = (1 << 64) - 1
    reqs = [(int(r) & M64, int(o) & M64, len(b)) for r, o, b in writes]
    _, blocks = _covering_blocks(reqs, lens, B)                # (the budget)
    src_off, src_total = pack_offsets([len(b) for _, _, b in writes])
    nbt = max(0, len(np.asarray(block_off).reshape(-1)) - 1)
    total = int(sum(lens))
    with _call(ctx) as (ctx, dev):
        wr = BlockWriter(ctx, fmt, B, n, nbt, nq, blocks)
        packed, d_packed = _dev_packed(packed, dev)
        h_src = np.zeros(src_total + 16, dtype=np.uint8)
        for (_, _, b), o in zip(writes, src_off):
            h_src[int(o): int(o) + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
        d_src = torch.from_numpy(h_src).to(dev)
        d_first, d_boff, d_len = _dev_u64(block_first, n + 1, dev), _dev_u64(block_off, nbt + 1, dev), _dev_u64(lens, 1, dev)
        d_req, d_soff = _dev_u64(np.array(reqs, dtype=np.uint64), 3, dev), _dev_u64(src_off, 1, dev)
        d_crc = None if block_crc is None else _dev_block_crc(block_crc, nbt, dev)
        d_new, _, d_noff, d_ncrc = _new_container(dev, None, nbt, total, block_crc is not None)
        d_wr = torch.zeros(max(1, nq), dtype=torch.int64, device=dev)
        d_st = torch.zeros(max(1, nq), dtype=torch.int32, device=dev)
        d_rst = torch.zeros(max(1, n), dtype=torch.int32, device=dev)
        wr.write(d_packed, d_first, d_boff, d_len, d_req, d_src, d_soff, d_new, d_noff, d_wr, d_st, d_rst, d_block_crc=d_crc, d_new_block_crc=d_ncrc,
                 packed_len=len(packed), new_cap=total)
        ctx.stream.synchronize()
        new_packed, _, noff, ncrc = _fetch_container(d_new, None, d_noff, d_ncrc, total)
        h_wr, h_st, h_rst = d_wr.cpu().numpy().view(np.uint64), d_st.cpu().numpy(), d_rst.cpu().numpy()
        wr.close()
    return new_packed, noff, ncrc, [int(x) for x in h_wr[:nq]], [int(x) for x in h_st[:nq]], [int(x) for x in h_rst[:n]]


def blocks_resize(fmt, packed, block_first, block_off, lengths, block_size, new_lengths, ctx=None, block_crc=None):
    """Cut or zero-extend the resources of a block container to ``new_lengths`` on the GPU (BlockWriter.resize); ``lengths`` are their
    lengths now, ``block_crc`` as blocks_crc returns it (optional: the block a cut falls into is held to its checksum first, and the new
    container gets checksums too). Returns numpy arrays and lists (new_packed uint8, new_block_off uint64, new_block_crc uint32 or None,
    new_first uint64 of n + 1, new_lengths, res_statuses); the tables have as many rows as the resized container needs."""
    import torch
    n = len(lengths)
    lens, want = [int(x) for x in lengths], [int(x) for x in new_lengths]
    if len(want) != n:
        raise ValueError("one new length per resource")
    B = int(block_size)
    blocks = lambda x: (x + B - 1) // B
    # (the block the shorter of the two lengths ends in changes its data length unless that end is a block boundary)
    budget = sum((1 if min(a, b) % B else 0) + max(0, blocks(b) - blocks(a)) for a, b in zip(lens, want) if a != b)
    nb_old = max(0, len(np.asarray(block_off).reshape(-1)) - 1)
    nbt = max(nb_old, sum(blocks(max(a, b)) for a, b in zip(lens, want)))
    room = sum(max(a, b) for a, b in zip(lens, want))
    with _call(ctx) as (ctx, dev):
        wr = BlockWriter(ctx, fmt, B, n, nbt, 0, budget)
        packed, d_packed = _dev_packed(packed, dev)
        d_first, d_boff, d_len, d_want = _dev_u64(block_first, n + 1, dev), _dev_u64(block_off, nbt + 1, dev), _dev_u64(lens, 1, dev), _dev_u64(want, 1, dev)
        d_crc = None if block_crc is None else _dev_block_crc(block_crc, nbt, dev)
        d_new, d_nfirst, d_noff, d_ncrc = _new_container(dev, n, nbt, room, block_crc is not None)
        d_nlen = torch.zeros(max(1, n), dtype=torch.int64, device=dev)
        d_rst = torch.zeros(max(1, n), dtype=torch.int32, device=dev)
        wr.resize(d_packed, d_first, d_boff, d_len, d_want, d_new, d_nfirst, d_noff, d_nlen, d_rst, d_block_crc=d_crc, d_new_block_crc=d_ncrc,
                  packed_len=len(packed), new_cap=room)
        ctx.stream.synchronize()
        new_packed, nfirst, noff, ncrc = _fetch_container(d_new, d_nfirst, d_noff, d_ncrc, room)
        h_len, h_rst = d_nlen.cpu().numpy().view(np.uint64), d_rst.cpu().numpy()
        wr.close()
    return new_packed, noff, ncrc, nfirst, [int(x) for x in h_len[:n]], [int(x) for x in h_rst[:n]]


def _blocks_views(sources):
    """a BlocksView array from the ``sources`` of BlockSplicer.splice / BlockDeduper.dedup"""
    views = (BlocksView * len(sources))()
    names = ("d_packed", "d_block_first", "d_block_off", "d_res_len", "d_block_crc", "packed_len", "n_res", "n_blocks_table")
    ptr = lambda t: None if t is None else t.data_ptr()
    for v, s in zip(views, sources):
        f = dict(zip(names, s)) if isinstance(s, (tuple, list)) else {k: getattr(s, k, None) for k in names}
        v.d_packed, v.d_block_first, v.d_block_off = ptr(f["d_packed"]), ptr(f["d_block_first"]), ptr(f["d_block_off"])
        v.d_res_len, v.d_block_crc = ptr(f["d_res_len"]), ptr(f.get("d_block_crc"))
        plen = f.get("packed_len")
        v.packed_len = (0 if f["d_packed"] is None else f["d_packed"].numel()) if plen is None else int(plen)
        nr, nt = f.get("n_res"), f.get("n_blocks_table")
        v.n_res = (0 if f["d_res_len"] is None else f["d_res_len"].numel()) if nr is None else int(nr)
        v.n_blocks_table = (0 if f["d_block_off"] is None else max(0, f["d_block_off"].numel() - 1)) if nt is None else int(nt)
    return views


class BlockSplicer(_Handle):
    """A block splicer (mscomp_amd_splicer_create): a new container made of ``n_pick`` picks (source, resource) out of ``n_src`` (1 .. 4)
    source containers of one format and one ``block_size``, without decoding a byte; ``n_blocks_table`` is the number of rows of the NEW
    container's table. All scratch is reserved here: 8 bytes per row of that table + 64. splice() enqueues two kernels on the ctx stream
    and nothing else (legal inside a capture of that stream). Arguments are torch CUDA tensors: uint8 data, int64 / uint64 tables, int32
    statuses and checksums."""
    _destroy = "mscomp_amd_splicer_destroy"

    def __init__(self, ctx, block_size, n_src, n_pick, n_blocks_table):
        _Handle.__init__(self, ctx)
        self.block_size, self.n_src, self.n_pick, self.n_blocks_table = int(block_size), int(n_src), int(n_pick), int(n_blocks_table)
        self._make("mscomp_amd_splicer_create", self.block_size, self.n_src, self.n_pick, self.n_blocks_table, 0)

    def splice(self, sources, d_pick, d_new_packed, d_new_block_first, d_new_block_off, d_new_res_len, d_status, d_new_block_crc=None, new_cap=None):
        """``sources``: n_src tuples (d_packed, d_block_first, d_block_off, d_res_len, d_block_crc or None, packed_len or None = all of
        d_packed) or objects with these attributes; a source has d_res_len.numel() resources and d_block_off.numel() - 1 table rows unless
        it says otherwise (``n_res``, ``n_blocks_table``). Pick p = (d_pick[2 p], d_pick[2 p + 1]) = (source, resource) becomes resource p
        of the new container: d_new_block_first (n_pick + 1), d_new_block_off (n_blocks_table + 1), d_new_block_crc (optional; every source
        needs checksums then), d_new_res_len and d_status (n_pick), the stored blocks to d_new_packed (nothing at or behind ``new_cap``,
        default: all of it). d_status[p] is MSCOMP_OK, MSCOMP_ARG_ERROR (no such source or resource, a broken table entry, or no room in
        the new table) or MSCOMP_DATA_ERROR (a wrong block count) with pick p an empty resource, or MSCOMP_BUF_ERROR (a block did not fit
        below new_cap)."""
        _, cap = _byte_bounds(d_new_packed=d_new_packed, new_cap=new_cap)
        if len(sources) != self.n_src:
            raise ValueError("one source per n_src")
        self._run("mscomp_amd_splicer_splice", _blocks_views(sources), d_pick, d_new_packed, cap, d_new_block_first, d_new_block_off, d_new_block_crc,
                  d_new_res_len, d_status)


    @classmethod
    def for_extents(cls, ctx, block_size, n_src, n_res, n_ext, n_blocks_table):
        """A splicer for splice_extents() (mscomp_amd_splicer_create_extents): ``n_res`` new resources made of at most ``n_ext`` extents in
        all. Its scratch adds 8 bytes per extent and 8 per SPLICE_ROW_TILE rows of the new table; it serves splice() too, with
        n_pick = n_res."""
        self = cls.__new__(cls)
        _Handle.__init__(self, ctx)
        self.block_size, self.n_src, self.n_pick, self.n_blocks_table = int(block_size), int(n_src), int(n_res), int(n_blocks_table)
        self.n_res, self.n_ext = int(n_res), int(n_ext)
        self._make("mscomp_amd_splicer_create_extents", self.block_size, self.n_src, self.n_res, self.n_ext, self.n_blocks_table, 0)
        return self

    def splice_extents(self, sources, d_ext_first, d_ext, d_new_packed, d_new_block_first, d_new_block_off, d_new_res_len, d_status, d_new_block_crc=None,
                       new_cap=None):
        """``sources`` as for splice(). New resource q is the concatenation of the extents d_ext_first[q] .. d_ext_first[q + 1] - 1; extent e =
        d_ext[4 e .. 4 e + 3] = (source, resource, first block, block count; a count of 2**64 - 1 = through the last block). The outputs
        are splice()'s, per new resource. d_status[q] is MSCOMP_OK, MSCOMP_ARG_ERROR (no such source, resource or block range, a broken
        table entry, an extent that ends short in front of another, or no room in the new table) or MSCOMP_DATA_ERROR (a wrong block
        count) with resource q empty, or MSCOMP_BUF_ERROR (a block did not fit below new_cap)."""
        _, cap = _byte_bounds(d_new_packed=d_new_packed, new_cap=new_cap)
        if len(sources) != self.n_src:
            raise ValueError("one source per n_src")
        self._run("mscomp_amd_splicer_splice_extents", _blocks_views(sources), d_ext_first, d_ext, d_new_packed, cap, d_new_block_first, d_new_block_off,
                  d_new_block_crc, d_new_res_len, d_status)


def _splice_host(containers, n_new, nbt, room, ctx, make, run):
    """what blocks_splice and blocks_splice_extents share: the sources uploaded, the new arrays made, ``run`` called, the results fetched"""
    import torch
    with_crc = all(c[4] is not None for c in containers)
    with _call(ctx) as (ctx, dev):
        sp = make(ctx)
        srcs, _, _ = _upload_containers(containers, dev, with_crc)
        d_new, d_nfirst, d_noff, d_ncrc = _new_container(dev, n_new, nbt, room, with_crc)
        d_nlen = torch.zeros(max(1, n_new), dtype=torch.int64, device=dev)
        d_st = torch.zeros(max(1, n_new), dtype=torch.int32, device=dev)
        run(sp, srcs, dev, d_new, d_nfirst, d_noff, d_nlen, d_st, d_ncrc)
        ctx.stream.synchronize()
        new_packed, nfirst, noff, ncrc = _fetch_container(d_new, d_nfirst, d_noff, d_ncrc, room)
        h_len, h_st = d_nlen.cpu().numpy().view(np.uint64), d_st.cpu().numpy()
        sp.close()
    return new_packed, nfirst, noff, [int(x) for x in h_len[:n_new]], ncrc, [int(x) for x in h_st[:n_new]]


def blocks_splice_extents(containers, resources, block_size, ctx=None):
    """A new block container whose resources are made of block extents of up to four others on the GPU (BlockSplicer.splice_extents), no
    block decoded: ``containers`` as for blocks_splice, ``resources`` a list -- one entry per new resource -- of lists of (container,
    resource, first block, block count), a count of None meaning "through the last block". Every extent but the last non-empty one of a
    new resource must end on a block boundary. Returns what blocks_splice returns."""
    B = int(block_size)
    M64 = (1 << 64) - 1
    lens = [[int(x) for x in c[3]] for c in containers]
    ext, ext_first, nbt, room = [], [0], 0, 0
    for exts in resources:
        for s, r, k0, c in exts:
            ext.append((int(s) & M64, int(r) & M64, int(k0) & M64, M64 if c is None else int(c) & M64))
            if 0 <= s < len(lens) and 0 <= r < len(lens[s]):       # what the extent can bring at most: sizes the new arrays
                n = (lens[s][r] + B - 1) // B
                k = min(max(int(k0), 0), n)
                cnt = n - k if c is None else min(max(int(c), 0), n - k)
                nbt += cnt
                room += min(cnt * B, lens[s][r] - k * B) if cnt else 0
        ext_first.append(len(ext))
    n_res = len(resources)

    def run(sp, srcs, dev, d_new, d_nfirst, d_noff, d_nlen, d_st, d_ncrc):
        d_ext = _dev_u64(np.array(ext, dtype=np.uint64).reshape(-1), 4, dev)
        sp.splice_extents(srcs, _dev_u64(ext_first, 1, dev), d_ext, d_new, d_nfirst, d_noff, d_nlen, d_st, d_new_block_crc=d_ncrc, new_cap=room)
    return _splice_host(containers, n_res, nbt, room, ctx, lambda c: BlockSplicer.for_extents(c, B, len(containers), n_res, len(ext), nbt), run)


def blocks_concat(containers, parts, block_size, ctx=None):
    """One resource that joins the whole resources ``parts`` = [(container, resource), ...] in that order (every part but the last non-empty
    one must be a whole number of blocks long). Returns what blocks_splice returns, for a container of one resource."""
    return blocks_splice_extents(containers, [[(s, r, 0, None) for s, r in parts]], block_size, ctx=ctx)


def blocks_split_at(container, resource, k, block_size, ctx=None):
    """Resource ``resource`` of ``container`` split in front of its block ``k``: a container of two resources, the blocks [0, k) and the
    blocks from k on. Returns what blocks_splice returns."""
    return blocks_splice_extents([container], [[(0, resource, 0, k)], [(0, resource, k, None)]], block_size, ctx=ctx)


def blocks_cut_range(container, resource, k0, count, block_size, ctx=None):
    """Resource ``resource`` of ``container`` without its blocks [k0, k0 + count) (FALLOC_FL_COLLAPSE_RANGE): a container of one resource.
    Returns what blocks_splice returns."""
    return blocks_splice_extents([container], [[(0, resource, 0, k0), (0, resource, k0 + count, None)]], block_size, ctx=ctx)


def blocks_splice(containers, picks, block_size, ctx=None):
    """A new block container from resources of up to four others on the GPU (BlockSplicer), no block decoded: ``containers`` is a list of
    (packed, block_first, block_off, lengths, block_crc or None) of one format and ``block_size``, ``picks`` a list of (container,
    resource): pick p becomes resource p. The new container gets checksums when every source has them. Returns numpy arrays and lists
    (new_packed uint8, new_first uint64 of n + 1, new_block_off uint64 of nb + 1, new_lengths, new_block_crc uint32 or None, statuses)."""
    B = int(block_size)
    M64 = (1 << 64) - 1
    npk = len(picks)
    lens = [[int(x) for x in c[3]] for c in containers]
    got = [lens[s][r] if 0 <= s < len(lens) and 0 <= r < len(lens[s]) else 0 for s, r in picks]
    nbt = sum((L + B - 1) // B for L in got)
    room = sum(got)

    def run(sp, srcs, dev, d_new, d_nfirst, d_noff, d_nlen, d_st, d_ncrc):
        d_pick = _dev_u64(np.array([(int(s) & M64, int(r) & M64) for s, r in picks], dtype=np.uint64), 2, dev)
        sp.splice(srcs, d_pick, d_new, d_nfirst, d_noff, d_nlen, d_st, d_new_block_crc=d_ncrc, new_cap=room)
    return _splice_host(containers, npk, nbt, room, ctx, lambda c: BlockSplicer(c, B, len(containers), npk, nbt), run)


class BlockDeduper(_Handle):
    """A block deduper (mscomp_amd_deduper_create): which resources of ``n_src`` (1 .. 4) source containers of one format and one
    ``block_size`` hold the same bytes, decided on the stored blocks without decoding one, for up to ``n_res_total`` resources and
    ``n_blocks_total`` table rows in all sources together. All scratch is reserved here: 56 bytes per resource + 840. dedup() enqueues
    eight kernels on the ctx stream and nothing else (legal inside a capture of that stream). Arguments are torch CUDA tensors: int64 /
    uint64 tables, int32 statuses."""
    _destroy = "mscomp_amd_deduper_destroy"

    def __init__(self, ctx, block_size, n_src, n_res_total, n_blocks_total):
        _Handle.__init__(self, ctx)
        self.block_size, self.n_src, self.n_res_total, self.n_blocks_total = int(block_size), int(n_src), int(n_res_total), int(n_blocks_total)
        self._make("mscomp_amd_deduper_create", self.block_size, self.n_src, self.n_res_total, self.n_blocks_total, 0)

    def dedup(self, sources, d_rep, d_new_index, d_pick, d_count, d_status):
        """``sources``: as BlockSplicer.splice takes them; their resources are numbered back to back, g = 0 .. N - 1. d_rep[g] = the smallest
        resource equal to g (g itself for a unique or a refused one), d_new_index[g] = the rank of d_rep[g] among the unique ones, d_pick
        (2 n_res_total) = the unique resources as (source, resource) pairs, padded with 2^64 - 1 -- the pick list of a BlockSplicer made
        for n_res_total picks --, d_count (4) = unique resources, N, stored bytes of the others, refuted candidates; d_status[g] is
        MSCOMP_OK, MSCOMP_ARG_ERROR (a broken block_first entry) or MSCOMP_DATA_ERROR (a wrong block count, a broken block_off entry).
        Checksums take part in the comparison when every source has them."""
        if len(sources) != self.n_src:
            raise ValueError("one source per n_src")
        self._run("mscomp_amd_deduper_dedup", _blocks_views(sources), d_rep, d_new_index, d_pick, d_count, d_status)


    @classmethod
    def for_diff(cls, ctx, block_size, n_pair, n_blocks_new):
        """A deduper for diff() (mscomp_amd_deduper_create_diff): ``n_pair`` pairs (base resource, new resource) whose new resources have
        at most ``n_blocks_new`` blocks in all. Its scratch: 32 bytes per pair, 4 per new block and 64 per SPLICE_ROW_TILE of them, + 72.
        It refuses dedup(), as a deduper made for dedup() refuses diff()."""
        self = cls.__new__(cls)
        _Handle.__init__(self, ctx)
        self.block_size, self.n_pair, self.n_blocks_new = int(block_size), int(n_pair), int(n_blocks_new)
        self.n_src, self.n_res_total, self.n_blocks_total = 2, self.n_pair, self.n_blocks_new
        self._make("mscomp_amd_deduper_create_diff", self.block_size, self.n_pair, self.n_blocks_new, 0)
        return self

    def diff(self, base, new, d_pair, d_delta_ext_first, d_delta_ext, d_patch_ext_first, d_patch_ext, d_changed, d_count, d_status):
        """``base`` and ``new``: two sources as BlockSplicer.splice takes one. Pair p = (d_pair[2 p], d_pair[2 p + 1]) = (base resource or
        MSCOMP_AMD_DIFF_NO_BASE, new resource). Block k of the new resource is unchanged when the base resource has a block k of the same
        data length, stored length, CRC word (when both sources have checksums) and stored bytes. The answer is two extent lists in the
        form BlockSplicer.splice_extents takes, one new resource per pair: d_delta_ext_first (n_pair + 1) / d_delta_ext (4 n_blocks_new),
        over the one source [new], cut out the changed blocks; d_patch_ext_first / d_patch_ext, over the sources [base, that delta
        container], put the new resources together again. d_changed (n_pair) = the changed blocks of a pair, d_count (4) = changed blocks,
        blocks looked at, stored bytes of the changed blocks, blocks only the byte compare told apart; d_status[p] is MSCOMP_OK,
        MSCOMP_ARG_ERROR (no such resource, a broken block_first entry, or no room within n_blocks_new) or MSCOMP_DATA_ERROR (a wrong
        block count, a broken block_off entry), a refused pair having no extents."""
        views = _blocks_views([base, new])
        self._run("mscomp_amd_deduper_diff", C.byref(views[0]), C.byref(views[1]), d_pair, d_delta_ext_first, d_delta_ext, d_patch_ext_first, d_patch_ext,
                  d_changed, d_count, d_status)


    @classmethod
    def for_match(cls, ctx, block_size, n_src, n_res_total, n_blocks_total, n_blocks_new):
        """A deduper for match() (mscomp_amd_deduper_create_match): ``n_src`` (0 .. 3) stores and one new container with at most
        ``n_res_total`` resources and ``n_blocks_total`` table rows in all of them together, the new container bringing at most
        ``n_blocks_new`` rows. Its scratch: 48 bytes per resource, 40 per row, 4 per new row and 64 per SPLICE_ROW_TILE of them, + 848.
        It refuses dedup() and diff(), as dedupers made for those refuse match()."""
        self = cls.__new__(cls)
        _Handle.__init__(self, ctx)
        self.block_size, self.n_src, self.n_res_total = int(block_size), int(n_src), int(n_res_total)
        self.n_blocks_total, self.n_blocks_new = int(n_blocks_total), int(n_blocks_new)
        self._make("mscomp_amd_deduper_create_match", self.block_size, self.n_src, self.n_res_total, self.n_blocks_total, self.n_blocks_new, 0)
        return self

    def match(self, stores, new, d_delta_ext_first, d_delta_ext, d_patch_ext_first, d_patch_ext, d_class, d_count, d_status):
        """``stores``: n_src sources as BlockSplicer.splice takes them, ``new``: one more. A block of a resource of ``new`` is found when an
        equal block -- same data length, stored length, CRC word (when every source has checksums) and stored bytes -- lies anywhere in a
        store, shared when one lies earlier in ``new``, fresh otherwise. The answer is two extent lists in the form
        BlockSplicer.splice_extents takes, one new resource per resource of ``new``: d_delta_ext_first (n_res + 1) / d_delta_ext
        (4 n_blocks_new), over the one source [new], cut out the fresh blocks; d_patch_ext_first / d_patch_ext, over the sources
        stores + [that delta container], put the resources of ``new`` together again. d_class (3 n_res) = found, shared and fresh blocks
        per resource, d_count (6) = found, shared, fresh, blocks looked at, stored bytes of the fresh blocks, refuted candidates;
        d_status, one entry per resource of the stores back to back and then of ``new``, is MSCOMP_OK, MSCOMP_ARG_ERROR (a broken
        block_first entry, or no room within n_blocks_total or n_blocks_new) or MSCOMP_DATA_ERROR (a wrong block count, a broken block_off
        entry): a refused resource of a store brings no blocks, one of ``new`` has no extents."""
        if len(stores) != self.n_src:
            raise ValueError("one store per n_src")
        views = _blocks_views(list(stores) + [new])
        self._run("mscomp_amd_deduper_match", views if self.n_src else None, C.byref(views[self.n_src]), d_delta_ext_first, d_delta_ext, d_patch_ext_first,
                  d_patch_ext, d_class, d_count, d_status)


    @classmethod
    def for_repair(cls, ctx, block_size, n_src, n_res, n_blocks_new):
        """A deduper for repair() (mscomp_amd_deduper_create_repair): ``n_src`` (1 .. 4) sources, the primary first, whose ``n_res``
        resources have at most ``n_blocks_new`` rows in all. Its scratch is diff's: 32 bytes per resource, 4 per row and 64 per
        SPLICE_ROW_TILE of them, + 72. It refuses dedup(), diff() and match(), as dedupers made for those refuse repair()."""
        self = cls.__new__(cls)
        _Handle.__init__(self, ctx)
        self.block_size, self.n_src, self.n_res, self.n_blocks_new = int(block_size), int(n_src), int(n_res), int(n_blocks_new)
        self.n_res_total, self.n_blocks_total = self.n_res, self.n_blocks_new
        self._make("mscomp_amd_deduper_create_repair", self.block_size, self.n_src, self.n_res, self.n_blocks_new, 0)
        return self

    def repair(self, sources, d_verdicts, d_ext_first, d_ext, d_fixed, d_lost, d_count, d_status):
        """``sources``: n_src sources as BlockSplicer.splice takes them, the primary first; ``d_verdicts``: per source the d_verdict array
        BlockContainer.salvage wrote for it (int32, one entry per table row). Row k of resource r is taken from the lowest source whose
        row is MSCOMP_AMD_BLOCK_GOOD -- a mirror counts only where it has the resource with the primary's length and, when every source
        has checksums, the primary's CRC word --; a row no source has is lost and stays the primary's. The answer is one extent list in
        the form BlockSplicer.splice_extents takes over the same sources: d_ext_first (n_res + 1), d_ext (4 n_blocks_new). d_fixed /
        d_lost (n_res) = the rows taken from a mirror / lost, d_count (4) = rows fixed, rows lost, stored bytes of the fixed rows,
        resources with a lost row; d_status[r] is MSCOMP_OK, MSCOMP_DATA_ERROR (a lost row, or a wrong block count) or MSCOMP_ARG_ERROR
        (no such resource, a broken block_first entry, or no room within n_blocks_new), a refused resource having no extents."""
        if len(sources) != self.n_src or len(d_verdicts) != self.n_src:
            raise ValueError("one source and one verdict array per n_src")
        q = (C.c_void_p * self.n_src)(*[None if t is None else t.data_ptr() for t in d_verdicts])
        self._run("mscomp_amd_deduper_repair", _blocks_views(sources), q, d_ext_first, d_ext, d_fixed, d_lost, d_count, d_status)


def _diff_pairs(base, new, pairs):
    """the pairs of blocks_diff as (base resource or MSCOMP_AMD_DIFF_NO_BASE, new resource) of 64 bits each"""
    M64 = MSCOMP_AMD_DIFF_NO_BASE
    if pairs is None:
        nb = len(base[3])
        pairs = [(r if r < nb else None, r) for r in range(len(new[3]))]
    return [(M64 if a is None else int(a) & M64, int(b) & M64) for a, b in pairs]


def _extent_lists(first, ext, n):
    """host lists, one per new resource, of (source, resource, first block, block count): what blocks_splice_extents takes"""
    rows = [tuple(int(x) for x in e) for e in ext.reshape(-1, 4)[: int(first[n])]]
    return [rows[int(first[p]): int(first[p + 1])] for p in range(n)]


def blocks_diff(base, new, block_size, pairs=None, ctx=None):
    """The blocks of ``new`` that differ from the blocks at the same index of ``base`` on the GPU (BlockDeduper.diff), no block decoded:
    two containers of one format and ``block_size`` as blocks_splice takes one -- (packed, block_first, block_off, lengths, block_crc or
    None) --, ``pairs`` a list of (base resource or None, new resource), by default (r, r) for the common resources and (None, r) for the
    new resources behind the base's last. Returns host lists (delta_resources, patch_resources, changed, counts, statuses): the two
    resource lists have the shape blocks_splice_extents takes -- blocks_splice_extents([new], delta_resources, block_size) is the delta
    container, blocks_patch(base, delta, patch_resources, block_size) the new resources again."""
    import torch
    B = int(block_size)
    pr = _diff_pairs(base, new, pairs)
    n = len(pr)
    new_lens = [int(x) for x in new[3]]
    nbn = sum((new_lens[b] + B - 1) // B for _, b in pr if b < len(new_lens))
    with_crc = base[4] is not None and new[4] is not None
    with _call(ctx) as (ctx, dev):
        srcs, _, _ = _upload_containers((base, new), dev, with_crc)
        dd = BlockDeduper.for_diff(ctx, B, n, nbn)
        d_pair = _dev_u64(np.array(pr, dtype=np.uint64).reshape(-1), 2, dev)
        d_df, d_pf = torch.zeros(n + 1, dtype=torch.int64, device=dev), torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_de, d_pe = torch.zeros(max(1, 4 * nbn), dtype=torch.int64, device=dev), torch.zeros(max(1, 4 * nbn), dtype=torch.int64, device=dev)
        d_ch, d_cnt = torch.zeros(max(1, n), dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
        d_st = torch.zeros(max(1, n), dtype=torch.int32, device=dev)
        dd.diff(srcs[0], srcs[1], d_pair, d_df, d_de, d_pf, d_pe, d_ch, d_cnt, d_st)
        ctx.stream.synchronize()
        u64 = lambda t: t.cpu().numpy().view(np.uint64)
        delta, patch = _extent_lists(u64(d_df), u64(d_de), n), _extent_lists(u64(d_pf), u64(d_pe), n)
        changed, counts, st = [int(x) for x in u64(d_ch)[:n]], [int(x) for x in u64(d_cnt)], [int(x) for x in d_st.cpu().numpy()[:n]]
        dd.close()
    return delta, patch, changed, counts, st


def blocks_delta(base, new, block_size, pairs=None, ctx=None):
    """The delta container of ``new`` against ``base`` -- per pair the changed blocks of the new resource, in order -- together with the
    recipe that rebuilds the new resources from base + delta: blocks_diff, then blocks_splice_extents over [new]. Returns (delta,
    patch_resources, changed, counts, statuses), delta = (packed, block_first, block_off, lengths, block_crc or None): a container as
    blocks_patch and blocks_splice take one."""
    with _call(ctx, enter=False) as (ctx, _):
        delta_res, patch_res, changed, counts, st = blocks_diff(base, new, block_size, pairs=pairs, ctx=ctx)
        with_crc = base[4] is not None and new[4] is not None
        packed, first, off, lens, crc, _ = blocks_splice_extents([new if with_crc else tuple(new[:4]) + (None,)], delta_res, block_size, ctx=ctx)
    return (packed, first, off, lens, crc), patch_res, changed, counts, st


def blocks_patch(base, delta, patch_resources, block_size, ctx=None):
    """The new resources from ``base`` and the ``delta`` container and ``patch_resources`` of blocks_delta:
    blocks_splice_extents([base, delta], patch_resources, block_size). Returns what blocks_splice returns."""
    return blocks_splice_extents([base, delta], patch_resources, block_size, ctx=ctx)


def blocks_repair(fmt, containers, block_size, ctx=None, _verdicts0=None):
    """Mend a damaged block container from up to three copies on the GPU: ``containers`` = [primary, mirror, ...], each (packed,
    block_first, block_off, lengths, block_crc or None) of format ``fmt`` and ``block_size``. The primary is salvaged (blocks_salvage); each
    mirror is salvaged only in the rows the primary lacks when its lengths are the primary's, and whole otherwise; BlockDeduper.repair
    picks every row's source and blocks_splice_extents builds the container. Returns (container, report): container = (packed,
    block_first, block_off, lengths, block_crc or None) as the other calls take one; report = a dict with the verdict arrays
    ("verdicts", one per container), the extent lists ("resources"), "fixed" and "lost" per resource, "counts" (rows fixed, rows
    lost, stored bytes of the fixed rows, resources with a lost row) and "statuses" (MSCOMP_OK: whole again; MSCOMP_DATA_ERROR: rows
    lost, which stay the primary's)."""
    import torch
    B = int(block_size)
    with_crc = all(c[4] is not None for c in containers)
    lens0 = [int(x) for x in containers[0][3]]
    n = len(lens0)
    nbn = sum((L + B - 1) // B for L in lens0)
    with _call(ctx, enter=False) as (ctx, dev):
        verdicts = []
        for i, (packed, first, off, lens, crc) in enumerate(containers):
            same = i > 0 and [int(x) for x in lens] == lens0
            if i == 0 and _verdicts0 is not None:                   # (blocks_rebuild has salvaged the primary already)
                verdicts.append(_verdicts0)
                continue
            verdicts.append(blocks_salvage(fmt, packed, first, off, lens, B, ctx=ctx, block_crc=crc, only=verdicts[0] if same else None)[1])
        with torch.cuda.device(ctx.device), torch.cuda.stream(ctx.stream):
            srcs, _, _ = _upload_containers(containers, dev, with_crc)
            d_ver = [_dev_block_crc(v, len(v), dev) for v in verdicts]
            dd = BlockDeduper.for_repair(ctx, B, len(containers), n, nbn)
            d_ef, d_ext = torch.zeros(n + 1, dtype=torch.int64, device=dev), torch.zeros(max(1, 4 * nbn), dtype=torch.int64, device=dev)
            d_fix, d_lost = torch.zeros(max(1, n), dtype=torch.int64, device=dev), torch.zeros(max(1, n), dtype=torch.int64, device=dev)
            d_cnt, d_st = torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(max(1, n), dtype=torch.int32, device=dev)
            dd.repair(srcs, d_ver, d_ef, d_ext, d_fix, d_lost, d_cnt, d_st)
            ctx.stream.synchronize()
            u64 = lambda t: t.cpu().numpy().view(np.uint64)
            resources = _extent_lists(u64(d_ef), u64(d_ext), n)
            report = {"verdicts": verdicts, "resources": resources, "fixed": [int(x) for x in u64(d_fix)[:n]], "lost": [int(x) for x in u64(d_lost)[:n]],
                      "counts": [int(x) for x in u64(d_cnt)], "statuses": [int(x) for x in d_st.cpu().numpy()[:n]]}
            dd.close()
        cons = containers if with_crc else [tuple(c[:4]) + (None,) for c in containers]
        packed, first, off, lens, crc, _ = blocks_splice_extents(cons, resources, B, ctx=ctx)
    return (packed, first, off, lens, crc), report


def blocks_match(stores, new, block_size, ctx=None):
    """For every block of ``new``, whether an equal block lies anywhere in one of the ``stores`` (0 .. 3 of them), earlier in ``new`` or
    nowhere, on the GPU (BlockDeduper.match), no block decoded: containers of one format and ``block_size`` as blocks_splice takes them.
    Returns host lists (delta_resources, patch_resources, classes, counts, statuses): the two resource lists have the shape
    blocks_splice_extents takes -- blocks_splice_extents([new], delta_resources, block_size) is the delta container of the blocks seen for
    the first time, blocks_match_patch(stores, delta, patch_resources, block_size) the resources of ``new`` again --, classes one (found,
    shared, fresh) per resource of ``new``, counts the six of BlockDeduper.match, statuses one per resource of the stores back to back
    and then of ``new``."""
    import torch
    B = int(block_size)
    cons = list(stores) + [new]
    with_crc = all(c[4] is not None for c in cons)
    with _call(ctx) as (ctx, dev):
        srcs, n_all, rows_all = _upload_containers(cons, dev, with_crc)
        n, nbn = srcs[-1][6], srcs[-1][7]
        dd = BlockDeduper.for_match(ctx, B, len(stores), n_all, rows_all, nbn)
        d_df, d_pf = torch.zeros(n + 1, dtype=torch.int64, device=dev), torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_de, d_pe = torch.zeros(max(1, 4 * nbn), dtype=torch.int64, device=dev), torch.zeros(max(1, 4 * nbn), dtype=torch.int64, device=dev)
        d_cl, d_cnt = torch.zeros(max(1, 3 * n), dtype=torch.int64, device=dev), torch.zeros(6, dtype=torch.int64, device=dev)
        d_st = torch.zeros(max(1, n_all), dtype=torch.int32, device=dev)
        dd.match(srcs[:-1], srcs[-1], d_df, d_de, d_pf, d_pe, d_cl, d_cnt, d_st)
        ctx.stream.synchronize()
        u64 = lambda t: t.cpu().numpy().view(np.uint64)
        delta, patch = _extent_lists(u64(d_df), u64(d_de), n), _extent_lists(u64(d_pf), u64(d_pe), n)
        classes = [tuple(int(x) for x in row) for row in u64(d_cl)[: 3 * n].reshape(-1, 3)]
        counts, st = [int(x) for x in u64(d_cnt)], [int(x) for x in d_st.cpu().numpy()[:n_all]]
        dd.close()
    return delta, patch, classes, counts, st


def blocks_match_delta(stores, new, block_size, ctx=None):
    """The delta container of ``new`` against the ``stores`` -- per resource the blocks no store holds and ``new`` has not held before, in
    order -- together with the recipe that rebuilds ``new`` from stores + delta: blocks_match, then blocks_splice_extents over [new].
    Returns (delta, patch_resources, classes, counts, statuses), delta = (packed, block_first, block_off, lengths, block_crc or None)."""
    with _call(ctx, enter=False) as (ctx, _):
        delta_res, patch_res, classes, counts, st = blocks_match(stores, new, block_size, ctx=ctx)
        with_crc = all(c[4] is not None for c in list(stores) + [new])
        packed, first, off, lens, crc, _ = blocks_splice_extents([new if with_crc else tuple(new[:4]) + (None,)], delta_res, block_size, ctx=ctx)
    return (packed, first, off, lens, crc), patch_res, classes, counts, st


def blocks_match_patch(stores, delta, patch_resources, block_size, ctx=None):
    """The resources of the new container from the ``stores`` and the ``delta`` container and ``patch_resources`` of blocks_match_delta:
    blocks_splice_extents(stores + [delta], patch_resources, block_size). Returns what blocks_splice returns."""
    return blocks_splice_extents(list(stores) + [delta], patch_resources, block_size, ctx=ctx)


def blocks_single_instance(container, block_size, ctx=None):
    """``container`` with every block stored once: blocks_match_delta([], container, block_size) -- the container of its unique blocks and
    the recipe (over that container alone) that blocks_match_patch([], delta, recipe, block_size) rebuilds it from."""
    return blocks_match_delta([], container, block_size, ctx=ctx)


def blocks_dedup(containers, block_size, ctx=None):
    """The duplicate resources among up to four block containers on the GPU (BlockDeduper), no block decoded: ``containers`` as
    blocks_splice takes them. Returns host lists (rep, new_index, picks of the unique resources as (container, resource), counts,
    statuses): blocks_splice(containers, picks, block_size) is the merged container with one copy of everything, and resource g of the
    sources is its resource new_index[g]."""
    import torch
    with_crc = all(c[4] is not None for c in containers)
    with _call(ctx) as (ctx, dev):
        srcs, n, rows_all = _upload_containers(containers, dev, with_crc)
        dd = BlockDeduper(ctx, block_size, len(containers), n, rows_all)
        d_rep, d_idx = torch.zeros(max(1, n), dtype=torch.int64, device=dev), torch.zeros(max(1, n), dtype=torch.int64, device=dev)
        d_pick, d_cnt = torch.zeros(max(1, 2 * n), dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
        d_st = torch.zeros(max(1, n), dtype=torch.int32, device=dev)
        dd.dedup(srcs, d_rep, d_idx, d_pick, d_cnt, d_st)
        ctx.stream.synchronize()
        counts = [int(x) for x in d_cnt.cpu().numpy().view(np.uint64)]
        picks = d_pick.cpu().numpy().view(np.uint64)[: 2 * counts[0]].reshape(-1, 2)
        rep, idx, st = d_rep.cpu().numpy().view(np.uint64)[:n], d_idx.cpu().numpy().view(np.uint64)[:n], d_st.cpu().numpy()[:n]
        dd.close()
    return [int(x) for x in rep], [int(x) for x in idx], [(int(s), int(r)) for s, r in picks], counts, [int(x) for x in st]


class BlockTranscoder(_Handle):
    """A block transcoder (mscomp_amd_transcoder_create): a container of format ``fmt`` cut at ``block_size`` written again as format
    ``new_fmt`` cut at ``new_block_size``, out of place. Made once for the tables of a container of ``n_res`` resources whose d_block_off
    has ``n_blocks_table`` + 1 entries, a new table of ``n_blocks_new`` rows and at most ``groups_max`` worked groups per call (a group: an
    aligned span of max(block_size, new_block_size) bytes of a resource in which anything is decoded or encoded). Between two LZNT1
    containers most blocks are carried: their stored bytes move as they lie. All scratch is reserved here: a cache and a staging area of
    groups_max groups each, two inner dev plans and the tables. transcode() enqueues kernels on the ctx stream and nothing else (legal
    inside a capture of that stream). Arguments are torch CUDA tensors: uint8 data, int64 / uint64 tables, int32 statuses and checksums."""
    _destroy = "mscomp_amd_transcoder_destroy"

    def __init__(self, ctx, fmt, block_size, new_fmt, new_block_size, n_res, n_blocks_table, n_blocks_new, groups_max):
        _Handle.__init__(self, ctx)
        self.fmt, self.block_size, self.new_fmt, self.new_block_size = int(fmt), int(block_size), int(new_fmt), int(new_block_size)
        self.n_res, self.n_blocks_table, self.n_blocks_new, self.groups_max = int(n_res), int(n_blocks_table), int(n_blocks_new), int(groups_max)
        self._make("mscomp_amd_transcoder_create", self.fmt, self.block_size, self.new_fmt, self.new_block_size, self.n_res, self.n_blocks_table,
                   self.n_blocks_new, self.groups_max, 0)

    def transcode(self, d_packed, d_block_first, d_block_off, d_res_len, d_new_packed, d_new_block_first, d_new_block_off, d_status, d_block_crc=None,
                  d_new_block_crc=None, packed_len=None, new_cap=None):
        """The old container (d_packed, d_block_first, d_block_off, d_res_len, d_block_crc) is only read; the new one is written to
        d_new_packed (nothing at or behind ``new_cap``, default: all of it), d_new_block_first (n_res + 1), d_new_block_off
        (n_blocks_new + 1) and d_new_block_crc (given exactly when d_block_crc is). d_status[r] is MSCOMP_OK, MSCOMP_DATA_ERROR (a wrong
        block count, a broken table entry or chunk header, a block that does not decode or not to its checksum), MSCOMP_ARG_ERROR (no room
        in the new table, or over the budget of groups_max) with resource r left without blocks, or MSCOMP_BUF_ERROR (a block did not fit
        below new_cap)."""
        plen, cap = _byte_bounds(d_packed, packed_len, d_new_packed, new_cap)
        self._run("mscomp_amd_transcoder_transcode", d_packed, plen, d_block_first, d_block_off, d_res_len, d_block_crc, d_new_packed, cap,
                  d_new_block_first, d_new_block_off, d_new_block_crc, d_status)

    def counts(self):
        """(new blocks carried, source blocks decoded, new blocks encoded) of the last transcode(); synchronizes the stream."""
        return _three_counts(self, "mscomp_amd_transcoder_counts")


def blocks_transcode(container, block_size, new_block_size, new_fmt=None, ctx=None, groups_max=None, n_blocks_new=None, new_cap=None):
    """Bring a block container to another block size and / or codec on the GPU (BlockTranscoder). ``container`` is (fmt, packed,
    block_first, block_off, lengths, block_crc or None) as blocks_compress and blocks_crc return them; ``new_fmt`` defaults to fmt. The new
    container gets checksums exactly when the old one has them. ``groups_max`` (default: every group of the container), ``n_blocks_new``
    (default: what the lengths need) and ``new_cap`` (default: the sum of the lengths) are the transcoder's bounds. Returns numpy arrays
    and lists (new_packed uint8, new_block_first uint64 of n + 1, new_block_off uint64, new_block_crc uint32 or None, statuses, counts)."""
    import torch
    fmt, packed, block_first, block_off, lengths, block_crc = container
    new_fmt = fmt if new_fmt is None else new_fmt
    lens = [int(x) for x in lengths]
    n = len(lens)
    B1, B2 = int(block_size), int(new_block_size)
    G = max(B1, B2)
    nbt = max(0, len(np.asarray(block_off).reshape(-1)) - 1)
    nbn = sum((x + B2 - 1) // B2 for x in lens) if n_blocks_new is None else int(n_blocks_new)
    gmax = sum((x + G - 1) // G for x in lens) if groups_max is None else int(groups_max)
    room = int(sum(lens)) if new_cap is None else int(new_cap)
    with _call(ctx) as (ctx, dev):
        tc = BlockTranscoder(ctx, fmt, B1, new_fmt, B2, n, nbt, nbn, gmax)
        packed, d_packed = _dev_packed(packed, dev)
        d_first, d_boff, d_len = _dev_u64(block_first, n + 1, dev), _dev_u64(block_off, nbt + 1, dev), _dev_u64(lens, 1, dev)
        d_crc = None if block_crc is None else _dev_block_crc(block_crc, nbt, dev)
        d_new, d_nfirst, d_noff, d_ncrc = _new_container(dev, n, nbn, room, block_crc is not None)
        d_st = torch.zeros(max(1, n), dtype=torch.int32, device=dev)
        tc.transcode(d_packed, d_first, d_boff, d_len, d_new, d_nfirst, d_noff, d_st, d_block_crc=d_crc, d_new_block_crc=d_ncrc,
                     packed_len=len(packed), new_cap=room)
        counts = tc.counts()
        new_packed, nfirst, noff, ncrc = _fetch_container(d_new, d_nfirst, d_noff, d_ncrc, room)
        h_st = d_st.cpu().numpy()
        tc.close()
    return new_packed, nfirst, noff, ncrc, [int(x) for x in h_st[:n]], counts


class BlockSyncer(_Handle):
    """A block syncer (mscomp_amd_syncer_create): the blocks of ONE store container of format ``fmt`` and ``block_size`` -- ``n_res``
    resources, ``n_blocks_table`` table rows, checksums required -- found at any byte offset of up to ``n_units`` raw units of
    ``in_total_max`` bytes together, by a rolling CRC-32 over every position; at most ``n_cand_max`` candidates are kept, confirmed byte
    for byte against the decoded store blocks and answered. All scratch is reserved here: a reader's for n_cand_max requests of one block
    each, and 8 n_res + 12 per slot of the key table (2 n_blocks_table + 64 rounded up to a power of two) + 40 n_units + 56 n_cand_max +
    68 per MSCOMP_AMD_SYNC_TILE bytes of input + 4 per 64 bytes + 38064 bytes of tables. sync() enqueues kernels on the ctx stream and nothing else (legal inside a capture of that stream)."""
    _destroy = "mscomp_amd_syncer_destroy"

    def __init__(self, ctx, fmt, block_size, n_res, n_blocks_table, n_units, in_total_max, n_cand_max):
        _Handle.__init__(self, ctx)
        self.fmt, self.block_size, self.n_res, self.n_blocks_table = int(fmt), int(block_size), int(n_res), int(n_blocks_table)
        self.n_units, self.in_total_max, self.n_cand_max = int(n_units), int(in_total_max), int(n_cand_max)
        self._make("mscomp_amd_syncer_create", self.fmt, self.block_size, self.n_res, self.n_blocks_table, self.n_units, self.in_total_max,
                   self.n_cand_max, 0)

    def sync(self, store, d_in, d_in_off, d_in_len, d_hit_first, d_req, d_req_off, d_lit_first, d_lit, d_count, d_res_status, d_status):
        """``store``: one source as BlockSplicer.splice takes them, with its checksums. Unit u = the d_in_len[u] bytes at d_in +
        d_in_off[u]. The answer is a recipe: hit i -- d_hit_first (n_units + 1) counts them per unit -- says that the block_size bytes
        at d_req_off[i] of the batch are the bytes of request d_req[3 i ..] = (resource, offset, block_size) of the store, in the form
        BlockReader.read takes both arrays; the literal runs d_lit[2 i ..] = (offset in the batch, length), counted by d_lit_first, are
        the bytes no hit covers. d_count (8): raw candidates, thinned, kept, confirmed, hits, literal runs, literal bytes, distinct rows;
        d_res_status one entry per resource of the store, d_status one per unit (MSCOMP_ARG_ERROR: over in_total_max)."""
        self._run("mscomp_amd_syncer_sync", _blocks_views([store]), d_in, d_in_off, d_in_len, d_hit_first, d_req, d_req_off, d_lit_first, d_lit, d_count,
                  d_res_status, d_status)

    def counts(self):
        """(kept candidates, distinct rows, hits) of the last sync(); synchronizes the stream. A digest syncer hashes every kept window
        once: its second count is the kept count."""
        return _three_counts(self, "mscomp_amd_syncer_counts")

    @classmethod
    def for_digest(cls, ctx, block_size, n_res, n_blocks_table, n_units, in_total_max, n_cand_max):
        """A syncer that confirms by digest (mscomp_amd_syncer_create_digest): the same bounds without a format. No reader core is
        reserved -- no inner plan, no cache of n_cand_max blocks --: the syncer's own tables and n_cand_max (16 block_size / 1024 + 32)
        + 64 bytes. Only sync_digest() runs on it."""
        self = cls.__new__(cls)
        _Handle.__init__(self, ctx)
        self.fmt, self.block_size, self.n_res, self.n_blocks_table = None, int(block_size), int(n_res), int(n_blocks_table)
        self.n_units, self.in_total_max, self.n_cand_max = int(n_units), int(in_total_max), int(n_cand_max)
        self._make("mscomp_amd_syncer_create_digest", self.block_size, self.n_res, self.n_blocks_table, self.n_units, self.in_total_max, self.n_cand_max, 0)
        return self

    def sync_digest(self, store, d_block_digest, d_in, d_in_off, d_in_len, d_hit_first, d_req, d_req_off, d_lit_first, d_lit, d_count, d_res_status,
                    d_status):
        """sync() on a syncer made by for_digest: a kept candidate is confirmed when the digest of its window of the new data equals the
        four words of ``d_block_digest`` (int32, 4 per table row, as BlockDigester.blocks writes them) at its row. The store's bytes are
        never read -- its d_packed may be None --, its checksums still are: the scan is built from them. d_count[7] = the kept count."""
        self._run("mscomp_amd_syncer_sync_digest", _blocks_views([store]), d_block_digest, d_in, d_in_off, d_in_len, d_hit_first, d_req, d_req_off,
                  d_lit_first, d_lit, d_count, d_res_status, d_status)


class BlockDigester(_Handle):
    """A block digester (mscomp_amd_digester_create): the 128-bit BLAKE2s tree digest of every block of ``block_size`` bytes of up to
    ``n_res`` resources of ``in_total_max`` bytes together -- over the blocks' DATA, like the checksums. A digest is four int32 words;
    viewed as bytes they are the hash. ``n_blocks_max`` = n_res + in_total_max // block_size. All scratch is reserved here:
    n_blocks_max (16 block_size / 1024 + 56) + 20 n_res + 72 bytes. Both calls enqueue kernels on the ctx stream and nothing else."""
    _destroy = "mscomp_amd_digester_destroy"

    def __init__(self, ctx, block_size, n_res, in_total_max):
        _Handle.__init__(self, ctx)
        self.block_size, self.n_res, self.in_total_max = int(block_size), int(n_res), int(in_total_max)
        self._make("mscomp_amd_digester_create", self.block_size, self.n_res, self.in_total_max, 0)
        self.n_blocks_max = self.n_res + self.in_total_max // self.block_size

    def blocks(self, d_data, d_res_off, d_res_len, d_block_digest, d_status):
        """As BlockContainer.crc, a digest for a checksum: d_block_digest (int32, 4 n_blocks_max; entry j belongs to the block compress puts at
        d_block_off[j], the entries behind the last block are zeros) and d_status (n_res: MSCOMP_OK, or MSCOMP_ARG_ERROR past in_total_max)."""
        self._run("mscomp_amd_digester_blocks", d_data, d_res_off, d_res_len, d_block_digest, d_status)

    def check(self, d_out, d_out_off, d_res_len, d_block_first, d_block_digest, d_out_len, d_status, d_range=None):
        """As BlockContainer.check: every block of the (clipped) range of every resource that is MSCOMP_OK in d_status is read back from
        d_out and held to d_block_digest; a mismatch turns the resource into MSCOMP_DATA_ERROR with d_out_len = 0."""
        self._run("mscomp_amd_digester_check", d_out, d_out_off, d_res_len, d_block_first, d_range, d_block_digest, d_out_len, d_status)


def blocks_digest(buffers, block_size, ctx=None):
    """The digest column of a list of byte strings (one resource each), computed on the GPU (BlockDigester): a numpy uint32 array of
    shape (nb, 4) in the block order of blocks_compress; row j viewed as bytes is the BLAKE2s tree digest of block j."""
    import torch
    n = len(buffers)
    with _call(ctx) as (ctx, dev):
        d_in, d_off, d_len, lens = _upload_unit_tables(buffers, dev)
        dg = BlockDigester(ctx, block_size, n, int(sum(lens)))
        d_dig = torch.zeros(max(1, 4 * dg.n_blocks_max), dtype=torch.int32, device=dev)
        d_st = torch.zeros(max(1, n), dtype=torch.int32, device=dev)
        dg.blocks(d_in, d_off, d_len, d_dig, d_st)
        ctx.stream.synchronize()
        nb = sum((x + block_size - 1) // block_size for x in lens)
        out = d_dig.cpu().numpy().view(np.uint32)[: 4 * nb].reshape(nb, 4).copy()
        dg.close()
    return out


def _dev_block_digest(block_digest, n, dev):
    """``block_digest`` (rows of four words) cut or zero-padded to ``n`` rows (one at least), as an int32 device tensor of 4 n words."""
    import torch
    h = np.zeros(4 * max(1, n), dtype=np.uint32)
    a = np.asarray(block_digest, dtype=np.uint32).reshape(-1)
    k = min(len(a), 4 * n)
    h[:k] = a[:k]
    return torch.from_numpy(h.view(np.int32).copy()).to(dev)


def blocks_sync(store, buffers, block_size, n_cand_max=None, ctx=None, fmt=None, block_digest=None):
    """Find the blocks of the container ``store`` = (packed, block_first, block_off, lengths, block_crc), written in format ``fmt`` at
    ``block_size``, at any byte offset of the raw ``buffers`` on the GPU (BlockSyncer). ``n_cand_max`` defaults to a bound no input
    reaches short of periodic floods: two candidates per block of input and eight per buffer. Returns host lists (hits, literals,
    counts, res_statuses, statuses): hits[u] = [(p, r, k)] -- the block_size bytes at p of buffer u are block k of resource r of the
    store --, literals[u] = [(p, length)] the stretches no hit covers. ``block_digest`` (as blocks_digest returns it for the store's data):
    the candidates are confirmed by digest instead (BlockSyncer.for_digest) -- no stored byte is read, and ``fmt`` is not needed."""
    import torch
    if fmt is None and block_digest is None:
        raise ValueError("fmt: the format the store was written in (its blocks are decoded)")
    B = int(block_size)
    bufs = [bytes(b) for b in buffers]
    nu, total = len(bufs), sum(len(b) for b in bufs)
    nc = 2 * (total // B) + 8 * nu if n_cand_max is None else int(n_cand_max)
    with _call(ctx) as (ctx, dev):
        srcs, n, rows = _upload_containers([store], dev, True)
        d_in, in_off, lens = _upload_units(bufs, dev)
        d_off, d_len = _dev_u64(in_off, 1, dev), _dev_u64(lens, 1, dev)
        sy = BlockSyncer(ctx, fmt, B, n, rows, nu, total, nc) if block_digest is None else BlockSyncer.for_digest(ctx, B, n, rows, nu, total, nc)
        z64 = lambda k: torch.zeros(max(1, k), dtype=torch.int64, device=dev)
        d_hf, d_req, d_roff, d_lf, d_lit, d_cnt = z64(nu + 1), z64(3 * nc), z64(nc), z64(nu + 1), z64(2 * (nc + nu)), z64(8)
        d_rst, d_st = torch.zeros(max(1, n), dtype=torch.int32, device=dev), torch.zeros(max(1, nu), dtype=torch.int32, device=dev)
        if block_digest is None:
            sy.sync(srcs[0], d_in, d_off, d_len, d_hf, d_req, d_roff, d_lf, d_lit, d_cnt, d_rst, d_st)
        else:
            sy.sync_digest(srcs[0], _dev_block_digest(block_digest, rows, dev), d_in, d_off, d_len, d_hf, d_req, d_roff, d_lf, d_lit, d_cnt, d_rst, d_st)
        ctx.stream.synchronize()
        u64 = lambda t: t.cpu().numpy().view(np.uint64)
        hf, req, roff, lf, lit, cnt = u64(d_hf), u64(d_req), u64(d_roff), u64(d_lf), u64(d_lit), u64(d_cnt)
        rst, st = [int(x) for x in d_rst.cpu().numpy()[:n]], [int(x) for x in d_st.cpu().numpy()[:nu]]
        sy.close()
    hits = [[(int(roff[i]) - int(in_off[u]), int(req[3 * i]), int(req[3 * i + 1]) // B) for i in range(int(hf[u]), int(hf[u + 1]))] for u in range(nu)]
    lits = [[(int(lit[2 * i]) - int(in_off[u]), int(lit[2 * i + 1])) for i in range(int(lf[u]), int(lf[u + 1]))] for u in range(nu)]
    return hits, lits, [int(x) for x in cnt], rst, st


def blocks_sync_delta(store, buffers, block_size, n_cand_max=None, ctx=None, fmt=None, block_digest=None):
    """What has to travel to rebuild ``buffers`` where ``store`` is: blocks_sync, then the literal bytes cut out of the buffers. Returns
    (recipe, literal_bytes): recipe = (lengths, hits, literals) as blocks_sync returns them, literal_bytes the runs' bytes back to back in
    (buffer, position) order. ``block_digest``: as for blocks_sync -- confirmed by digest, without ``fmt``."""
    hits, lits, _, _, st = blocks_sync(store, buffers, block_size, n_cand_max=n_cand_max, ctx=ctx, fmt=fmt, block_digest=block_digest)
    if any(st):
        raise MSCompError(next(s for s in st if s), "blocks_sync")
    data = b"".join(bytes(b)[p: p + ln] for b, runs in zip(buffers, lits) for p, ln in runs)
    return ([len(b) for b in buffers], hits, lits), data


def blocks_sync_patch(store, recipe, literal_bytes, block_size, ctx=None, fmt=None, block_digest=None):
    """The buffers of blocks_sync_delta again: the hits read from ``store`` on the GPU (blocks_read, every block held to its checksum),
    the literal runs taken from ``literal_bytes``. Returns the list of buffers. ``block_digest`` (the store's digest column): the blocks
    read are held to their digests too (blocks_digest over them), MSCOMP_DATA_ERROR otherwise; reading still decodes, so ``fmt`` stays."""
    if fmt is None:
        raise ValueError("fmt: the format the store was written in (its blocks are decoded)")
    lengths, hits, lits = recipe
    B = int(block_size)
    packed, first, off, lens, crc = store
    reqs = [(r, k * B, B) for hs in hits for _, r, k in hs]
    got, st = blocks_read(fmt, packed, first, off, lens, B, reqs, ctx=ctx, block_crc=crc) if reqs else ([], [])
    if any(st):
        raise MSCompError(next(s for s in st if s), "blocks_read")
    if block_digest is not None and reqs:
        want = np.asarray(block_digest, dtype=np.uint32).reshape(-1, 4)
        rows = [int(first[r]) + k for hs in hits for _, r, k in hs]
        if not np.array_equal(blocks_digest(got, B, ctx=ctx), want[rows]):
            raise MSCompError(MSCOMP_DATA_ERROR, "blocks_digest")
    out, at, q = [], 0, 0
    for L, hs, runs in zip(lengths, hits, lits):
        buf = bytearray(L)
        for p, _, _ in hs:
            buf[p: p + B] = got[q]
            q += 1
        for p, ln in runs:
            buf[p: p + ln] = literal_bytes[at: at + ln]
            at += ln
        out.append(bytes(buf))
    return out


class BlockParity(_Handle):
    """Reed-Solomon parity rows beside a block container (mscomp_amd_parity_create): ``m`` (1 .. 3) parity rows for every ``k`` (1 .. 255)
    stored rows of a table of ``n_blocks_table`` rows, over the STORED bytes -- no format, no decoder --, and up to m lost rows per group
    back from them without a mirror. GF(2^8), polynomial 0x11D, alpha = 2: P_p = XOR_i alpha^(p i) D_i. Groups are interleaved: with nb
    rows and G = ceil(nb / k) groups, row j is member j // G of group j % G. All scratch is reserved here: 28 bytes per parity row of
    m ceil(n_blocks_table / k), 12 per table row, 24 per group, + 72. Both calls enqueue kernels on the ctx stream and nothing else."""
    _destroy = "mscomp_amd_parity_destroy"

    def __init__(self, ctx, block_size, n_blocks_table, k, m):
        _Handle.__init__(self, ctx)
        self.block_size, self.n_blocks_table, self.k, self.m = int(block_size), int(n_blocks_table), int(k), int(m)
        self._make("mscomp_amd_parity_create", self.block_size, self.n_blocks_table, self.k, self.m, 0)

    def bound(self):
        """(parity rows, parity bytes) a build writes at most: m G_max and m G_max block_size"""
        out = (C.c_uint64 * 2)()
        self._run("mscomp_amd_parity_bound", out)           # (answers 0 or MSCOMP_ERRNO)
        return int(out[0]), int(out[1])

    def build(self, source, d_par, d_par_off, d_par_crc, d_row_len, d_par_head, d_status, par_cap=None):
        """``source``: the container as BlockSplicer.splice takes one. Writes the parity set: d_par (uint8, 16-byte aligned; ``par_cap``
        bytes of it, by default all), d_par_off (int64, rows + 1), d_par_crc (int32, rows: zlib's CRC-32 of every parity row), d_row_len
        (int32, n_blocks_table: the stored length the parity was taken over, 0 for a row the table refuses), d_par_head (int64, 4: nb,
        G, k, m) and d_status (int32, 1: MSCOMP_OK; MSCOMP_BUF_ERROR when a parity row ends beyond par_cap -- it is not written, the
        tables hold the full layout --; MSCOMP_ARG_ERROR when the container has more rows than n_blocks_table or a table of another size)."""
        cap = (0 if d_par is None else d_par.numel()) if par_cap is None else int(par_cap)
        if d_par is not None and cap > d_par.numel():
            raise ValueError("par_cap exceeds d_par")
        self._run("mscomp_amd_parity_build", _blocks_views([source]), d_par, cap, d_par_off, d_par_crc, d_row_len, d_par_head, d_status)

    def rebuild(self, source, d_verdict, d_par, d_par_off, d_par_crc, d_row_len, d_par_head, d_fix_packed, d_fix_block_off, d_fix_verdict, d_count,
                d_status, par_len=None, fix_cap=None):
        """``source`` and ``d_verdict``: the damaged container and the verdicts BlockContainer.salvage gave for it; then the parity set as
        build wrote it. A row is missing when its verdict is not GOOD or its table entries are not what d_row_len says; a group with e
        missing rows and at least e parity rows that pass their CRC-32 gets them back. The answer is a SPARSE MIRROR: d_fix_packed (the
        rebuilt rows' stored bytes in row order, ``fix_cap`` bytes of it at most), d_fix_block_off (int64, n_blocks_table + 1: stored
        length 0 for every row not rebuilt) and d_fix_verdict (int32, n_blocks_table: GOOD for a row rebuilt and written, SKIPPED
        otherwise) -- see fix_view. d_count (int64, 6) = rows missing, rows rebuilt, groups with a missing row, groups unrecoverable,
        parity rows unusable, stored bytes rebuilt; d_status (int32, 1) = MSCOMP_OK, MSCOMP_BUF_ERROR (a rebuilt row beyond fix_cap),
        MSCOMP_DATA_ERROR (a group lost more rows than it has usable parity; or parity of another container), MSCOMP_ARG_ERROR."""
        plen, cap = _byte_bounds(d_par, par_len, d_fix_packed, fix_cap)
        self._run("mscomp_amd_parity_rebuild", _blocks_views([source]), d_verdict, d_par, plen, d_par_off, d_par_crc, d_row_len, d_par_head, d_fix_packed, cap,
                  d_fix_block_off, d_fix_verdict, d_count, d_status)

    @staticmethod
    def fix_view(source, d_fix_packed, d_fix_block_off, fix_len=None):
        """The sparse mirror rebuild wrote, as a source of BlockDeduper.repair and BlockSplicer.splice_extents beside ``source`` (the
        primary, a full source tuple): its d_block_first, d_res_len and d_block_crc with the fix's stored bytes and offset table.
        ``fix_len``: d_fix_block_off[nb] when the caller knows it (by default all of d_fix_packed: every offset lies inside it)."""
        s = tuple(source)
        return (d_fix_packed, s[1], d_fix_block_off, s[3], s[4] if len(s) > 4 else None, d_fix_packed.numel() if fix_len is None else int(fix_len),
                s[6] if len(s) > 6 else None, s[7] if len(s) > 7 else None)


def blocks_parity(container, block_size, k, m, ctx=None):
    """The parity set of ``container`` = (packed, block_first, block_off, lengths, ...) on the GPU (BlockParity.build): (par, par_off,
    par_crc, row_len, head) as numpy arrays -- par (uint8) cut to its length par_off[-1], par_off (uint64, m G + 1), par_crc (uint32,
    m G), row_len (uint32, one per table row), head (uint64: nb, G, k, m). Keep it beside the container; blocks_rebuild takes it."""
    import torch
    packed, first, off, lens = container[:4]
    with _call(ctx) as (ctx, dev):
        srcs, _, nbt = _upload_containers([(packed, first, off, lens, None)], dev, False)
        pr = BlockParity(ctx, block_size, nbt, k, m)
        rows, room = pr.bound()
        d_par = torch.zeros(room + 16, dtype=torch.uint8, device=dev)
        d_off, d_crc = torch.zeros(rows + 1, dtype=torch.int64, device=dev), torch.zeros(max(1, rows), dtype=torch.int32, device=dev)
        d_rl, d_head, d_st = torch.zeros(max(1, nbt), dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        pr.build(srcs[0], d_par, d_off, d_crc, d_rl, d_head, d_st, par_cap=room)
        ctx.stream.synchronize()
        if int(d_st.cpu()[0]) != MSCOMP_OK:                      # (the status build wrote on the device)
            raise MSCompError(int(d_st.cpu()[0]), "mscomp_amd_parity_build")
        par_off = d_off.cpu().numpy().view(np.uint64).copy()
        out = (d_par.cpu().numpy()[: int(par_off[-1])].copy(), par_off, d_crc.cpu().numpy().view(np.uint32)[:rows].copy(),
               d_rl.cpu().numpy().view(np.uint32)[:nbt].copy(), d_head.cpu().numpy().view(np.uint64).copy())
        pr.close()
    return out


def blocks_rebuild(fmt, container, parity, block_size, ctx=None, mirrors=()):
    """Mend a damaged block container from its parity set on the GPU, without a second copy: ``container`` = (packed, block_first,
    block_off, lengths, block_crc or None), ``parity`` as blocks_parity returned it. The container is salvaged (blocks_salvage),
    BlockParity.rebuild writes the sparse mirror of the rows it can give back, and blocks_repair over [container, mirror, *mirrors] --
    which salvages the mirror in the rows the container lacks, holding every rebuilt row to its CRC-32 -- and blocks_splice_extents
    build the container. ``mirrors``: up to two real copies, asked only for what parity could not give. Returns (container, report):
    blocks_repair's, plus "rebuild_counts" (rows missing, rows rebuilt, groups with a missing row, groups unrecoverable, parity rows
    unusable, stored bytes rebuilt) and "rebuild_status"."""
    import torch
    B = int(block_size)
    packed, first, off, lens, crc = container
    par, par_off, par_crc, row_len, head = parity
    k, m = int(head[2]), int(head[3])
    with _call(ctx, enter=False) as (ctx, dev):
        ver0 = blocks_salvage(fmt, packed, first, off, lens, B, ctx=ctx, block_crc=crc)[1]
        with torch.cuda.device(ctx.device), torch.cuda.stream(ctx.stream):
            srcs, _, nbt = _upload_containers([(packed, first, off, lens, None)], dev, False)
            pr = BlockParity(ctx, B, nbt, k, m)
            rows = pr.bound()[0]
            par = np.ascontiguousarray(par, dtype=np.uint8)
            d_par = torch.zeros(len(par) + 16, dtype=torch.uint8, device=dev)
            if len(par):
                d_par[: len(par)] = torch.from_numpy(par.copy()).to(dev)
            d_poff, d_pcrc, d_rl = _dev_u64(par_off, rows + 1, dev), _dev_block_crc(par_crc, rows, dev), _dev_block_crc(row_len, nbt, dev)
            d_head, d_ver = _dev_u64(head, 4, dev), _dev_block_crc(ver0, nbt, dev)
            room = int(np.asarray(row_len, dtype=np.uint64).sum())
            d_fix, d_foff = torch.zeros(room + 16, dtype=torch.uint8, device=dev), torch.zeros(nbt + 1, dtype=torch.int64, device=dev)
            d_fver = torch.full((max(1, nbt),), MSCOMP_AMD_BLOCK_SKIPPED, dtype=torch.int32, device=dev)
            d_cnt, d_st = torch.zeros(6, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
            pr.rebuild(srcs[0], d_ver, d_par, d_poff, d_pcrc, d_rl, d_head, d_fix, d_foff, d_fver, d_cnt, d_st, par_len=len(par), fix_cap=room)
            ctx.stream.synchronize()
            fix_off = d_foff.cpu().numpy().view(np.uint64).copy()
            fix = (d_fix.cpu().numpy()[: int(fix_off[-1])].copy(), first, fix_off, lens, crc)
            counts, status = [int(x) for x in d_cnt.cpu().numpy()], int(d_st.cpu()[0])
            pr.close()
        new, report = blocks_repair(fmt, [container, fix] + list(mirrors), B, ctx=ctx, _verdicts0=ver0)
    report["rebuild_counts"], report["rebuild_status"] = counts, status
    return new, report


def res_crc_from_blocks(block_first, lengths, block_crc, block_size, ctx=None):
    """zlib's crc32 of every whole resource of a block container from its block checksums alone (mscomp_amd_res_crc_dev): no data is read.
    Returns (numpy uint32 array of n, list of status)."""
    import torch
    n = len(lengths)
    nbt = len(np.asarray(block_crc).reshape(-1))
    with _call(ctx) as (ctx, dev):
        d_first, d_len = _dev_u64(block_first, n + 1, dev), _dev_u64([int(x) for x in lengths], 1, dev)
        d_bcrc = _dev_block_crc(block_crc, nbt, dev)
        d_rcrc = torch.zeros(max(1, n), dtype=torch.int32, device=dev)
        d_st = torch.zeros(max(1, n), dtype=torch.int32, device=dev)
        res_crc_dev(ctx, block_size, n, nbt, d_first, d_len, d_bcrc, d_rcrc, d_st)
        ctx.stream.synchronize()
        out, st = d_rcrc.cpu().numpy().view(np.uint32)[:n].copy(), [int(x) for x in d_st.cpu().numpy()[:n]]
    return out, st


def res_crc_dev(ctx, block_size, n_res, n_blocks_table, d_block_first, d_res_len, d_block_crc, d_res_crc, d_status):
    """mscomp_amd_res_crc_dev on torch CUDA tensors: d_res_crc[r] (int32) = the CRC-32 of resource r from d_block_crc, d_status[r] MSCOMP_OK,
    MSCOMP_ARG_ERROR (a table entry beyond n_blocks_table) or MSCOMP_DATA_ERROR (a wrong block count). Kernels on the ctx stream only."""
    _run(ctx, "mscomp_amd_res_crc_dev", ctx._h, int(block_size), int(n_res), int(n_blocks_table), d_block_first, d_res_len, d_block_crc, d_res_crc, d_status)


def plan_paths(plan):
    """mscomp_amd_debug_plan_paths (test hook; synchronizes the stream): what the last execution of a decompress or size plan of any kind put
    on the optional paths -- (units walked by segments, units on the all-CU byte stage, candidate slots with token scratch)."""
    return _three_counts(plan, "mscomp_amd_debug_plan_paths")


def _scratch_target(target):
    """(kind, handle) of a scratch hook's target: None (the calling thread's one-shot context), a Context, a plan of any kind or a block object"""
    if target is None or isinstance(target, Context):
        return 0, (None if target is None else target._h)
    kinds = ((BlockContainer, 2), (BlockReader, 3), (BlockWriter, 4), (BlockSplicer, 5), (BlockDeduper, 6), (_Handle, 1))
    return next(k for cls, k in kinds if isinstance(target, cls)), target._h


def scratch_names():
    """mscomp_amd_debug_scratch_names (test hook, needs no device): the names of a context's scratch buffers, in a report's order."""
    lib = load_library()
    n = lib.mscomp_amd_debug_scratch_names(None, 0)
    if n < 0:
        raise MSCompError(MSCOMP_ERRNO, "mscomp_amd_debug_scratch_names")
    names = (C.c_char_p * n)()
    lib.mscomp_amd_debug_scratch_names(names, n)
    return [x.decode() for x in names]


def scratch_poison(target, byte, slack_only=False):
    """mscomp_amd_debug_scratch_poison (test hook): every buffer of ``target`` -- None, a Context, a plan, a block object -- filled with
    ``byte`` on the context's stream, whole or over its slack alone. Returns the number of buffers filled, -1 when refused."""
    kind, h = _scratch_target(target)
    return load_library().mscomp_amd_debug_scratch_poison(kind, h, 1 if slack_only else 0, int(byte))


def scratch_report(target, byte):
    """mscomp_amd_debug_scratch_report (test hook; synchronizes the stream): {name: (asked, cap, changed)} over the buffers of ``target``,
    changed = the bytes of [asked, cap) that differ from ``byte``. Raises MSCompError when refused."""
    kind, h = _scratch_target(target)
    lib = load_library()
    recs = (ScratchRec * 64)()
    n = lib.mscomp_amd_debug_scratch_report(kind, h, int(byte), recs, 64)
    if n < 0 or n > 64:
        raise MSCompError(MSCOMP_ERRNO, "mscomp_amd_debug_scratch_report")
    return {recs[i].name.decode(): (int(recs[i].asked), int(recs[i].cap), int(recs[i].changed)) for i in range(n)}


def compact_dev(ctx, d_src, d_src_off, d_len, align=1, d_packed=None, d_packed_off=None, packed_cap=None):
    """mscomp_amd_compact_dev: the d_len[i] bytes at d_src + d_src_off[i] packed in unit order into d_packed, every start rounded up to
    ``align``, the padding zeroed; d_packed_off (int64, n + 1) gets the offsets layout_dev(d_len, align) would write, the last one the total.
    All tables are device tensors; enqueued on the ctx stream, nothing is synchronized or read back. Returns (d_packed, d_packed_off) and
    allocates only the arguments left None. ``packed_cap`` is the room of d_packed in bytes (default: all of a given d_packed). When d_packed
    is None its size is ``packed_cap`` -- the total is NOT read back to size it -- or, without one, d_src.numel() + n * (align - 1): enough
    whenever the units do not overlap in d_src. A unit that ends beyond packed_cap is left out whole; d_packed_off[n] > packed_cap says so."""
    import torch
    n = d_len.numel()
    align = max(1, int(align))
    if d_packed is None:
        if packed_cap is None:
            packed_cap = d_src.numel() + n * (align - 1)
        d_packed = torch.empty(max(1, int(packed_cap)), dtype=torch.uint8, device=d_len.device)
    elif packed_cap is None:
        packed_cap = d_packed.numel()
    if int(packed_cap) > d_packed.numel():
        raise ValueError("packed_cap exceeds d_packed")
    if d_packed_off is None:
        d_packed_off = torch.empty(n + 1, dtype=torch.int64, device=d_len.device)
    _run(ctx, "mscomp_amd_compact_dev", ctx._h, n, d_src, d_src_off, d_len, align, d_packed, int(packed_cap), d_packed_off)
    return d_packed, d_packed_off


def plan_layout_dev(ctx, fmt, d_in_len, align=16, d_off=None, d_cap=None):
    """mscomp_amd_plan_layout_dev: per unit the largest compressed size of d_in_len[i] bytes in format ``fmt`` (d_cap), and their exclusive
    running sum rounded up to ``align`` (d_off, n + 1 entries, the last one the total), on the device and enqueued on the ctx stream. Returns
    (d_off, d_cap); either is allocated (int64) when not given."""
    import torch
    n = d_in_len.numel()
    if d_off is None:
        d_off = torch.empty(n + 1, dtype=torch.int64, device=d_in_len.device)
    if d_cap is None:
        d_cap = torch.empty(n, dtype=torch.int64, device=d_in_len.device)
    _run(ctx, "mscomp_amd_plan_layout_dev", ctx._h, int(fmt), n, d_in_len, int(align), d_off, d_cap)
    return d_off, d_cap


def layout_dev(ctx, d_cap, align=16, d_off=None):
    """mscomp_amd_layout_dev: the exclusive running sum of d_cap rounded up to ``align``, on the device (int64 tensor of n + 1 offsets, the
    last one the total), enqueued on the ctx stream. ``d_off`` (optional) is the tensor to write."""
    import torch
    n = d_cap.numel()
    if d_off is None:
        d_off = torch.empty(n + 1, dtype=torch.int64, device=d_cap.device)
    _run(ctx, "mscomp_amd_layout_dev", ctx._h, n, d_cap, int(align), d_off)
    return d_off


def _upload_units(units, dev):
    import torch
    lens = [len(u) for u in units]
    in_off, in_total = pack_offsets(lens)
    blob = np.zeros(in_total + 16, dtype=np.uint8)
    for u, o in zip(units, in_off):
        if len(u):
            blob[int(o): int(o) + len(u)] = np.frombuffer(bytes(u), dtype=np.uint8)
    return torch.from_numpy(blob).to(dev), in_off, lens


def _upload_unit_tables(units, dev):
    """_upload_units, with the offsets and lengths on the device too (int64, one entry at least): (d_in, d_off, d_len, lens)."""
    import torch
    d_in, in_off, lens = _upload_units(units, dev)
    d_off = torch.from_numpy(np.ascontiguousarray(in_off, dtype=np.uint64).view(np.int64).copy()).to(dev) if lens else torch.zeros(1, dtype=torch.int64, device=dev)
    return d_in, d_off, torch.tensor(lens or [0], dtype=torch.int64, device=dev), lens


def _dev_u64(a, least, dev):
    """``a`` flattened, as an int64 device tensor of ``least`` entries or more: the last one repeated (0 when there is none)."""
    import torch
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
    a = np.concatenate([a, np.full(max(0, least - len(a)), a[-1] if len(a) else 0, dtype=np.uint64)])
    return torch.from_numpy(a.view(np.int64).copy()).to(dev)


def _dev_packed(packed, dev):
    """The stored blocks of a container (bytes or a numpy array) as (numpy uint8 array, device tensor with 16 bytes of room behind it)."""
    import torch
    packed = np.ascontiguousarray(np.frombuffer(bytes(packed), dtype=np.uint8) if not isinstance(packed, np.ndarray) else packed, dtype=np.uint8)
    d_packed = torch.zeros(len(packed) + 16, dtype=torch.uint8, device=dev)
    if len(packed):
        d_packed[: len(packed)] = torch.from_numpy(packed.copy()).to(dev)
    return packed, d_packed


def _dev_block_crc(block_crc, n, dev):
    """``block_crc`` cut or zero-padded to ``n`` entries (one at least), as an int32 device tensor."""
    import torch
    h_crc = np.zeros(max(1, n), dtype=np.uint32)
    k = min(len(block_crc), len(h_crc))
    h_crc[:k] = np.asarray(block_crc, dtype=np.uint32)[:k]
    return torch.from_numpy(h_crc.view(np.int32).copy()).to(dev)


def _upload_containers(containers, dev, with_crc):
    """Containers (packed, block_first, block_off, lengths, block_crc or None) on the device, as the source tuples BlockSplicer.splice takes
    with every field stated -- checksums only ``with_crc`` --, and the resources and table rows of all of them: (sources, n_res, rows)."""
    srcs, n_all, rows_all = [], 0, 0
    for packed, first, off, lens, crc in containers:
        lens = [int(x) for x in lens]
        packed, d_packed = _dev_packed(packed, dev)
        rows = max(0, len(np.asarray(off).reshape(-1)) - 1)
        n_all += len(lens)
        rows_all += rows
        srcs.append((d_packed, _dev_u64(first, len(lens) + 1, dev), _dev_u64(off, rows + 1, dev), _dev_u64(lens, 1, dev),
                     _dev_block_crc(crc, rows, dev) if with_crc else None, len(packed), len(lens), rows))
    return srcs, n_all, rows_all


def _new_container(dev, n_new, nbt, room, with_crc):
    """The zeroed device arrays a call writes a new container into: (d_new_packed of room + 16 bytes, d_new_block_first of n_new + 1 entries --
    None for n_new None: a write keeps the old one --, d_new_block_off of nbt + 1, d_new_block_crc of nbt, one at least, or None)."""
    import torch
    return (torch.zeros(room + 16, dtype=torch.uint8, device=dev),
            None if n_new is None else torch.zeros(n_new + 1, dtype=torch.int64, device=dev),
            torch.zeros(nbt + 1, dtype=torch.int64, device=dev),
            torch.zeros(max(1, nbt), dtype=torch.int32, device=dev) if with_crc else None)


def _fetch_container(d_new, d_nfirst, d_noff, d_ncrc, room):
    """Those arrays on the host, cut to the nb blocks the new block_first counts (without one: to every row of the table): (new_packed,
    new_first uint64 or None, new_block_off uint64 of nb + 1, new_block_crc uint32 of nb or None)."""
    nfirst = None if d_nfirst is None else d_nfirst.cpu().numpy().view(np.uint64).copy()
    nb = d_noff.numel() - 1 if nfirst is None else int(nfirst[-1])
    noff = d_noff.cpu().numpy().view(np.uint64)[: nb + 1].copy()
    new_packed = d_new.cpu().numpy()[: min(int(noff[nb]), room)].copy()
    ncrc = None if d_ncrc is None else d_ncrc.cpu().numpy().view(np.uint32)[:nb].copy()
    return new_packed, nfirst, noff, ncrc


def _covering_blocks(reqs, lens, B):
    """Per (resource, offset, length) request the bytes it wants once clipped to its resource, and the blocks of ``B`` bytes that cover all
    of them, counted per request (unshared)."""
    wants, blocks = [], 0
    for r, o, ln in reqs:
        L = lens[r] if r < len(lens) else 0
        o = min(o, L)
        w = min(ln, L - o)
        wants.append(w)
        blocks += ((o + w - 1) // B - o // B + 1) if w else 0
    return wants, blocks


def decompressed_sizes(fmt, units, limits=None, ctx=None):
    """Size a list of independent compressed buffers on the GPU without decoding them. ``limits`` (optional, one per unit; default
    no limit) is the capacity each is judged at. Returns numpy arrays (out_lens uint64, needs uint64, statuses int32): the status and
    length ms_decompress would return with *out_len = limit, and the smallest capacity that decodes (0 where the status is not OK)."""
    import torch
    n = len(units)
    with _call(ctx) as (ctx, dev):
        d_in, in_off, lens = _upload_units(units, dev)
        d_len = torch.zeros(max(1, n), dtype=torch.int64, device=dev)
        d_need = torch.zeros(max(1, n), dtype=torch.int64, device=dev)
        d_st = torch.zeros(max(1, n), dtype=torch.int32, device=dev)
        plan = SizePlan(ctx, fmt, in_off, lens, limits)
        plan.execute(d_in, d_len, d_need, d_st)
        ctx.stream.synchronize()
        out = (d_len.cpu().numpy().view(np.uint64)[:n].copy(), d_need.cpu().numpy().view(np.uint64)[:n].copy(), d_st.cpu().numpy()[:n].copy())
        plan.close()
    return out


def decompress_units_auto(fmt, units, limits=None, ctx=None):
    """Decompress a list of compressed buffers whose sizes are not known: sizes them first (decompressed_sizes, at ``limits``), then
    decodes with capacity ``need`` for every unit, outputs back to back. Returns what decompress_units returns; a unit that is not
    MSCOMP_OK at its limit gets None and its status from the size pass."""
    with _call(ctx, enter=False) as (ctx, _):
        _, need, st = decompressed_sizes(fmt, units, limits, ctx=ctx)
        ok = [i for i in range(len(units)) if st[i] == MSCOMP_OK]
        res, status = [None] * len(units), [int(x) for x in st]
        if ok:
            got, gst = decompress_units(fmt, [units[i] for i in ok], [int(need[i]) for i in ok], ctx=ctx)
            for i, g, s in zip(ok, got, gst):
                res[i], status[i] = g, s
    return res, status


def compact_batch(ctx, out_off, out_cap, d_out, d_out_len):
    """mscomp_amd_compact_batch: the outputs of an executed batch packed back to back, in unit order, on the
    device. Returns (d_packed uint8 tensor, d_packed_off int64 tensor of n + 1 offsets); enqueued on the ctx stream."""
    import torch
    out_off = np.ascontiguousarray(out_off, dtype=np.uint64)
    out_cap = np.ascontiguousarray(out_cap, dtype=np.uint64)
    n = len(out_off)
    dev = torch.device("cuda", ctx.device)
    d_packed = torch.empty(int(out_cap.sum()) + 16, dtype=torch.uint8, device=dev)
    d_poff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    _run(ctx, "mscomp_amd_compact_batch", ctx._h, n, d_out, out_off.ctypes.data, out_cap.ctypes.data, d_out_len, d_packed, d_poff)
    return d_packed, d_poff


def decompress_units(fmt, units, capacities, ctx=None):
    """Decompress a list of independent compressed buffers on the GPU (each exactly as one ms_decompress call would, with
    *out_len = capacities[i] on entry). Returns (list of bytes, or None where the status is not MSCOMP_OK; list of status)."""
    return compress_units(fmt, units, ctx=ctx, capacities=capacities, decompress=True)


def compress_units(fmt, units, ctx=None, capacities=None, decompress=False):
    """Compress a list of independent byte strings on the GPU (each exactly as one ms_compress call would).
    ``capacities`` (optional) gives the exact output capacity of every unit (default: ms_max_compressed_size+2).
    Returns (list of compressed bytes, or None where the unit got MSCOMP_BUF_ERROR; list of status)."""
    import torch
    own = ctx is None
    ctx = ctx or Context()
    lens = [len(u) for u in units]
    in_off, in_total = pack_offsets(lens)
    if capacities is None:
        caps = [max_compressed_size(fmt, n) + 2 for n in lens]
        out_off, out_total = pack_offsets(caps)
    else:
        caps = [int(x) for x in capacities]
        out_off, out_total = pack_offsets(caps, align=1)
    blob = np.zeros(in_total + 16, dtype=np.uint8)
    for u, o in zip(units, in_off):
        if len(u):
            blob[int(o): int(o) + len(u)] = np.frombuffer(bytes(u), dtype=np.uint8)
    dev = torch.device("cuda", ctx.device)
    with torch.cuda.device(ctx.device), torch.cuda.stream(ctx.stream):
        d_in = torch.from_numpy(blob).to(dev)
        d_out = torch.zeros(out_total + 16, dtype=torch.uint8, device=dev)
        d_len = torch.zeros(max(1, len(units)), dtype=torch.int64, device=dev)
        d_st = torch.zeros(max(1, len(units)), dtype=torch.int32, device=dev)
        plan = Plan(ctx, fmt, in_off, lens, out_off, caps, decompress=decompress)
        plan.execute(d_in, d_out, d_len, d_st)
        ctx.stream.synchronize()
        h_out, h_len, h_st = d_out.cpu().numpy(), d_len.cpu().numpy(), d_st.cpu().numpy()
        plan.close()
    res = []
    for i in range(len(units)):
        o = int(out_off[i])
        res.append(bytes(h_out[o: o + int(h_len[i])]) if h_st[i] == MSCOMP_OK else None)
    if own:
        ctx.close()
    return res, [int(x) for x in h_st[: len(units)]]




def decompress_units_host(fmt, in_arrays, out_arrays, devices=(0,)):
    """mscomp_amd_decompress_units_host: like compress_units_host for the decoders (capacity of unit i = len(out_arrays[i]))."""
    return compress_units_host(fmt, in_arrays, out_arrays, devices=devices, decompress=True)


class HostViews:
    """n units as views of ONE numpy uint8 array: unit i = base[off[i] : off[i] + length[i]]. The pointer table of a call is then built
    by numpy (base address + offsets) instead of one Python attribute access per unit (milliseconds for thousands of units)."""

    def __init__(self, base, off, length):
        self.base = base
        self.off = np.ascontiguousarray(off, dtype=np.uint64)
        self.length = np.ascontiguousarray(length, dtype=np.uint64)
        assert len(self.off) == len(self.length) and (len(self.off) == 0 or int((self.off + self.length).max()) <= base.size)

    def __len__(self):
        return len(self.off)

    def tables(self):
        return (self.off + np.uint64(self.base.ctypes.data)), self.length


def _host_tables(arrays):
    if isinstance(arrays, HostViews):
        return arrays.tables()
    n = len(arrays)
    return (np.array([a.ctypes.data for a in arrays], dtype=np.uint64) if n else np.zeros(0, np.uint64),
            np.array([a.size for a in arrays], dtype=np.uint64) if n else np.zeros(0, np.uint64))


def compress_units_host(fmt, in_arrays, out_arrays, devices=(0,), decompress=False):
    """mscomp_amd_compress_units_host: units given as numpy uint8 arrays (host memory, any layout) or as HostViews of one array, outputs
    written into the numpy uint8 arrays / HostViews of out_arrays (capacity = their length), on the GPUs `devices` (a range per entry; an
    ordinal may repeat). Returns (status of the call, out_lens uint64 array, statuses int32 array). Nothing is copied on the Python side."""
    lib = load_library()
    n = len(in_arrays)
    assert len(out_arrays) == n
    ip, il = _host_tables(in_arrays)
    op, oc = _host_tables(out_arrays)
    pad = np.zeros(1, np.uint64)
    ip, il, op, oc = [(x if n else pad) for x in (ip, il, op, oc)]
    ol = np.zeros(max(1, n), dtype=np.uint64)
    st = np.full(max(1, n), -9, dtype=np.int32)
    dv = (C.c_int * len(devices))(*[int(d) for d in devices])
    fn = lib.mscomp_amd_decompress_units_host if decompress else lib.mscomp_amd_compress_units_host
    rc = fn(int(fmt), len(devices), dv, n, ip.ctypes.data, il.ctypes.data, op.ctypes.data, oc.ctypes.data, ol.ctypes.data, st.ctypes.data)
    return rc, ol[:n], st[:n]
