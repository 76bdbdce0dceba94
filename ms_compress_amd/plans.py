"""Batches of independent units: the plan classes and the module-level *_dev calls (thin wrappers: tensors go straight through _run; the
timed path of bench.py), their host conveniences (bytes in, one plan run once, bytes out), the host-batch entry (HostViews,
compress_units_host) and the hooks tests read plans and scratch through. Nothing about block containers belongs here."""
import ctypes as C

import numpy as np

from ._abi import MSCOMP_AMD_DEV_LARGE_UNITS, MSCOMP_ERRNO, MSCOMP_OK, MSCompError, ScratchRec, load_library
from ._core import Context, _call, _Handle, _outputs, _run, _three_counts, _upload_unit_tables, _upload_units, max_compressed_size, pack_offsets
from .blocks import BlockContainer, BlockDeduper, BlockReader, BlockSplicer, BlockWriter


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


def crc32_units(units, ctx=None):
    """zlib's crc32 of every byte string of a list, computed on the GPU (CrcDevPlan). Returns a numpy uint32 array."""
    n = len(units)
    with _call(ctx) as f:
        d_in, d_off, d_len, lens = _upload_unit_tables(units, f.dev)
        d_crc, d_st = f.alloc(n, "int32"), f.alloc(n, "int32")
        f.make(CrcDevPlan, n, int(sum(lens))).execute(d_in, d_off, d_len, d_crc, d_st)
        f.sync()
        out, st = f.fetch(d_crc, n), f.fetch(d_st, n, signed=True)
    if st.any():
        raise MSCompError(int(st[st != 0][0]), "mscomp_amd_plan_execute_crc_dev")
    return out


def decompressed_sizes(fmt, units, limits=None, ctx=None):
    """Size a list of independent compressed buffers on the GPU without decoding them. ``limits`` (optional, one per unit; default
    no limit) is the capacity each is judged at. Returns numpy arrays (out_lens uint64, needs uint64, statuses int32): the status and
    length ms_decompress would return with *out_len = limit, and the smallest capacity that decodes (0 where the status is not OK)."""
    n = len(units)
    with _call(ctx) as f:
        d_in, in_off, lens = _upload_units(units, f.dev)
        d_len, d_need, d_st = f.alloc(n), f.alloc(n), f.alloc(n, "int32")
        f.make(SizePlan, fmt, in_off, lens, limits).execute(d_in, d_len, d_need, d_st)
        f.sync()
        return f.fetch(d_len, n), f.fetch(d_need, n), f.fetch(d_st, n, signed=True)


def decompress_units_auto(fmt, units, limits=None, ctx=None):
    """Decompress a list of compressed buffers whose sizes are not known: sizes them first (decompressed_sizes, at ``limits``), then
    decodes with capacity ``need`` for every unit, outputs back to back. Returns what decompress_units returns; a unit that is not
    MSCOMP_OK at its limit gets None and its status from the size pass."""
    with _call(ctx, enter=False) as f:
        _, need, st = decompressed_sizes(fmt, units, limits, ctx=f.ctx)
        ok = [i for i in range(len(units)) if st[i] == MSCOMP_OK]
        res, status = [None] * len(units), [int(x) for x in st]
        if ok:
            got, gst = decompress_units(fmt, [units[i] for i in ok], [int(need[i]) for i in ok], ctx=f.ctx)
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
    n = len(units)
    with _call(ctx) as f:
        d_in, in_off, lens = _upload_units(units, f.dev)
        if capacities is None:
            caps = [max_compressed_size(fmt, x) + 2 for x in lens]
            out_off, out_total = pack_offsets(caps)
        else:
            caps = [int(x) for x in capacities]
            out_off, out_total = pack_offsets(caps, align=1)
        d_out, d_len, d_st = f.alloc(out_total + 16, "uint8"), f.alloc(n), f.alloc(n, "int32")
        f.make(Plan, fmt, in_off, lens, out_off, caps, decompress=decompress).execute(d_in, d_out, d_len, d_st)
        f.sync()
        h_out, h_len, h_st = f.fetch(d_out), f.fetch(d_len, n), f.fetch(d_st, n, signed=True)
    return _outputs(h_out, out_off, h_len, h_st == MSCOMP_OK), [int(x) for x in h_st]


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
