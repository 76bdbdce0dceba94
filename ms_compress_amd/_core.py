"""What every part of the binding stands on: the one-shot host calls, Context and _Handle (an object of the library and the context it lives
in), _run (the one place an export is called with tensors), and what the host conveniences share -- the frame _call yields (device and
stream, object lifetime, result tensors, synchronize, fetch) and the upload helpers. No plan or block object is named here: the wrappers
are plans.py and blocks.py, the conveniences over them plans.py and blocks_host.py."""
import contextlib
import ctypes as C
import weakref

import numpy as np

from ._abi import MSCOMP_OK, MSCompError, load_library


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


def _fetch(t, n=None, signed=False):
    """A device tensor on the host as a numpy array that owns its memory, cut to ``n`` entries (None: all of them). An int64 / int32 tensor
    is viewed as uint64 / uint32 -- torch has no unsigned 64-bit arithmetic, so every table travels as int64 -- unless ``signed``: statuses."""
    a = t.cpu().numpy()
    if not signed and a.dtype in (np.int64, np.int32):
        a = a.view(np.uint64 if a.dtype == np.int64 else np.uint32)
    return a[:n].copy()


class _Frame:
    """What _call yields to a host convenience: ``ctx`` and its torch device ``dev``, and the four steps every convenience takes around its
    one device call."""

    def __init__(self, ctx, stack):
        import torch
        self.ctx, self.dev, self._stack = ctx, torch.device("cuda", ctx.device), stack

    def make(self, factory, *args, **kwargs):
        """``factory(ctx, ...)`` -- a plan or block-object class, or one of its for_* constructors --, closed when the frame is left"""
        obj = factory(self.ctx, *args, **kwargs)
        self._stack.callback(obj.close)
        return obj

    def alloc(self, n, dtype="int64", least=1, fill=0):
        """a device tensor of max(least, n) entries of ``fill``: an empty tensor has a null data_ptr(), which several exports refuse"""
        import torch
        return torch.full((max(least, int(n)),), fill, dtype=getattr(torch, dtype), device=self.dev)

    def sync(self):
        """the one synchronize between the device call and the first fetch"""
        self.ctx.stream.synchronize()

    fetch = staticmethod(_fetch)


@contextlib.contextmanager
def _call(ctx, enter=True):
    """The frame of a host convenience: ``ctx`` or, for None, a Context of its own that is closed on the way out, after every object the
    frame made -- also when the body raises; the context's device and stream are torch's current ones inside (not with ``enter`` False: a
    wrapper whose inner calls enter them). Yields a _Frame."""
    import torch
    with contextlib.ExitStack() as stack:                      # (unwound in reverse: the objects, the stream and device, the context)
        if ctx is None:
            ctx = Context()
            stack.callback(ctx.close)
        if enter:
            stack.enter_context(torch.cuda.device(ctx.device))
            stack.enter_context(torch.cuda.stream(ctx.stream))
        yield _Frame(ctx, stack)


def _outputs(h_out, out_off, h_len, kept):
    """per unit the h_len[i] bytes at out_off[i] of ``h_out`` as bytes, or None where kept[i] is false"""
    return [bytes(h_out[int(o): int(o) + int(n)]) if k else None for o, n, k in zip(out_off, h_len, kept)]


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
    nfirst = None if d_nfirst is None else _fetch(d_nfirst)
    nb = d_noff.numel() - 1 if nfirst is None else int(nfirst[-1])
    noff = _fetch(d_noff, nb + 1)
    return _fetch(d_new, min(int(noff[nb]), room)), nfirst, noff, None if d_ncrc is None else _fetch(d_ncrc, nb)


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
