"""Block containers that stay in device memory from call to call: DeviceBlocks is a container as tensors, BlockOps the calls of blocks.py at
one set of bounds -- it owns the objects, allocates every result with the entry count the header asks for (sizes(), the one table of them)
and hands a call's container to the next one. Nothing here launches a kernel of its own except layout_dev in decompress(), the two torch
fills of read() (arange for the slots, a constant for the capacities) and those of prepare("diff"); nothing synchronises or fetches except
DeviceBlocks.packed_len, .host and .from_host. Covered: compress, decompress + check, read, write, resize, splice, splice_extents, diff, delta, patch.

Left out, to follow in the same shape: dedup, match, sync, digests, parity, salvage / repair and transcode. Until then the handle classes
of blocks.py take ``con.view()`` as a source and the fields of a DeviceBlocks as their tables; transcode changes the shape and needs a
second BlockOps. The blocks_* host conveniences do not run on this layer yet."""
import collections
import contextlib

import numpy as np

from ._abi import MSCOMP_AMD_SPLICE_SRC_MAX
from ._core import _dev_block_crc, _dev_u64, _fetch
from .blocks import BlockContainer, BlockDeduper, BlockReader, BlockSplicer, BlockWriter
from .plans import layout_dev

SLACK = 64                                                     # unstated bytes behind ``cap`` in every packed tensor (_core._new_container's room)
KINDS = ("container", "read", "write", "resize", "splice", "splice_extents", "diff")
BlockDiff = collections.namedtuple("BlockDiff", "delta_ext_first delta_ext patch_ext_first patch_ext changed count status")


def _tables(n_res, n_blocks_max, bounds):
    """The header's parameter names and entry counts, once: per kind what the layer allocates ("makes") and what it is handed ("takes")."""
    n, nb = int(n_res), int(n_blocks_max)
    b = lambda name: int(bounds.get(name, 0))
    room, nq = b("in_total_max") + SLACK, b("n_req")
    slot = (b("cap_each") + 15) // 16 * 16
    new = {"d_new_packed": (room, "uint8"), "d_new_block_first": (n + 1, "int64"), "d_new_block_off": (nb + 1, "int64"),
           "d_new_block_crc": (nb, "int32"), "d_new_res_len": (n, "int64")}
    ext = {"d_ext_first": (n + 1, "int64"), "d_ext": (4 * b("n_ext"), "int64")}
    lists = {"d_delta_ext_first": (n + 1, "int64"), "d_delta_ext": (4 * nb, "int64"), "d_patch_ext_first": (n + 1, "int64"),
             "d_patch_ext": (4 * nb, "int64")}
    return {
        "container": ({"d_packed": (room, "uint8"), "d_block_first": (n + 1, "int64"), "d_block_off": (nb + 1, "int64"), "d_block_crc": (nb, "int32"),
                       "d_status": (n, "int32"), "d_out": (b("in_total_max") + 16 * n, "uint8"), "d_out_off": (n + 1, "int64"),
                       "d_out_len": (n, "int64")},
                      {"d_res_off": (n, "int64"), "d_res_len": (n, "int64"), "d_range": (2 * n, "int64")}, {"in_total_max"}),
        "read": ({"d_out": (nq * slot, "uint8"), "d_out_off": (nq, "int64"), "d_out_cap": (nq, "int64"), "d_out_len": (nq, "int64"),
                  "d_status": (nq, "int32")},
                 {"d_req": (3 * nq, "int64")}, {"n_req", "blocks_max", "cap_each"}),
        "write": ({k: new[k] for k in ("d_new_packed", "d_new_block_off", "d_new_block_crc")}
                  | {"d_written": (nq, "int64"), "d_status": (nq, "int32"), "d_res_status": (n, "int32")},
                  {"d_req": (3 * nq, "int64"), "d_src_off": (nq, "int64")}, {"in_total_max", "n_req", "blocks_max"}),
        "resize": (new | {"d_res_status": (n, "int32")}, {"d_want_len": (n, "int64")}, {"in_total_max", "blocks_max"}),
        "splice": (new | {"d_status": (n, "int32")}, {"d_pick": (2 * n, "int64")}, {"in_total_max", "n_src"}),
        "splice_extents": (new | {"d_status": (n, "int32")}, ext, {"in_total_max", "n_src", "n_ext"}),
        "diff": (lists | {"d_pair": (2 * n, "int64"), "d_changed": (n, "int64"), "d_count": (4, "int64"), "d_status": (n, "int32")},
                 {"d_pair": (2 * n, "int64")}, set()),
    }


def _kind(kind, n_res, n_blocks_max, bounds):
    table = _tables(n_res, n_blocks_max, bounds)
    if kind not in table:
        raise ValueError("no such kind: %r (one of %s)" % (kind, ", ".join(KINDS)))
    if set(bounds) - table[kind][2]:
        raise ValueError("%s takes no bound named %s" % (kind, ", ".join(sorted(set(bounds) - table[kind][2]))))
    return table[kind]


def sizes(kind, n_res, n_blocks_max, **bounds):
    """{header parameter name: (entries, dtype)} of every tensor the layer allocates for the calls of ``kind`` against containers of ``n_res``
    resources and ``n_blocks_max`` table rows. ``bounds``: the kind's own (n_req, n_ext, ...), ``in_total_max`` for the kinds that write
    packed bytes or decoded data (SLACK bytes lie behind it) and, for read, ``cap_each``; one left out counts as 0. A pure function."""
    return dict(_kind(kind, n_res, n_blocks_max, bounds)[0])


def takes(kind, n_res, n_blocks_max, **bounds):
    """sizes() for the tensors a caller hands to the calls of ``kind``: the entries each must have at least."""
    return dict(_kind(kind, n_res, n_blocks_max, bounds)[1])


def _capturing():
    """whether torch's current stream is being captured; a process that never initialised the GPU runtime captures nothing"""
    import torch
    return torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing()


def _torch_device(ctx, _device=None):
    import torch
    return torch.device("cuda", ctx.device) if _device is None else torch.device(_device)


class DeviceBlocks:
    """A block container in device memory: ``packed`` (uint8, ``cap`` bytes of it stated to the library), ``block_first`` (n_res + 1),
    ``block_off`` (n_blocks_table + 1), ``res_len`` (n_res), ``block_crc`` (int32, n_blocks_table, or None) and ``status`` (int32, n_res: the
    per-resource status of the call that made it); tables are int64. A tensor may be shared with the container it was made from or with the
    caller's input (compress keeps d_res_len, write keeps block_first and res_len): they are only ever read."""

    def __init__(self, ctx, fmt, block_size, n_res, n_blocks_table, packed, cap, block_first, block_off, res_len, block_crc, status):
        self.ctx, self.fmt, self.block_size, self.n_res, self.n_blocks_table = ctx, int(fmt), int(block_size), int(n_res), int(n_blocks_table)
        self.packed, self.cap, self.block_first, self.block_off, self.res_len = packed, int(cap), block_first, block_off, res_len
        self.block_crc, self.status = block_crc, status
        if self.cap > packed.numel():
            raise ValueError("cap exceeds packed")
        for name, t, least in (("block_first", block_first, self.n_res + 1), ("block_off", block_off, self.n_blocks_table + 1),
                               ("res_len", res_len, self.n_res), ("block_crc", block_crc, self.n_blocks_table), ("status", status, self.n_res)):
            if t is not None and t.numel() < least:
                raise ValueError("%s has %d entries, the container needs %d" % (name, t.numel(), least))

    def view(self, crc=True):
        """The source the view-taking calls of blocks.py take (BlockSplicer.splice, BlockDeduper.diff, ...), every field of the BlocksView
        stated: packed_len is ``cap``. ``crc`` False leaves the checksums out."""
        return (self.packed, self.block_first, self.block_off, self.res_len, self.block_crc if crc else None, self.cap, self.n_res, self.n_blocks_table)

    def packed_len(self):
        """the exact stored length block_off[block_first[n_res]]; synchronizes the stream"""
        self.ctx.stream.synchronize()
        nb = min(int(_fetch(self.block_first[self.n_res: self.n_res + 1])[0]), self.n_blocks_table)
        return min(int(_fetch(self.block_off[nb: nb + 1])[0]), self.cap)

    def host(self):
        """(packed[:packed_len], block_first, block_off, lengths, block_crc or None) as the blocks_* conveniences take and return a container:
        numpy arrays cut to the resources and blocks there are, the lengths a list; synchronizes the stream"""
        self.ctx.stream.synchronize()
        first = _fetch(self.block_first, self.n_res + 1)
        nb = min(int(first[self.n_res]), self.n_blocks_table)
        off = _fetch(self.block_off, nb + 1)
        return (_fetch(self.packed, min(int(off[nb]), self.cap)), first, off, [int(x) for x in _fetch(self.res_len, self.n_res)],
                None if self.block_crc is None else _fetch(self.block_crc, nb))

    @classmethod
    def from_host(cls, ctx, fmt, block_size, container, n_blocks_table=None, cap=None, _device=None):
        """``container`` = (packed, block_first, block_off, lengths, block_crc or None) uploaded: a table of ``n_blocks_table`` rows (default:
        those of block_off), the rows behind its own repeating the total; ``cap`` stated bytes (default: those of packed) and SLACK more."""
        import torch
        dev = _torch_device(ctx, _device)
        packed, first, off, lens, crc = container
        packed = np.ascontiguousarray(np.frombuffer(bytes(packed), dtype=np.uint8) if not isinstance(packed, np.ndarray) else packed, dtype=np.uint8)
        n, rows = len(lens), max(0, len(np.asarray(off).reshape(-1)) - 1)
        nbt = rows if n_blocks_table is None else int(n_blocks_table)
        cap = len(packed) if cap is None else int(cap)
        if nbt < rows or cap < len(packed):
            raise ValueError("the container has %d rows and %d stored bytes" % (rows, len(packed)))
        d_packed = torch.zeros(cap + SLACK, dtype=torch.uint8, device=dev)
        if len(packed):
            d_packed[: len(packed)] = torch.from_numpy(packed.copy()).to(dev)
        return cls(ctx, fmt, block_size, n, nbt, d_packed, cap, _dev_u64(first, n + 1, dev), _dev_u64(off, nbt + 1, dev),
                   _dev_u64([int(x) for x in lens], 1, dev), None if crc is None else _dev_block_crc(crc, nbt, dev),
                   torch.zeros(max(1, n), dtype=torch.int32, device=dev))


class BlockOps:
    """The block calls at one set of bounds. Every container it makes or takes has ``n_res`` resources, a table of
    n_blocks_max = n_res + in_total_max // block_size rows (mscomp_amd_blocks_bound) and ``cap`` = in_total_max stated bytes -- a stored block
    is never longer than its data, so that capacity refuses no write whose data fits the bounds --, so containers of one BlockOps compose; one of
    another shape raises ValueError before anything is enqueued. ``crc``: whether compress writes checksums; every other call carries them
    exactly when its sources have them.

    The objects of blocks.py are made once: prepare(kind, **bounds) makes and keeps the one a kind needs, and a method whose kind was not
    prepared prepares it with the widest bounds the shape allows. Making one allocates device memory, which is illegal while the stream
    is being captured: a method that would have to then raises RuntimeError naming the kind, before anything is enqueued.

    Every method enqueues on the ctx stream and returns at once; results are fresh tensors, allocated on that stream, whose entries behind
    what the call writes are unspecified. Per-unit errors stay in the status tensors; only a call-level status raises MSCompError."""

    def __init__(self, ctx, fmt, block_size, n_res, in_total_max, crc=True, _device=None):
        self.ctx, self.fmt, self.block_size, self.n_res, self.in_total_max = ctx, int(fmt), int(block_size), int(n_res), int(in_total_max)
        self.crc = bool(crc)
        self.n_blocks_max = self.n_res + self.in_total_max // self.block_size
        self._dev = _torch_device(ctx, _device)
        self._made = {}                                           # (kind, the bounds a call must meet exactly) -> the object
        self._pairs = None                                        # the pairs (r, r) of diff

    # ---- the objects --------------------------------------------------------------------------------------------------------------------
    def prepare(self, kind, **bounds):
        """Makes the object of ``kind`` and keeps it; bounds left out are the widest the shape allows. "container": none. "read" / "write":
        ``n_req`` (no default: one object per request count), ``blocks_max`` (n_blocks_max). "resize": ``blocks_max`` (n_blocks_max) -- it
        runs on a prepared writer whose blocks_max is no smaller. "splice": ``n_src`` (1). "splice_extents": ``n_src`` (without it 1 and 2,
        what delta and patch take), ``n_ext`` (n_blocks_max: what a diff's lists hold) -- one object per pair of them. "diff": none.
        Preparing a kind again with bounds its object does not meet replaces the object."""
        _kind(kind, self.n_res, self.n_blocks_max, bounds)
        nbm, B, ctx = self.n_blocks_max, self.block_size, self.ctx
        bmax = int(bounds.get("blocks_max", nbm))
        if kind == "container":
            self._keep(("container",), lambda o: True, lambda: BlockContainer(ctx, self.fmt, B, self.n_res, self.in_total_max))
        elif kind in ("read", "write"):
            if "n_req" not in bounds:
                raise ValueError("prepare(%r, n_req=...): a %s is made for one request count" % (kind, "reader" if kind == "read" else "writer"))
            cls = BlockReader if kind == "read" else BlockWriter
            obj = self._keep((kind, int(bounds["n_req"])), lambda o: o.blocks_max >= bmax,
                             lambda: cls(ctx, self.fmt, B, self.n_res, nbm, int(bounds["n_req"]), bmax))
            old = self._made.get(("resize",))
            if kind == "write" and old is not None and old is not obj and old.n_req == 0 and obj.blocks_max >= old.blocks_max:
                self._made[("resize",)] = obj                   # (resize moves onto the writer; its own goes)
                old.close()
        elif kind == "resize":
            fits = [o for k, o in self._made.items() if k[0] == "write" and o.blocks_max >= bmax]
            self._keep(("resize",), lambda o: o.blocks_max >= bmax, lambda: fits[0] if fits else BlockWriter(ctx, self.fmt, B, self.n_res, nbm, 0, bmax))
        elif kind == "splice":
            n_src = int(bounds.get("n_src", 1))
            self._keep(("splice", n_src), lambda o: True, lambda: BlockSplicer(ctx, B, n_src, self.n_res, nbm))
        elif kind == "splice_extents":
            n_ext = int(bounds.get("n_ext", nbm))
            for n_src in ([int(bounds["n_src"])] if "n_src" in bounds else [1, 2]):
                self._keep(("splice_extents", n_src, n_ext), lambda o: True, lambda: BlockSplicer.for_extents(ctx, B, n_src, self.n_res, n_ext, nbm))
        else:
            self._keep(("diff",), lambda o: True, lambda: BlockDeduper.for_diff(ctx, B, self.n_res, nbm))
            if self._pairs is None:
                import torch
                with self._stream():
                    self._pairs = self._alloc("d_pair", sizes("diff", self.n_res, nbm)["d_pair"][0], "int64")
                    if self.n_res:
                        torch.arange(2 * self.n_res, dtype=torch.int64, device=self._dev, out=self._pairs).bitwise_right_shift_(1)

    def _keep(self, key, fits, make):
        """the object kept under ``key`` when it ``fits``; otherwise ``make()`` in its place -- never while the stream is being captured"""
        obj = self._made.get(key)
        if obj is not None and fits(obj):
            return obj
        if _capturing():
            raise RuntimeError("BlockOps: making the %s object allocates, which a capturing stream forbids: prepare(%r, ...) before the capture"
                               % (key[0], key[0]))
        new = make()
        if obj is not None and obj is not new and not any(o is obj for k, o in self._made.items() if k != key):
            obj.close()
        self._made[key] = new
        return new

    def _have(self, kind, key, **bounds):
        """the prepared object under ``key``, prepared now with ``bounds`` when there is none"""
        if key not in self._made:
            self.prepare(kind, **bounds)
        return self._made[key]

    def close(self):
        """closes every object made here (a closed context has closed them already: closing twice is harmless)"""
        for obj in self._made.values():
            obj.close()
        self._made, self._pairs = {}, None

    @contextlib.contextmanager
    def graph(self, *kinds):
        """Prepares ``kinds`` -- those not prepared yet, with their default bounds; read and write need their n_req, so prepare them first --,
        then captures the context's stream: ``with ops.graph("container", "resize") as g: ...; g.replay()``. Every method is legal inside;
        packed_len, host and from_host are not. The context must sit on a stream of its own: the default stream cannot be captured."""
        import torch
        if self.ctx.stream == torch.cuda.default_stream(self.ctx.device):
            raise ValueError("BlockOps.graph: the context sits on the default stream, which cannot be captured")
        for kind in kinds:
            _kind(kind, self.n_res, self.n_blocks_max, {})
            if not any(k[0] == kind for k in self._made):
                self.prepare(kind)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=self.ctx.stream):
            yield g

    # ---- tensors ------------------------------------------------------------------------------------------------------------------------
    def _alloc(self, name, entries, dtype, fill=0):
        """The one place a tensor is made: ``entries`` of ``dtype`` for the header's parameter ``name``, one at least -- an empty tensor has
        a null data_ptr(), which several exports refuse --, holding ``fill``; None leaves them unwritten (the call writes them: no launch)."""
        import torch
        n = max(1, int(entries))
        if fill is None:
            return torch.empty(n, dtype=getattr(torch, dtype), device=self._dev)
        return torch.full((n,), fill, dtype=getattr(torch, dtype), device=self._dev)

    def _outputs(self, kind, names, **bounds):
        """the named tensors of sizes(kind), unwritten; a None for every name ``names`` maps to False"""
        table = sizes(kind, self.n_res, self.n_blocks_max, **bounds)
        return [self._alloc(name, *table[name], fill=None) if want else None for name, want in names.items()]

    def _stream(self):
        """torch's current device and stream are the context's inside: allocations are ordered with the library's kernels"""
        import torch
        if self._dev.type != "cuda":
            return contextlib.nullcontext()
        stack = contextlib.ExitStack()
        stack.enter_context(torch.cuda.device(self.ctx.device))
        stack.enter_context(torch.cuda.stream(self.ctx.stream))
        return stack

    def _check(self, kind, bounds=None, **tensors):
        """ValueError for a handed tensor with fewer entries than takes(kind) asks of its name, or of another width"""
        table = takes(kind, self.n_res, self.n_blocks_max, **(bounds or {}))
        for name, t in tensors.items():
            entries, dtype = table[name]
            if t is not None and (t.numel() < entries or t.element_size() != np.dtype(dtype).itemsize):
                raise ValueError("%s: %d entries of %d bytes, %s needs %d of %s" % (name, t.numel(), t.element_size(), kind, entries, dtype))

    def _own(self, *cons):
        """ValueError for a container of another context, format or shape"""
        for c in cons:
            if (c.ctx is not self.ctx or (c.fmt, c.block_size, c.n_res, c.n_blocks_table) != (self.fmt, self.block_size, self.n_res, self.n_blocks_max)
                    or c.cap > self.in_total_max):
                raise ValueError("a container of another shape: (fmt, block_size, n_res, n_blocks_table, cap) = %r, this BlockOps has %r"
                                 % ((c.fmt, c.block_size, c.n_res, c.n_blocks_table, c.cap),
                                    (self.fmt, self.block_size, self.n_res, self.n_blocks_max, self.in_total_max)))

    def _container(self, packed, first, off, lens, crc, status):
        return DeviceBlocks(self.ctx, self.fmt, self.block_size, self.n_res, self.n_blocks_max, packed, self.in_total_max, first, off, lens, crc, status)

    # ---- the calls ----------------------------------------------------------------------------------------------------------------------
    def compress(self, d_data, d_res_off, d_res_len):
        """BlockContainer.compress, and .crc with ``crc``: resource r = d_res_len[r] bytes at d_data + d_res_off[r]. The container keeps
        d_res_len itself as its res_len; its status is compress's."""
        self._check("container", d_res_off=d_res_off, d_res_len=d_res_len)
        bk = self._have("container", ("container",))
        with self._stream():
            d_packed, d_first, d_off, d_crc, d_st = self._outputs("container", {"d_packed": 1, "d_block_first": 1, "d_block_off": 1, "d_block_crc": self.crc,
                                                                                "d_status": 1}, in_total_max=self.in_total_max)
            if self.crc:                                        # (first: both write d_status, and compress's is the one kept)
                bk.crc(d_data, d_res_off, d_res_len, d_crc, d_st)
            bk.compress(d_data, d_res_off, d_res_len, d_packed, d_first, d_off, d_st, packed_cap=self.in_total_max)
        return self._container(d_packed, d_first, d_off, d_res_len, d_crc, d_st)

    def decompress(self, con, d_range=None, check=True):
        """BlockContainer.decompress -- and .check with ``check`` and a block_crc -- of ``con``, or of the blocks ``d_range`` (2 n_res: first
        block, count) names: (d_out, d_out_off, d_out_len, d_status). Resource r lies at d_out + d_out_off[r], the offsets being
        layout_dev's over res_len at align 16 (n_res + 1 entries); its capacity is its length."""
        self._own(con)
        self._check("container", d_range=d_range)
        bk = self._have("container", ("container",))
        with self._stream():
            d_out, d_ooff, d_olen, d_st = self._outputs("container", {"d_out": 1, "d_out_off": 1, "d_out_len": 1, "d_status": 1}, in_total_max=self.in_total_max)
            layout_dev(self.ctx, con.res_len[: self.n_res], align=16, d_off=d_ooff)
            bk.decompress(con.packed, con.block_first, con.block_off, con.res_len, d_out, d_ooff, con.res_len, d_olen, d_st, d_range=d_range,
                          packed_len=con.cap)
            if check and con.block_crc is not None:
                bk.check(d_out, d_ooff, con.res_len, con.block_first, con.block_crc, d_olen, d_st, d_range=d_range)
        return d_out, d_ooff, d_olen, d_st

    def read(self, con, d_req, cap_each):
        """BlockReader.read of the requests ``d_req`` (3 per request: resource, offset, length; no arithmetic is done on them):
        (d_out, d_out_off, d_out_len, d_status). Request q gets the slot at q * (cap_each rounded up to 16) and the capacity cap_each, whether
        or not the library will serve it. Every block read is held to the container's checksums when it has them."""
        import torch
        self._own(con)
        nq, cap_each = d_req.numel() // 3, int(cap_each)
        bounds = {"n_req": nq, "cap_each": cap_each}
        self._check("read", bounds, d_req=d_req)
        rd = self._have("read", ("read", nq), n_req=nq)
        with self._stream():
            d_out, d_olen, d_st = self._outputs("read", {"d_out": 1, "d_out_len": 1, "d_status": 1}, **bounds)
            table = sizes("read", self.n_res, self.n_blocks_max, **bounds)
            d_ocap, d_ooff = self._alloc("d_out_cap", *table["d_out_cap"], fill=cap_each), self._alloc("d_out_off", *table["d_out_off"], fill=None)
            slot = table["d_out"][0] // max(1, nq)
            if nq and slot:
                torch.arange(0, nq * slot, slot, dtype=torch.int64, device=self._dev, out=d_ooff)
            else:
                d_ooff.zero_()
            rd.read(con.packed, con.block_first, con.block_off, con.res_len, d_req, d_out, d_ooff, d_ocap, d_olen, d_st, d_block_crc=con.block_crc,
                    packed_len=con.cap)
        return d_out, d_ooff, d_olen, d_st

    def write(self, con, d_req, d_src, d_src_off):
        """BlockWriter.write of the requests ``d_req`` (3 per request), request q's bytes at d_src + d_src_off[q]:
        (container, d_written, d_status). The new container shares block_first and res_len with ``con``; its status is d_res_status."""
        self._own(con)
        nq = d_req.numel() // 3
        self._check("write", {"n_req": nq}, d_req=d_req, d_src_off=d_src_off)
        wr = self._have("write", ("write", nq), n_req=nq)
        with_crc = con.block_crc is not None
        with self._stream():
            d_new, d_noff, d_ncrc, d_wr, d_st, d_rst = self._outputs(
                "write", {"d_new_packed": 1, "d_new_block_off": 1, "d_new_block_crc": with_crc, "d_written": 1, "d_status": 1, "d_res_status": 1},
                in_total_max=self.in_total_max, n_req=nq)
            wr.write(con.packed, con.block_first, con.block_off, con.res_len, d_req, d_src, d_src_off, d_new, d_noff, d_wr, d_st, d_rst,
                     d_block_crc=con.block_crc, d_new_block_crc=d_ncrc, packed_len=con.cap, new_cap=self.in_total_max)
        return self._container(d_new, con.block_first, d_noff, con.res_len, d_ncrc, d_rst), d_wr, d_st

    def resize(self, con, d_want_len):
        """BlockWriter.resize: every resource cut or zero-extended to d_want_len[r]. The new container's status is d_res_status; lengths
        that sum to more than in_total_max are answered by the library's own statuses (MSCOMP_BUF_ERROR, or a refused table)."""
        self._own(con)
        self._check("resize", d_want_len=d_want_len)
        wr = self._have("resize", ("resize",))
        with_crc = con.block_crc is not None
        with self._stream():
            d_new, d_nfirst, d_noff, d_ncrc, d_nlen, d_rst = self._outputs(
                "resize", {"d_new_packed": 1, "d_new_block_first": 1, "d_new_block_off": 1, "d_new_block_crc": with_crc, "d_new_res_len": 1,
                           "d_res_status": 1}, in_total_max=self.in_total_max)
            wr.resize(con.packed, con.block_first, con.block_off, con.res_len, d_want_len, d_new, d_nfirst, d_noff, d_nlen, d_rst,
                      d_block_crc=con.block_crc, d_new_block_crc=d_ncrc, packed_len=con.cap, new_cap=self.in_total_max)
        return self._container(d_new, d_nfirst, d_noff, d_nlen, d_ncrc, d_rst)

    def _spliced(self, kind, sources, run, **bounds):
        """what splice and splice_extents share: the new container's tensors made, ``run(d_new, ...)`` called, the container"""
        with_crc = all(c.block_crc is not None for c in sources)
        with self._stream():
            d_new, d_nfirst, d_noff, d_ncrc, d_nlen, d_st = self._outputs(
                kind, {"d_new_packed": 1, "d_new_block_first": 1, "d_new_block_off": 1, "d_new_block_crc": with_crc, "d_new_res_len": 1, "d_status": 1},
                in_total_max=self.in_total_max, **bounds)
            run([c.view(with_crc) for c in sources], d_new, d_nfirst, d_noff, d_nlen, d_st, d_ncrc)
        return self._container(d_new, d_nfirst, d_noff, d_nlen, d_ncrc, d_st)

    def splice(self, sources, d_pick):
        """BlockSplicer.splice over the containers ``sources`` (1 .. 4): pick p = (d_pick[2 p], d_pick[2 p + 1]) = (source, resource) becomes
        resource p, n_res picks. Checksums are carried when every source has them."""
        sources = list(sources)
        self._own(*sources)
        if not 1 <= len(sources) <= MSCOMP_AMD_SPLICE_SRC_MAX:
            raise ValueError("1 .. %d sources" % MSCOMP_AMD_SPLICE_SRC_MAX)
        self._check("splice", d_pick=d_pick)
        sp = self._have("splice", ("splice", len(sources)), n_src=len(sources))
        return self._spliced("splice", sources, lambda views, d_new, d_nfirst, d_noff, d_nlen, d_st, d_ncrc: sp.splice(
            views, d_pick, d_new, d_nfirst, d_noff, d_nlen, d_st, d_new_block_crc=d_ncrc, new_cap=self.in_total_max), n_src=len(sources))

    def splice_extents(self, sources, d_ext_first, d_ext):
        """BlockSplicer.splice_extents over the containers ``sources`` (1 .. 4): new resource q is the extents d_ext_first[q] ..
        d_ext_first[q + 1] - 1 of ``d_ext`` (4 per extent: source, resource, first block, count). n_ext is what d_ext holds: there is one
        splicer per (n_src, n_ext), so the library never reads behind d_ext whatever d_ext_first says."""
        sources = list(sources)
        self._own(*sources)
        if not 1 <= len(sources) <= MSCOMP_AMD_SPLICE_SRC_MAX:
            raise ValueError("1 .. %d sources" % MSCOMP_AMD_SPLICE_SRC_MAX)
        bounds = {"n_src": len(sources), "n_ext": d_ext.numel() // 4}
        self._check("splice_extents", bounds, d_ext_first=d_ext_first, d_ext=d_ext)
        sp = self._have("splice_extents", ("splice_extents",) + tuple(bounds.values()), **bounds)
        return self._spliced("splice_extents", sources, lambda views, d_new, d_nfirst, d_noff, d_nlen, d_st, d_ncrc: sp.splice_extents(
            views, d_ext_first, d_ext, d_new, d_nfirst, d_noff, d_nlen, d_st, d_new_block_crc=d_ncrc, new_cap=self.in_total_max), **bounds)

    def diff(self, base, new, d_pair=None):
        """BlockDeduper.diff of ``new`` against ``base``: a BlockDiff. Pair p = (d_pair[2 p], d_pair[2 p + 1]) = (base resource or
        MSCOMP_AMD_DIFF_NO_BASE, new resource), n_res pairs; None: the pairs (r, r). Checksums take part when both containers have them."""
        self._own(base, new)
        self._check("diff", d_pair=d_pair)
        dd = self._have("diff", ("diff",))
        with_crc = base.block_crc is not None and new.block_crc is not None
        with self._stream():
            outs = self._outputs("diff", {"d_delta_ext_first": 1, "d_delta_ext": 1, "d_patch_ext_first": 1, "d_patch_ext": 1, "d_changed": 1, "d_count": 1,
                                          "d_status": 1})
            dd.diff(base.view(with_crc), new.view(with_crc), self._pairs if d_pair is None else d_pair, *outs)
        return BlockDiff(*outs)

    def delta(self, base, new, d_pair=None):
        """(the delta container, the BlockDiff): diff, then splice_extents over [new] with the delta lists -- per pair the changed blocks of
        the new resource, in order -- as blocks_delta does."""
        df = self.diff(base, new, d_pair)
        with_crc = base.block_crc is not None and new.block_crc is not None
        src = new if with_crc or new.block_crc is None else self._container(new.packed, new.block_first, new.block_off, new.res_len, None, new.status)
        return self.splice_extents([src], df.delta_ext_first, df.delta_ext), df

    def patch(self, base, delta, diff):
        """the new resources again: splice_extents over [base, delta] with the patch lists of ``diff``"""
        return self.splice_extents([base, delta], diff.patch_ext_first, diff.patch_ext)
