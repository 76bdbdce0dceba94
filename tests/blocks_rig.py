"""What the GPU tests of the block family (containers, readers, writers, splicers, dedupers, transcoders) share: the constants, the small
upload helpers and data builders, a block container on host and device (Container), the sentinel-filled arrays a call writes a new
container into (NewContainer) or lists into (ListOuts), the one image comparison (same_image), and the rigs that more than one file
drives (BlockRig / CrcRig: one BlockContainer in place; Splices / Extents: splice calls over two containers). The comparisons run on
host arrays (NewContainer.compare, ListOuts.compare), so tests/test_blocks_rig.py pins them without a device. torch is imported inside
the functions that need it. Not collected as a test."""
import copy

import numpy as np

import blocks_model as M
import crc_model as K
import dedup_model as D
import extents_model as X
import read_model as R
import resize_model as Z
import splice_model as S
import write_model as W
from resize_model import SPARE
from splice_model import ORDER2

FMTS = {"lznt1": 2, "xpress": 3, "xpress_huff": 4}
BLOCKS = (4096, 65536)
ALL = M.M64
FILL, CRC_FILL, ST_FILL = 0xA5, 0x55555555, 77                  # what output bytes, checksum words and statuses hold before a call
SENT, SENT32 = 0x7777777777777777, 77                           # what the list outputs of ListOuts hold before a call
POISONS = (0x00, 0xFF, 0xA5)
BYTE_GUARD, CAP_GUARD, ENTRY_GUARD = 48, 64, 5                  # watched bytes around a request's range and behind a capacity; entries behind a list
MIXED, TEXT, ZEROS5, MIXED5, RANDOM1 = 5, 7, 6, 9, 3            # rows of R.RECIPES: 3 B + 17 mixed / text, 5 B zeros / mixed, one raw block


# ---- uploads ----------------------------------------------------------------------------------------------------------------------------
def d64(a, dev, least=1):
    """``a`` as an int64 device tensor of at least ``least`` entries, zeros behind its own (an empty ``a``: ``least`` zeros)"""
    import torch
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
    h = np.zeros(max(least, len(a)), dtype=np.uint64)
    h[: len(a)] = a
    return torch.from_numpy(h.view(np.int64)).to(dev)


def d8(b, dev):
    """bytes as a uint8 device tensor with 16 zero bytes behind them"""
    import torch
    h = np.zeros(len(b) + 16, dtype=np.uint8)
    h[: len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
    return torch.from_numpy(h).to(dev)


def i32(a, dev):
    """32-bit words (checksums) as an int32 device tensor"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).to(dev)


def u32(t, n):
    """the first n entries of an int32 device tensor, as uint32 on the host"""
    return t.cpu().numpy().view(np.uint32)[:n]


# ---- data -------------------------------------------------------------------------------------------------------------------------------
def rand(seed, n):
    return np.random.RandomState(seed).bytes(n)


def soft(seed, n):
    """n bytes that every format compresses"""
    return bytes(np.random.RandomState(seed).randint(0, 8, n).astype(np.uint8))


def text(seed, n):
    return M._text(np.random.RandomState(seed), n)


def mixed(seed, n, B=4096, period=2):
    """blocks of B bytes by turns random and text (every period-th one random)"""
    rs = np.random.RandomState(seed)
    return b"".join(rs.bytes(min(B, n - at)) if (at // B) % period == 0 else M._text(rs, min(B, n - at)) for at in range(0, n, B))


def flipped(buf, *at):
    out = bytearray(buf)
    for a in at:
        out[a] ^= 0xFF
    return bytes(out)


def recipe(kind, seed, mult, add, B):
    return M.build({"kind": kind, "seed": seed, "mult": mult, "add": add}, B)


# ---- comparisons on the host --------------------------------------------------------------------------------------------------------------
def same_image(got, model_bytes, fill, what):
    """``got`` (a whole output buffer, numpy uint8) is ``model_bytes`` laid over a buffer of ``fill``: fails with the first differing byte"""
    image = np.full(len(got), fill, dtype=np.uint8)
    for at, b in ([(0, model_bytes)] if isinstance(model_bytes, (bytes, bytearray, np.ndarray)) else model_bytes):
        image[at: at + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
    bad = np.nonzero(np.asarray(got) != image)[0]
    assert bad.size == 0, (what, "differs from the model at byte", int(bad[0]))


def memo(make=None):
    """For a module-scoped fixture (``yield from memo(...)``): get(*key) makes a thing once per key -- with ``make(*key)``, or without one
    with the maker that follows the key --, and whatever has a close() is closed at the module's end."""
    made = {}

    def get(*key):
        if make is None:
            *key, maker = key
            key = tuple(key)
        if key not in made:
            made[key] = make(*key) if make else maker()
        return made[key]
    yield get
    for v in made.values():
        if hasattr(v, "close"):
            v.close()


def odd_offsets(bufs, room):
    """(offsets, input buffer of ``room`` bytes): the sources at position 1 and 3 bytes apart, 0x5A between them -- every source alignment"""
    off, pos = [], 1
    for b in bufs:
        off.append(pos)
        pos += len(b) + 3
    blob = np.full(room, 0x5A, dtype=np.uint8)
    for b, o in zip(bufs, off):
        blob[o: o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return off, blob


def fresh(ctx, bk, bufs):
    """BlockContainer.compress + .crc of ``bufs`` (one resource each, back to back) through ``bk``, in tensors of their own; returns
    (packed bytes, first, off of n_blocks_max + 1, crc of n_blocks_max) on the host"""
    import torch
    dev = torch.device("cuda", ctx.device)
    n, room, nbm = bk.n_res, bk.in_total_max, bk.n_blocks_max
    lens = [len(b) for b in bufs]
    assert len(bufs) == n and sum(lens) <= room
    blob = np.frombuffer(b"".join(bufs), dtype=np.uint8)
    d_in = torch.zeros(room + 64, dtype=torch.uint8, device=dev)
    if len(blob):
        d_in[: len(blob)] = torch.from_numpy(blob.copy()).to(dev)
    d_off, d_len = d64(np.cumsum([0] + lens[:-1]), dev), d64(lens, dev)
    d_packed = torch.zeros(room + 64, dtype=torch.uint8, device=dev)
    d_first, d_boff = d64([], dev, n + 1), d64([], dev, nbm + 1)
    d_st, d_crc = torch.zeros(max(1, n), dtype=torch.int32, device=dev), torch.zeros(max(1, nbm), dtype=torch.int32, device=dev)
    bk.compress(d_in, d_off, d_len, d_packed, d_first, d_boff, d_st, packed_cap=room)
    bk.crc(d_in, d_off, d_len, d_crc, d_st)
    ctx.stream.synchronize()
    assert not d_st.cpu().numpy().any()
    off = d_boff.cpu().numpy().view(np.uint64)
    return bytes(d_packed.cpu().numpy()[: int(off[-1])]), d_first.cpu().numpy().view(np.uint64), off, u32(d_crc, nbm)


# ---- a container --------------------------------------------------------------------------------------------------------------------------
class Container:
    """A block container, on the host as the models read it (packed bytes, first, off, lens, crc; n resources, nbt table rows, plen stored
    bytes) and on the device as a view takes it (d_packed, d_first, d_boff, d_len, d_crc). ``cap`` is the packed length a view states,
    ``with_crc`` whether it brings its checksums; edited() gives copies that state something else, far() one whose stored bytes lie
    at ``base`` of a large arena."""
    base = 0

    @classmethod
    def make(cls, ctx, fmt, B, bufs):
        """``bufs`` compressed and checksummed on the GPU by a BlockContainer that the container keeps (bk): the tables have its
        n_blocks_max + 1 entries. Statuses and checksums are asserted."""
        import torch
        import ms_compress_amd as m
        self = cls.__new__(cls)
        self.m, self.ctx, self.fmt, self.B, self.with_crc = m, ctx, fmt, B, True
        self.dev = dev = torch.device("cuda", ctx.device)
        self.n, self.lens = len(bufs), [len(b) for b in bufs]
        self.total = total = sum(self.lens)
        self.bk = m.BlockContainer(ctx, fmt, B, self.n, total)
        self.nbt = self.bk.n_blocks_max
        self.d_in = torch.zeros(total + 3 * self.n + 64, dtype=torch.uint8, device=dev)
        self.d_off, self.d_len = d64([], dev, self.n), d64(self.lens, dev)
        self.d_packed = torch.zeros(total + 64, dtype=torch.uint8, device=dev)
        self.d_first, self.d_boff = d64([], dev, self.n + 1), d64([], dev, self.nbt + 1)
        self.d_cst = torch.zeros(max(1, self.n), dtype=torch.int32, device=dev)
        self.d_crc = torch.zeros(max(1, self.nbt), dtype=torch.int32, device=dev)
        self.load(bufs)
        self.compress()
        ctx.stream.synchronize()
        self.pull()
        return self

    def load(self, bufs):
        """the sources at odd offsets (position 1, 3 bytes apart, 0x5A between them): every source alignment"""
        import torch
        self.bufs, self.lens = bufs, [len(b) for b in bufs]
        off, blob = odd_offsets(bufs, self.d_in.numel())
        self.d_in.copy_(torch.from_numpy(blob))
        self.d_off.copy_(d64(off, self.dev, self.n)); self.d_len.copy_(d64(self.lens, self.dev, self.n))

    def compress(self):
        self.bk.compress(self.d_in, self.d_off, self.d_len, self.d_packed, self.d_first, self.d_boff, self.d_cst, packed_cap=self.total)
        self.bk.crc(self.d_in, self.d_off, self.d_len, self.d_crc, self.d_cst)

    def pull(self):
        """the container as the host sees it: what the model reads"""
        self.first = self.d_first.cpu().numpy().view(np.uint64).copy()
        self.off = self.d_boff.cpu().numpy().view(np.uint64).copy()
        self.plen = self.cap = int(self.off[int(self.first[-1])])
        self.packed = bytes(self.d_packed.cpu().numpy()[: self.plen])
        self.crc = u32(self.d_crc, self.nbt).copy()
        assert not self.d_cst.cpu().numpy().any()
        assert (self.crc == R.block_crcs(self.bufs, self.B, self.nbt)).all()

    @classmethod
    def from_host(cls, ctx, fmt, B, packed, first, off, lens, crc, cap=None):
        """a container from host arrays (as blocks_compress and blocks_crc return them), uploaded with ``cap`` + 64 bytes of room"""
        import torch
        import ms_compress_amd as m
        self = cls.__new__(cls)
        self.m, self.ctx, self.fmt, self.B, self.with_crc, self.bk, self.bufs = m, ctx, fmt, B, True, None, None
        self.dev = dev = torch.device("cuda", ctx.device)
        self.packed = bytes(packed)
        self.first, self.off = np.array(first, dtype=np.uint64), np.array(off, dtype=np.uint64)
        self.lens, self.n, self.nbt = [int(x) for x in lens], len(lens), len(self.off) - 1
        self.total, self.plen = sum(self.lens), len(self.packed)
        self.cap = self.plen if cap is None else cap
        self.d_packed = torch.zeros(self.cap + 64, dtype=torch.uint8, device=dev)
        self.d_packed[: self.plen] = torch.from_numpy(np.frombuffer(self.packed, dtype=np.uint8).copy()).to(dev)
        self.d_first, self.d_boff, self.d_len = d64(self.first, dev), d64(self.off, dev), d64(self.lens, dev)
        self._set_crc(crc)
        return self

    @classmethod
    def via_host(cls, ctx, fmt, B, bufs):
        """from_host of what the host conveniences blocks_compress and blocks_crc make of ``bufs``"""
        import ms_compress_amd as m
        packed, first, off, st = m.blocks_compress(fmt, bufs, B, ctx=ctx)
        crc, _ = m.blocks_crc(fmt, bufs, B, ctx=ctx)
        assert not st.any() and (crc == R.block_crcs(bufs, B, len(crc))).all()
        return cls.from_host(ctx, fmt, B, packed, first, off, [len(b) for b in bufs], crc)

    def _set_crc(self, crc):
        self.crc = np.zeros(self.nbt, dtype=np.uint32)
        self.crc[: len(crc)] = np.asarray(crc, dtype=np.uint32)[: self.nbt]
        self.d_crc = i32(np.concatenate([self.crc, np.zeros(1, dtype=np.uint32)]), self.dev)

    def edited(self, packed=None, first=None, off=None, lens=None, crc=None, nbt=None, plen=None, with_crc=None):
        """a copy with some of its tables or its stored bytes (of the same length) edited on the host and uploaded again, or one that
        states other table rows (nbt), another packed length (plen) or no checksums (with_crc); what is not named is shared"""
        import torch
        c = copy.copy(self)
        c.bk = None
        if packed is not None:
            assert len(packed) == self.plen
            c.packed, c.d_packed = bytes(packed), self.d_packed.clone()
            c.d_packed[: c.plen] = torch.from_numpy(np.frombuffer(c.packed, dtype=np.uint8).copy()).to(self.dev)
        if first is not None:
            c.first, c.d_first = np.array(first, dtype=np.uint64), d64(first, self.dev)
        if off is not None:
            c.off, c.d_boff = np.array(off, dtype=np.uint64), d64(off, self.dev)
        if lens is not None:
            c.lens, c.n, c.d_len = [int(x) for x in lens], len(lens), d64(lens, self.dev)
        if crc is not None:
            c._set_crc(crc)
        c.nbt = self.nbt if nbt is None else nbt
        c.cap = self.cap if plen is None else plen
        c.with_crc = self.with_crc if with_crc is None else with_crc
        return c

    def far(self, arena, base):
        """a copy whose stored bytes lie at byte ``base`` of ``arena`` (a far_rig arena; the caller writes them there): d_packed is the
        arena, every entry of off is shifted by base -- off[0] = base is what the header's rules admit --, plen = cap = base + the stored
        length, and ``packed``, which the models read and model() hands them, is a FarBytes. Everything else is shared."""
        from far_rig import FarBytes
        assert not self.base
        c = copy.copy(self)
        c.bk, c.base = None, int(base)
        c.off = self.off + np.uint64(base)
        c.d_packed, c.d_boff = arena.t, d64(c.off, self.dev)
        c.plen = c.cap = base + self.plen
        c.packed = FarBytes(base, self.packed)
        return c

    def view(self, crc=None, nbt=None, plen=None):
        """the source tuple a splicer or deduper takes, every field stated; crc / nbt / plen default to what the container states"""
        crc = self.with_crc if crc is None else crc
        return (self.d_packed, self.d_first, self.d_boff, self.d_len, self.d_crc if crc else None, self.cap if plen is None else plen, self.n,
                self.nbt if nbt is None else nbt)

    def model(self, crc=None, nbt=None, plen=None):
        """the same view as the models take a source: the stored bytes are followed by the zeros of the device buffer up to plen"""
        crc, plen = self.with_crc if crc is None else crc, self.cap if plen is None else plen
        if self.base:
            packed = type(self.packed)(self.base, (self.packed.data + bytes(max(0, plen - self.plen)))[:max(0, plen - self.base)])
        else:
            packed = (self.packed + bytes(max(0, plen - self.plen)))[:plen]
        return (packed, plen, self.first, self.off, self.lens, self.crc if crc else None, self.n, self.nbt if nbt is None else nbt)

    def host(self):
        """what the host conveniences take as a container"""
        return (self.packed, self.first, self.off, self.lens, self.crc)

    def written(self, writes):
        """the container after blocks_write of (resource, offset, bytes)"""
        packed, off, crc, wr, st, rst = self.m.blocks_write(self.fmt, *self.host()[:4], self.B, writes, ctx=self.ctx, block_crc=self.crc)
        assert st == [0] * len(writes) and not any(rst) and wr == [len(b) for _, _, b in writes]
        return Container.from_host(self.ctx, self.fmt, self.B, packed, self.first, off, self.lens, crc)

    def resized(self, lens):
        """the container after blocks_resize to these lengths"""
        packed, off, crc, first, new_lens, rst = self.m.blocks_resize(self.fmt, *self.host()[:4], self.B, lens, ctx=self.ctx, block_crc=self.crc)
        assert not any(rst) and new_lens == list(lens)
        return Container.from_host(self.ctx, self.fmt, self.B, packed, first, off, new_lens, crc)

    def blocks(self, r):
        return (self.lens[r] + self.B - 1) // self.B

    def fresh(self, bufs):
        """fresh() through the container's own BlockContainer: other bytes of the same lengths"""
        return fresh(self.ctx, self.bk, bufs)

    # -- the geometry of (resource, offset, length) requests against this container, for readers and writers
    def wants(self, reqs):
        out = []
        for r, o, ln in reqs:
            L = self.lens[r] if r < self.n else 0
            out.append(min(ln, L - min(o, L)))
        return out

    def budget(self, reqs):
        return sum(len(R.covering(min(o, self.lens[r]), w, self.B)) for (r, o, ln), w in zip(reqs, self.wants(reqs)) if w and r < self.n)

    def layout(self, caps, residues=None):
        """offsets of buffers of ``caps`` bytes with BYTE_GUARD bytes between them, buffer q at the residue (7 q + 3) % 16, and the room"""
        off, pos = [], BYTE_GUARD
        for q, c in enumerate(caps):
            pos = (pos + 15) // 16 * 16 + (residues[q] if residues else (7 * q + 3) % 16)
            off.append(pos)
            pos += c + BYTE_GUARD
        return off, pos + 16

    def close(self):
        if self.bk is not None:
            self.bk.close()


def flip(oracle, con, j, e, decodes):
    """a byte of stored block j whose flip the reference's decoder takes with defined behaviour: to other bytes (decodes) or to an error"""
    o0, o1 = int(con.off[j]), int(con.off[j + 1])
    good = oracle.oracle_decompress_ex(con.fmt, con.packed[o0:o1], e)[1]
    for p in range(o1 - o0 - 1, -1, -1):
        blk = bytearray(con.packed[o0:o1]); blk[p] ^= 0x01
        ds, got, undefined = oracle.oracle_decompress_ex(con.fmt, bytes(blk), e)
        if not undefined and ((ds == 0 and len(got) == e and got != good) if decodes else (ds != 0 or len(got) != e)):
            return o0 + p
    raise AssertionError("no such byte in this block")


def long_runs(cls, ctx):
    """(container of class cls, first row of the long resource) where the runs of a move pass matter, with its shape assertions: B = 4096,
    Xpress, a small text resource, one of 311 blocks -- random and text by turns, then 150 blocks of zeros (hundreds of rows within one
    4096-byte slice of the new container), then text --, a small random one"""
    B = 4096
    long = recipe("mixed", 21, 100, 0, B) + bytes(150 * B) + recipe("text", 22, 60, 17, B)
    con = cls.make(ctx, FMTS["xpress"], B, [recipe("text", 23, 1, 5, B), long, recipe("random", 24, 0, 77, B)])
    stored = np.diff(con.off[: int(con.first[-1]) + 1].astype(np.int64))
    assert int(con.first[2] - con.first[1]) == 311 and len(set(stored.tolist())) > 20 and (stored[120:240] < 64).all()
    return con, int(con.first[1])


# ---- one BlockContainer driven in place ---------------------------------------------------------------------------------------------------
class BlockRig:
    """one BlockContainer with device buffers that stay where they are: load() / set_*() rewrite their contents in place"""

    def __init__(self, ctx, fmt, B, n, in_total_max, in_room=None, out_room=None):
        import torch
        import ms_compress_amd as m
        self.ctx, self.fmt, self.B, self.n, self.itm = ctx, fmt, B, n, in_total_max
        self.dev = dev = torch.device("cuda", ctx.device)
        self.bk = m.BlockContainer(ctx, fmt, B, n, in_total_max)
        self.nbmax = self.bk.n_blocks_max
        assert self.nbmax == n + in_total_max // B
        in_room = in_room or in_total_max
        z64 = lambda k: torch.zeros(max(1, k), dtype=torch.int64, device=dev)
        self.d_in = torch.zeros(in_room + 3 * n + 64, dtype=torch.uint8, device=dev)
        self.d_off, self.d_len = z64(n), z64(n)
        self.d_packed = torch.zeros(in_room + CAP_GUARD, dtype=torch.uint8, device=dev)
        self.d_first, self.d_boff, self.d_cst = z64(n + 1), z64(self.nbmax + 1), torch.zeros(max(1, n), dtype=torch.int32, device=dev)
        self.d_out = torch.zeros((out_room or in_room) + (CAP_GUARD + 16) * (n + 1), dtype=torch.uint8, device=dev)
        self.d_ooff, self.d_ocap, self.d_olen, self.d_range = z64(n), z64(n), z64(n), z64(2 * n)
        self.d_dst = torch.zeros(max(1, n), dtype=torch.int32, device=dev)

    def load(self, bufs):
        """resources at odd offsets (every source alignment), the buffers refilled"""
        import torch
        assert len(bufs) == self.n
        self.bufs, self.lens = bufs, [len(b) for b in bufs]
        off, blob = odd_offsets(bufs, self.d_in.numel())
        self.d_in.copy_(torch.from_numpy(blob))
        self.d_off.copy_(d64(off, self.dev)); self.d_len.copy_(d64(self.lens, self.dev))

    def compress(self, packed_cap=None):
        self.d_packed.fill_(FILL); self.d_first.fill_(-1); self.d_boff.fill_(-1); self.d_cst.fill_(ST_FILL)
        self.cap = self.d_packed.numel() - CAP_GUARD if packed_cap is None else packed_cap
        self.bk.compress(self.d_in, self.d_off, self.d_len, self.d_packed, self.d_first, self.d_boff, self.d_cst, packed_cap=self.cap)

    def compressed(self):
        self.ctx.stream.synchronize()
        return (self.d_packed.cpu().numpy(), self.d_first.cpu().numpy().view(np.uint64), self.d_boff.cpu().numpy().view(np.uint64),
                self.d_cst.cpu().numpy()[: self.n])

    def check_compress(self, oracle, packed_cap=None):
        """run, and compare everything with the model; returns the model's (packed, first, off, status)"""
        self.compress(packed_cap)
        packed, first, off, st = self.compressed()
        mp, mf, mo, ms = M.model_compress(oracle, self.fmt, self.bufs, self.B, self.itm, self.cap)
        assert (first == mf).all() and (off == mo).all(), "tables"
        assert [int(x) for x in st] == [int(x) for x in ms], "statuses"
        assert bytes(packed[: len(mp)]) == mp, "packed bytes"
        assert (packed[len(mp):] == FILL).all(), "written behind the last block that fits / behind packed_cap"
        return mp, mf, mo, ms

    def set_out(self, caps):
        self.caps = [int(c) for c in caps]
        off, pos = [], CAP_GUARD + 5
        for c in self.caps:
            off.append(pos)
            pos += c + CAP_GUARD
        assert pos <= self.d_out.numel()
        self.ooff = off
        self.d_ooff.copy_(d64(off, self.dev)); self.d_ocap.copy_(d64(self.caps, self.dev))

    def decompress(self, ranges=None, packed_len=None, first=None, boff=None, packed=None):
        self.d_out.fill_(FILL); self.d_olen.fill_(-1); self.d_dst.fill_(ST_FILL)
        if ranges is not None:
            self.d_range.copy_(d64(np.array(ranges, dtype=np.uint64).reshape(-1), self.dev))
        self.bk.decompress(self.d_packed if packed is None else packed, self.d_first if first is None else first, self.d_boff if boff is None else boff,
                           self.d_len, self.d_out, self.d_ooff, self.d_ocap, self.d_olen, self.d_dst,
                           d_range=None if ranges is None else self.d_range, packed_len=packed_len)
        self.ctx.stream.synchronize()
        return self.d_out.cpu().numpy(), self.d_olen.cpu().numpy().view(np.uint64)[: self.n], self.d_dst.cpu().numpy()[: self.n]

    def check_decompress(self, oracle, model_args, ranges=None, **kw):
        """model_args = (packed bytes, packed_len, first, off) the model decodes; kw: what the device call gets in their place"""
        out, olen, st = self.decompress(ranges, packed_len=model_args[1], **kw)
        mo, ms = M.model_decompress(oracle, self.fmt, model_args[0], model_args[1], model_args[2], model_args[3], self.lens, self.B, self.itm, self.caps, ranges)
        assert [int(x) for x in st] == ms, ("statuses", [int(x) for x in st], ms)
        keep = np.ones(len(out), dtype=bool)
        for r in range(self.n):
            o, c = self.ooff[r], self.caps[r]
            keep[o: o + c] = False
            if ms[r] == 0:
                assert int(olen[r]) == len(mo[r]) and bytes(out[o: o + len(mo[r])]) == mo[r], ("bytes of resource", r)
                assert (out[o + len(mo[r]): o + c] == FILL).all(), ("written behind the range of resource", r)
            else:
                assert int(olen[r]) == 0
                if ms[r] in (M.ARG, M.BUF):
                    assert (out[o: o + c] == FILL).all(), ("a rejected resource was written", r)
        assert (out[keep] == FILL).all(), "written outside every capacity"
        return mo, ms

    def close(self):
        self.bk.close()


def fixture_bufs(fixture, fmt, B):
    return [M.build(r, B) for r in M.recipes_for(fixture, fmt, B)]


def crc_bufs(fixture, f, B):
    return fixture_bufs(fixture, f, B) + [np.random.RandomState(77).bytes(2 * B + 100)]   # (one incompressible resource added)


class CrcRig(BlockRig):
    """BlockRig with the checksum arrays of BlockContainer.crc / .check, against tests/crc_model.py"""

    def __init__(self, *a, **kw):
        import torch
        super().__init__(*a, **kw)
        self.d_bcrc, self.d_rcrc, self.d_kst = (torch.zeros(max(1, k), dtype=torch.int32, device=self.dev) for k in (self.nbmax, self.n, self.n))

    def crc(self):
        self.d_bcrc.fill_(0x5A5A5A5A); self.d_rcrc.fill_(0x5A5A5A5A); self.d_kst.fill_(ST_FILL)
        self.bk.crc(self.d_in, self.d_off, self.d_len, self.d_bcrc, self.d_kst, d_res_crc=self.d_rcrc)

    def check_crc(self):
        self.crc()
        self.ctx.stream.synchronize()
        bc, rc, st = K.blocks(self.bufs, self.B, self.itm)
        assert (u32(self.d_bcrc, self.nbmax) == bc).all(), "block crcs"
        assert (u32(self.d_rcrc, self.n) == rc).all(), "resource crcs"
        assert (self.d_kst.cpu().numpy()[: self.n] == st).all()
        return bc, rc, st

    def decode_and_check(self, ranges=None, packed=None):
        """decompress, then check with the same tables; returns (statuses after decompress, statuses and lengths after check)"""
        out, olen, st = self.decompress(ranges, packed_len=self.d_packed.numel() - 64, packed=packed)
        self.bk.check(self.d_out, self.d_ooff, self.d_len, self.d_first, self.d_bcrc, self.d_olen, self.d_dst,
                      d_range=None if ranges is None else self.d_range)
        self.ctx.stream.synchronize()
        st2, olen2 = self.d_dst.cpu().numpy()[: self.n], self.d_olen.cpu().numpy().view(np.uint64)[: self.n]
        ms, ml = K.check(out, self.ooff, self.lens, self.d_first.cpu().numpy().view(np.uint64), u32(self.d_bcrc, self.nbmax), st, olen,
                         self.B, self.itm, ranges)
        assert [int(x) for x in st2] == ms and [int(x) for x in olen2] == ml, ("check against the model", [int(x) for x in st2], ms)
        assert (self.d_out.cpu().numpy() == out).all(), "check wrote to the output"
        return [int(x) for x in st], [int(x) for x in st2], [int(x) for x in olen2]


# ---- the container a call writes ----------------------------------------------------------------------------------------------------------
class NewContainer:
    """The arrays a call writes a new container of n resources and nbt table rows into, sentinel-filled: d_new (room + 64 bytes of FILL),
    d_first (n + 1) and d_off (nbt + 1) of -1, d_crc (nbt words of CRC_FILL, one at least; None without ``crc``), d_len of -1 (None
    without ``lens``: the call writes no lengths) and d_st of ST_FILL (n entries, one at least). ``fill``: one value for every table,
    checksum, length and status in place of these (the transcoder's tests keep their -77)."""

    def __init__(self, dev, n, nbt, room, crc=True, lens=True, fill=None):
        import torch
        self.n, self.nbt, self.room = n, nbt, room
        self.fills = (-1, CRC_FILL, ST_FILL) if fill is None else (fill, fill, fill)     # tables and lengths, checksums, statuses
        full = lambda k, v, t: torch.full((k,), v, dtype=t, device=dev)
        self.d_new = full(room + 64, FILL, torch.uint8)
        self.d_first, self.d_off = full(n + 1, self.fills[0], torch.int64), full(nbt + 1, self.fills[0], torch.int64)
        self.d_crc = full(max(1, nbt), self.fills[1], torch.int32) if crc else None
        self.d_len = full(max(1, n), self.fills[0], torch.int64) if lens else None
        self.d_st = full(max(1, n), self.fills[2], torch.int32)

    def tensors(self):
        return self.d_new, self.d_first, self.d_off, self.d_crc, self.d_len, self.d_st

    def fill(self):
        self.d_new.fill_(FILL); self.d_first.fill_(self.fills[0]); self.d_off.fill_(self.fills[0]); self.d_st.fill_(self.fills[2])
        if self.d_len is not None:
            self.d_len.fill_(self.fills[0])
        if self.d_crc is not None:
            self.d_crc.fill_(self.fills[1])

    def pull(self):
        """everything on the host, whole: image, first, off, crc (or None), new_len (or None), status -- and the tensors themselves under "d" """
        return {"d": self.tensors(), "image": self.d_new.cpu().numpy(), "first": self.d_first.cpu().numpy().view(np.uint64),
                "off": self.d_off.cpu().numpy().view(np.uint64), "crc": None if self.d_crc is None else self.d_crc.cpu().numpy().view(np.uint32),
                "new_len": None if self.d_len is None else [int(x) for x in self.d_len.cpu().numpy().view(np.uint64)],
                "status": [int(x) for x in self.d_st.cpu().numpy()]}

    def view(self):
        """the written container as a source of the next call"""
        return (self.d_new, self.d_first, self.d_off, self.d_len, self.d_crc, self.room, self.n, self.nbt)

    @staticmethod
    def compare(got, model, what, n, nbt, crc=True, status="status", fills=(-1, CRC_FILL, ST_FILL)):
        """pull()'s arrays against a model's dict (packed, first, off, crc, new_len and statuses under ``status``), whole: with n = 0 the
        one-entry status and length arrays still hold their sentinels; a checksum array that the call was not given (crc=False), or a table
        without rows, still holds its fill; the image is the model's bytes over FILL. An array the rig does not have (None) is passed over."""
        assert got["status"] == ([int(x) for x in model[status]] if n else [fills[2]]), (what, "statuses", got["status"], model[status])
        if got["new_len"] is not None:
            assert got["new_len"] == ([int(x) for x in model["new_len"]] if n else [fills[0] & M.M64]), (what, "lengths", got["new_len"], model["new_len"])
        assert np.array_equal(got["first"], model["first"]), (what, "first", got["first"], model["first"])
        assert np.array_equal(got["off"], model["off"]), (what, "offsets", got["off"], model["off"])
        if got["crc"] is not None:
            want = model["crc"] if crc and nbt else np.full(max(1, nbt), fills[1] & 0xFFFFFFFF, dtype=np.uint32)
            assert np.array_equal(got["crc"], want), (what, "checksums", np.nonzero(got["crc"] != want)[0])
        same_image(got["image"], model["packed"], FILL, (what, "new packed bytes, %d in the model" % len(model["packed"])))

    def against(self, model, what, crc=True, status="status"):
        got = self.pull()
        self.compare(got, model, what, self.n, self.nbt, crc, status, self.fills)
        return got


class Spliced(NewContainer):
    """the container a splicer writes by extents: room = cap, checksums only with_crc"""

    def __init__(self, dev, n, nbt, cap, with_crc):
        NewContainer.__init__(self, dev, n, nbt, cap, crc=with_crc)

    def run(self, sp, sources, d_ext_first, d_ext):
        sp.splice_extents(sources, d_ext_first, d_ext, self.d_new, self.d_first, self.d_off, self.d_len, self.d_st, d_new_block_crc=self.d_crc, new_cap=self.room)

    def as_built(self):
        got = self.pull()
        return {"packed": got["image"], "first": got["first"], "off": got["off"], "crc": got["crc"], "new_len": got["new_len"][: self.n]}


# ---- splices, by picks and by extents --------------------------------------------------------------------------------------------------
class Splices:
    """splice calls against two containers: rig[0] holds R.buffers(B), rig[1] the same buffers in the order ORDER2; src = the sources of a
    call, by default the two as they are (Container.edited gives damaged ones)"""

    def __init__(self, ctx, fmt, B, bufs0=None, bufs1=None):
        base = R.buffers(B)
        self.rig = [Container.make(ctx, fmt, B, bufs0 or base), Container.make(ctx, fmt, B, bufs1 or [base[i] for i in ORDER2])]
        self.m, self.ctx, self.fmt, self.B, self.dev = self.rig[0].m, ctx, fmt, B, self.rig[0].dev
        self.room = 2 * max(r.total for r in self.rig) + 3 * B
        self.src = list(self.rig)

    def outputs(self, npk, nbt):
        """the sentinel-filled NewContainer of a call: npk resources, nbt rows, the room of every call here"""
        return NewContainer(self.dev, npk, nbt, self.room)

    def pull(self, outs):
        self.ctx.stream.synchronize()
        return outs.pull()

    def compare(self, got, mo, npk, nbt, crc=True):
        """everything the call wrote, and everything it must not have written, against the model"""
        NewContainer.compare(got, mo, "spliced", npk, nbt, crc)

    def check(self, picks, nbt, srcs=None, cap=None, crc=True, splicer=None):
        """run, and compare with the model; returns (model, outputs)"""
        srcs = self.src if srcs is None else srcs
        npk = len(picks)
        cap = self.room if cap is None else cap
        outs = self.outputs(npk, nbt)
        d_new, d_first, d_off, d_crc, d_len, d_st = outs.tensors()
        sp = splicer or self.m.BlockSplicer(self.ctx, self.B, len(srcs), npk, nbt)
        d_pick = d64(np.array(picks, dtype=np.uint64), self.dev, 2)
        sp.splice([s.view() for s in srcs], d_pick, d_new, d_first, d_off, d_len, d_st, d_new_block_crc=d_crc if crc else None, new_cap=cap)
        got = self.pull(outs)
        if splicer is None:
            sp.close()
        mo = S.model_splice([s.model() for s in srcs], picks, self.B, nbt, cap, with_crc=crc)
        self.compare(got, mo, npk, nbt, crc)
        return mo, got

    def data(self, picks):
        return S.picked([r.bufs for r in self.rig], picks)

    def table_for(self, picks):
        """the rows of the container BlockContainer makes for the picked data: n_blocks_max = n + total // B"""
        return len(picks) + sum(len(b) for b in self.data(picks)) // self.B

    def check_consequence(self, got, data, nbt):
        """the header's consequence: the new container is what compress and crc write for the picked data, whole tables included"""
        bk = self.m.BlockContainer(self.ctx, self.fmt, self.B, len(data), sum(len(b) for b in data))
        assert bk.n_blocks_max == nbt
        packed, first, off, crc = fresh(self.ctx, bk, data)
        bk.close()
        assert (got["first"] == first).all() and (got["off"] == off).all() and int(got["off"][-1]) == len(packed)
        assert (got["crc"] == crc).all() and bytes(got["image"][: len(packed)]) == packed

    def close(self):
        for r in self.rig:
            r.close()


class Extents(Splices):
    """splice_extents calls against two Rigs: rig[0] holds buffers(B), rig[1] the same reversed"""

    def __init__(self, ctx, fmt, B, bufs0=None, bufs1=None):
        base = X.buffers(B)
        Splices.__init__(self, ctx, fmt, B, bufs0 or base, bufs1 or base[::-1])

    def run(self, sp, srcs, ext_first, ext, outs, cap, crc=True):
        d_new, d_first, d_off, d_crc, d_len, d_st = outs.tensors()
        d_ext = d64(np.array(ext, dtype=np.uint64), self.dev, 4)
        sp.splice_extents([s.view() for s in srcs], d64(ext_first, self.dev), d_ext, d_new, d_first, d_off, d_len, d_st,
                          d_new_block_crc=d_crc if crc else None, new_cap=cap)
        return self.pull(outs)

    def check(self, resources, nbt, srcs=None, cap=None, crc=True, ext_first=None, n_ext=None):
        """run, and compare with the model; returns (model, outputs)"""
        srcs = self.src if srcs is None else srcs
        ef, ext = X.flat(resources)
        ef = ef if ext_first is None else ext_first
        n_res, n_ext = len(resources), len(ext) if n_ext is None else n_ext
        cap = self.room if cap is None else cap
        sp = self.m.BlockSplicer.for_extents(self.ctx, self.B, len(srcs), n_res, n_ext, nbt)
        got = self.run(sp, srcs, ef, ext, self.outputs(n_res, nbt), cap, crc)
        sp.close()
        mo = X.model_splice_extents([s.model() for s in srcs], ef, ext, self.B, n_ext, nbt, cap, with_crc=crc)
        self.compare(got, mo, n_res, nbt, crc)
        return mo, got

    def data(self, resources):
        return X.extent_data([r.bufs for r in self.rig], resources, self.B)

    def table_for(self, resources):
        """the rows of the container BlockContainer makes for the extent data: n_blocks_max = n + total // B"""
        return len(resources) + sum(len(b) for b in self.data(resources)) // self.B


# ---- the lists a call writes ---------------------------------------------------------------------------------------------------------------
class ListOuts:
    """Named int64 output arrays of the given sizes, each with ENTRY_GUARD entries behind it, filled with SENT, and one int32 status array
    of n_status + ENTRY_GUARD entries filled with SENT32: longer than a call may write, so a write behind an array's end fails."""

    def __init__(self, dev, sizes, n_status):
        import torch
        self.sizes, self.n_status = dict(sizes), n_status
        self.t = {k: torch.full((v + ENTRY_GUARD,), SENT, dtype=torch.int64, device=dev) for k, v in self.sizes.items()}
        self.status = torch.full((n_status + ENTRY_GUARD,), SENT32, dtype=torch.int32, device=dev)

    def __getitem__(self, name):
        return self.t[name]

    def tensors(self):
        return tuple(self.t.values()) + (self.status,)

    def reset(self):
        for t in self.t.values():
            t.fill_(SENT)
        self.status.fill_(SENT32)

    def pull(self):
        got = {k: [int(x) for x in t.cpu().numpy().view(np.uint64)] for k, t in self.t.items()}
        got["status"] = [int(x) for x in self.status.cpu().numpy()]
        return got

    def untouched(self):
        return all(set(v) == {SENT32 if k == "status" else SENT} for k, v in self.pull().items())

    @staticmethod
    def compare(got, model, exact=(), prefixes=()):
        """pull()'s lists against a model's: an ``exact`` key is the model's list and nothing but sentinels behind it, a ``prefixes`` key
        begins with the model's extents, flattened, and has nothing but sentinels behind them; the statuses are an exact key"""
        for k in tuple(exact) + ("status",):
            want = [int(x) for x in model[k]]
            assert got[k] == want + [SENT32 if k == "status" else SENT] * (len(got[k]) - len(want)), (k, got[k], model[k])
        for k in prefixes:
            want = [int(x) for e in model[k] for x in e]
            assert got[k][: len(want)] == want, (k, got[k][: len(want)], model[k])
            assert set(got[k][len(want):]) == {SENT}, (k, "written behind the extents in use")

    def against(self, model, exact=(), prefixes=()):
        got = self.pull()
        self.compare(got, model, exact, prefixes)
        return got


def same_lists(outs, want):
    """a ListOuts against closed-form expectations, whole and in numpy (ListOuts.compare goes entry by entry in Python lists: not for a
    call over a million rows): every list named in ``want`` -- the statuses under "status" -- begins with want's entries and holds
    nothing but its sentinel behind them"""
    for k, w in want.items():
        got = outs.status.cpu().numpy() if k == "status" else outs[k].cpu().numpy().view(np.uint64)
        w = np.asarray(w, dtype=got.dtype).reshape(-1)
        bad = np.nonzero(got[: len(w)] != w)[0]
        assert bad.size == 0, (k, "differs at entry", int(bad[0]), int(got[bad[0]]), int(w[bad[0]]))
        assert (got[len(w):] == (SENT32 if k == "status" else SENT)).all(), (k, "written behind the entries in use")


def table_only(ctx, B, rows):
    """a Container of hand-made tables and no stored byte: resource r has rows[r] whole blocks, each of stored length 0 (packed_len 0,
    every block_off 0, every checksum 0). The table-only passes of the dedupers take it at a million rows."""
    nbt = int(sum(rows))
    return Container.from_host(ctx, FMTS["xpress"], B, b"", np.concatenate([[0], np.cumsum(rows)]), np.zeros(nbt + 1, dtype=np.uint64),
                               [int(k) * B for k in rows], np.zeros(nbt, dtype=np.uint32))


# ---- readers --------------------------------------------------------------------------------------------------------------------------------
class ReadRig(Container):
    """a container made on the GPU once (ReadRig.make); read() / check() run request batches against it"""

    def read(self, reqs, blocks_max=None, caps=None, crc=False, residues=None, first=None, boff=None, packed=None, packed_len=None, reader=None, d_out=None):
        import torch
        caps = self.wants(reqs) if caps is None else caps
        blocks_max = self.budget(reqs) if blocks_max is None else blocks_max
        ooff, room = self.layout(caps, residues)
        rd = reader or self.m.BlockReader(self.ctx, self.fmt, self.B, self.n, self.nbt, len(reqs), blocks_max)
        d_out = torch.empty(room, dtype=torch.uint8, device=self.dev) if d_out is None else d_out
        d_out.fill_(FILL)
        nq = max(1, len(reqs))
        d_req = d64(np.array(reqs, dtype=np.uint64), self.dev, 3)
        d_ooff, d_ocap = d64(ooff, self.dev), d64(caps, self.dev)
        d_olen = torch.full((nq,), -1, dtype=torch.int64, device=self.dev)
        d_st = torch.full((nq,), ST_FILL, dtype=torch.int32, device=self.dev)
        rd.read(self.d_packed if packed is None else packed, self.d_first if first is None else d64(first, self.dev),
                self.d_boff if boff is None else d64(boff, self.dev), self.d_len, d_req, d_out, d_ooff, d_ocap, d_olen, d_st,
                d_block_crc=self.d_crc if crc else None, packed_len=self.plen if packed_len is None else packed_len)
        counts = rd.counts()
        if reader is None:
            rd.close()
        return d_out.cpu().numpy(), d_olen.cpu().numpy().view(np.uint64)[: len(reqs)], [int(x) for x in d_st.cpu().numpy()[: len(reqs)]], ooff, counts

    def check(self, oracle, reqs, blocks_max=None, caps=None, crc=False, model_packed=None, **kw):
        """run, and compare statuses, lengths, counts and the WHOLE output buffer with the model; returns (outputs, statuses, counts)"""
        caps = self.wants(reqs) if caps is None else caps
        blocks_max = self.budget(reqs) if blocks_max is None else blocks_max
        out, olen, st, ooff, counts = self.read(reqs, blocks_max, caps, crc, **kw)
        mo, ms, mc = R.model_read(oracle, self.fmt, self.packed if model_packed is None else model_packed,
                                  self.plen if kw.get("packed_len") is None else kw["packed_len"],
                                  self.first if kw.get("first") is None else kw["first"], self.off if kw.get("boff") is None else kw["boff"],
                                  self.lens, self.B, self.nbt, reqs, caps, blocks_max, self.crc if crc else None)
        assert st == ms, ("statuses", st, ms)
        for q, o in enumerate(mo):
            assert int(olen[q]) == (len(o) if ms[q] == 0 else 0), ("length of request", q)
        same_image(out, [(ooff[q], o) for q, o in enumerate(mo) if ms[q] == 0 and o], FILL, ("output, request offsets", ooff))
        assert counts == mc, ("counts", counts, mc)
        return mo, ms, mc


def slices(rig, reqs):
    return [rig.bufs[r][o: o + min(ln, rig.lens[r])] for r, o, ln in reqs]


def geometry(rig):
    B, reqs = rig.B, []
    for r, L in enumerate(rig.lens):                              # every resource: whole, at and behind its end, nothing, its first and last byte
        reqs += [(r, 0, ALL), (r, L, 5), (r, L + 7, ALL), (r, 3, 0), (r, 0, 1), (r, max(0, L - 1), 1), (r, B - 1, 1), (r, B, 1)]
    for r in (MIXED, TEXT, MIXED5):
        reqs += [(r, B + 100, 50), (r, B - 3, 10), (r, B - 1, 2 * B + 2), (r, B, B), (r, 0, 2 * B), (r, 2 * B, B), (r, 1, B - 1), (r, B, 2 * B + 17)]
    for r in (MIXED, TEXT):                                       # the short last block
        reqs += [(r, 3 * B, 17), (r, 3 * B + 5, 100), (r, 3 * B - 1, 2), (r, 3 * B + 16, 1)]
    return reqs


# ---- writers: write --------------------------------------------------------------------------------------------------------------------------
class Writes:
    """write batches against a Container made on the GPU (or against another container of the same resources: cont=)"""

    def __init__(self, rig):
        self.rig = rig

    def run(self, reqs, srcs, blocks_max=None, crc=True, new_cap=None, first=None, boff=None, packed=None, packed_len=None, residues=None, writer=None,
            cont=None):
        import torch
        rig = self.rig
        dev, nq = rig.dev, max(1, len(reqs))
        wants = rig.wants(reqs)
        blocks_max = rig.budget(reqs) if blocks_max is None else blocks_max
        soff, room = rig.layout(wants, residues)
        blob = np.full(room, 0xEE, dtype=np.uint8)
        for o, w, s in zip(soff, wants, srcs):
            blob[o: o + w] = np.frombuffer(bytes(s[:w]), dtype=np.uint8)
        d_src, d_soff = torch.from_numpy(blob).to(dev), d64(soff, dev)
        d_req = d64(np.array(reqs, dtype=np.uint64), dev, 3)
        cap = rig.total if new_cap is None else new_cap
        d_new = torch.full((rig.total + 64,), FILL, dtype=torch.uint8, device=dev)
        d_noff = torch.full((rig.nbt + 1,), -1, dtype=torch.int64, device=dev)
        d_ncrc = torch.full((max(1, rig.nbt),), CRC_FILL, dtype=torch.int32, device=dev) if crc else None
        d_wr = torch.full((nq,), -1, dtype=torch.int64, device=dev)
        d_st = torch.full((nq,), ST_FILL, dtype=torch.int32, device=dev)
        d_rst = torch.full((rig.n,), ST_FILL, dtype=torch.int32, device=dev)
        d_packed, plen, d_boff, d_crc = cont or (rig.d_packed if packed is None else packed, rig.plen if packed_len is None else packed_len,
                                                 rig.d_boff if boff is None else d64(boff, dev), rig.d_crc)
        wr = writer or rig.m.BlockWriter(rig.ctx, rig.fmt, rig.B, rig.n, rig.nbt, len(reqs), blocks_max)
        wr.write(d_packed, rig.d_first if first is None else d64(first, dev), d_boff, rig.d_len, d_req, d_src, d_soff, d_new, d_noff, d_wr, d_st, d_rst,
                 d_block_crc=d_crc if crc else None, d_new_block_crc=d_ncrc, packed_len=plen, new_cap=cap)
        counts = wr.counts()
        if writer is None:
            wr.close()
        return {"d": (d_new, d_noff, d_ncrc), "image": d_new.cpu().numpy(), "off": d_noff.cpu().numpy().view(np.uint64),
                "crc": None if d_ncrc is None else d_ncrc.cpu().numpy().view(np.uint32)[: rig.nbt],
                "written": [int(x) for x in d_wr.cpu().numpy().view(np.uint64)[: len(reqs)]],
                "status": [int(x) for x in d_st.cpu().numpy()[: len(reqs)]], "res_status": [int(x) for x in d_rst.cpu().numpy()], "counts": counts}

    def check(self, oracle, reqs, srcs, blocks_max=None, crc=True, new_cap=None, model_cont=None, model_packed=None, **kw):
        """run, and compare everything the call wrote with the model; returns (what the model says, what the device said)"""
        rig = self.rig
        blocks_max = rig.budget(reqs) if blocks_max is None else blocks_max
        cap = rig.total if new_cap is None else new_cap
        got = self.run(reqs, srcs, blocks_max, crc, cap, **kw)
        packed, plen, off, bcrc = model_cont or (rig.packed if model_packed is None else model_packed,
                                                 rig.plen if kw.get("packed_len") is None else kw["packed_len"],
                                                 rig.off if kw.get("boff") is None else kw["boff"], rig.crc)
        mo = W.model_write(oracle, rig.fmt, packed, plen, rig.first if kw.get("first") is None else kw["first"], off, rig.lens, rig.B, rig.nbt,
                           reqs, srcs, blocks_max, cap, bcrc if crc else None)
        for key in ("status", "written", "res_status", "counts"):
            assert got[key] == mo[key], (key, got[key], mo[key])
        assert (got["off"] == mo["off"]).all(), ("offsets", got["off"], mo["off"])
        if crc:
            assert (got["crc"] == mo["crc"]).all(), ("checksums", np.nonzero(got["crc"] != mo["crc"])[0])
        same_image(got["image"], mo["packed"], FILL, "new packed bytes, %d in the model" % len(mo["packed"]))
        return mo, got

    def check_rule_10(self, got, reqs, srcs):
        packed, _, off, crc = self.rig.fresh(W.patched(self.rig.bufs, reqs, srcs))
        assert (got["off"] == off).all() and bytes(got["image"][: len(packed)]) == packed
        assert got["crc"] is None or (got["crc"] == crc).all()

    def close(self):
        self.rig.close()


def sources(rig, reqs, seed, kinds=None):
    rs = np.random.RandomState(seed)
    out = []
    for q, w in enumerate(rig.wants(reqs)):
        kind = kinds[q] if kinds else q % 3
        out.append(bytes(w) if kind == 0 else rs.bytes(w) if kind == 1 else (b"written text " * (w // 13 + 1))[:w])
    return out


# ---- writers: resize -------------------------------------------------------------------------------------------------------------------------
BUDGET = 24                                                     # blocks_max of the resize writers


class Resizes:
    """resize calls against a Container made on the GPU, its tables widened to nb + SPARE rows"""

    def __init__(self, rig):
        self.rig = rig
        nb = int(rig.first[-1])
        self.nbt = nb + SPARE
        self.off = np.concatenate([rig.off[: nb + 1], np.full(SPARE, rig.off[nb], dtype=np.uint64)])
        self.crc = np.concatenate([rig.crc[:nb], np.zeros(SPARE, dtype=np.uint32)])
        self.d_boff, self.d_crc = d64(self.off, rig.dev), i32(self.crc, rig.dev)
        self.room = rig.total + BUDGET * rig.B                   # what the resources can hold after one call
        self.big = rig.m.BlockContainer(rig.ctx, rig.fmt, rig.B, rig.n, self.room)

    def outputs(self):
        """(d_new, d_nfirst, d_noff, d_ncrc, d_nlen, d_rst), sentinel-filled"""
        return NewContainer(self.rig.dev, self.rig.n, self.nbt, self.room).tensors()

    def run(self, want, blocks_max=BUDGET, crc=True, new_cap=None, first=None, boff=None, packed=None, lens=None, writer=None):
        rig, dev = self.rig, self.rig.dev
        outs = NewContainer(dev, rig.n, self.nbt, self.room)
        d_new, d_nfirst, d_noff, d_ncrc, d_nlen, d_rst = outs.tensors()
        wr = writer or rig.m.BlockWriter(rig.ctx, rig.fmt, rig.B, rig.n, self.nbt, 0, blocks_max)
        wr.resize(rig.d_packed if packed is None else packed, rig.d_first if first is None else d64(first, dev),
                  self.d_boff if boff is None else d64(boff, dev), rig.d_len if lens is None else d64(lens, dev), d64(want, dev),
                  d_new, d_nfirst, d_noff, d_nlen, d_rst, d_block_crc=self.d_crc if crc else None, d_new_block_crc=d_ncrc if crc else None,
                  packed_len=rig.plen, new_cap=self.room if new_cap is None else new_cap)
        counts = wr.counts()
        if writer is None:
            wr.close()
        got = outs.pull()                                          # (the resource statuses under "status")
        got["counts"] = counts
        return got

    def check(self, oracle, want, blocks_max=BUDGET, crc=True, new_cap=None, model_packed=None, read_back=True, **kw):
        """run, compare everything the call wrote with the model, and read every resource of the new container back"""
        rig = self.rig
        cap = self.room if new_cap is None else new_cap
        got = self.run(want, blocks_max, crc, cap, **kw)
        lens = rig.lens if kw.get("lens") is None else kw["lens"]
        mo = Z.model_resize(oracle, rig.fmt, rig.packed if model_packed is None else model_packed, rig.plen,
                            rig.first if kw.get("first") is None else kw["first"], self.off if kw.get("boff") is None else kw["boff"], lens, rig.B,
                            self.nbt, want, blocks_max, cap, self.crc if crc else None)
        NewContainer.compare(got, mo, "resized", rig.n, self.nbt, crc, status="res_status")
        assert got["counts"] == mo["counts"], ("counts", got["counts"], mo["counts"])
        if not crc:
            got["crc"] = None                                      # (compared above: the array the call was not given still holds CRC_FILL)
        if read_back and not any(mo["res_status"]) and model_packed is None and kw.get("boff") is None:
            self.read_back(got, Z.resized(rig.bufs, mo["new_len"]))
        return mo, got

    def read_back(self, got, data):
        rig = self.rig
        nb = int(got["first"][-1])
        out, st = rig.m.blocks_read(rig.fmt, got["image"][: int(got["off"][nb])], got["first"], got["off"], [len(b) for b in data], rig.B,
                                    [(r, 0, ALL) for r in range(rig.n)], ctx=rig.ctx, block_crc=got["crc"])
        assert st == [0] * rig.n and out == data

    def check_consequence(self, got, data):
        """the header's consequence: the new container is what compress and crc write for the resized data"""
        packed, first, off, crc = fresh(self.rig.ctx, self.big, data)
        nb = int(first[-1])
        assert (got["first"] == first).all() and (got["off"][: nb + 1] == off[: nb + 1]).all() and (got["off"][nb:] == off[nb]).all()
        assert bytes(got["image"][: len(packed)]) == packed
        assert got["crc"] is None or ((got["crc"][:nb] == crc[:nb]).all() and not got["crc"][nb:].any())

    def res_crc(self, d_first, d_len, d_crc):
        import torch
        rig = self.rig
        d_out = torch.full((rig.n,), 0x33333333, dtype=torch.int32, device=rig.dev)
        d_st = torch.full((rig.n,), ST_FILL, dtype=torch.int32, device=rig.dev)
        rig.m.res_crc_dev(rig.ctx, rig.B, rig.n, self.nbt, d_first, d_len, d_crc, d_out, d_st)
        rig.ctx.stream.synchronize()
        return [int(x) for x in d_out.cpu().numpy().view(np.uint32)], [int(x) for x in d_st.cpu().numpy()]

    def close(self):
        self.big.close()
        self.rig.close()


# ---- dedupers --------------------------------------------------------------------------------------------------------------------------------
DEDUP_EXACT = ("rep", "new_index", "pick", "count")             # every list of a dedup is compared whole


def dedup_outs(dev, n_max):
    """the five output arrays of a deduper made for n_max resources, sentinel-filled and guarded"""
    outs = ListOuts(dev, {"rep": n_max, "new_index": n_max, "pick": 2 * n_max, "count": 4}, n_max)
    outs.n_max = n_max
    return outs


def dedup_views(srcs, with_crc):
    return [s.view(crc=with_crc) for s in srcs]


def check_dedup(zs, srcs, with_crc=True, n_max=None, rows_max=None, deduper=None, outs=None):
    """one call compared with the model, entry for entry; returns (model, Outs)"""
    N, rows = sum(s.n for s in srcs), sum(s.nbt for s in srcs)
    n_max = N if n_max is None else n_max
    dd = deduper or zs.m.BlockDeduper(zs.ctx, zs.B, len(srcs), n_max, rows if rows_max is None else rows_max)
    outs = outs or dedup_outs(zs.dev, n_max)
    outs.reset()
    dd.dedup(dedup_views(srcs, with_crc), *outs.tensors())
    zs.ctx.stream.synchronize()
    if deduper is None:
        dd.close()
    mo = D.model_dedup([s.model() for s in srcs], zs.B, with_crc, n_res_total=n_max)
    assert len(mo["rep"]) == len(mo["new_index"]) == len(mo["status"]) == N and len(mo["pick"]) == 2 * n_max
    outs.against(mo, exact=DEDUP_EXACT)
    return mo, outs
