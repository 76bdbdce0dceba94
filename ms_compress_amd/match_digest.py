"""Block dedupers that match by block digest (include/mscomp_amd_match_digest.h): which blocks of a new container a set of stores already
holds, decided by data length and the 128-bit digest column a BlockDigester writes, no stored byte read -- a store may be known by its
tables and its column alone, and the containers of one call may be written by different codecs. A module of its own beside the binding of
include/mscomp_amd.h: SIGNATURES below is the table of the third header (tests/test_match_digest_abi.py holds it to that header), bind()
sets its entries on the library _abi.load_library() returns, BlockDigestMatcher is the thin wrapper over device tensors,
blocks_match_digest and blocks_match_digest_delta the host conveniences. Nothing here touches a device or imports torch at import time."""
import ctypes as C
import re

import numpy as np

from ._abi import _CODES, load_library
from ._core import _call, _run, _upload_containers
from .blocks import _blocks_views
from .blocks_host import _dev_block_digest, _extent_lists, blocks_splice_extents

# every function include/mscomp_amd_match_digest.h declares, in its order, in the codes of _abi._CODES
SIGNATURES = {
    "mscomp_amd_deduper_create_match_digest": "i:vuuzqquH",
    "mscomp_amd_deduper_match_digest":        "i:vBHBv8",
}
EXPORTS = list(SIGNATURES)


def signature(name):
    """(restype, argtypes) of an export of the match-digest header, as ctypes classes"""
    ret, _, args = SIGNATURES[name].partition(":")
    return _CODES[ret], [_CODES[c] for c, n in re.findall(r"(\D)(\d*)", args) for _ in range(int(n or 1))]


def bind(lib=None):
    """``lib`` (default: the loaded library) with every export of the match-digest header bound to its signature; one the library lacks is an error"""
    lib = load_library() if lib is None else lib
    for name in SIGNATURES:
        f = getattr(lib, name)
        f.restype, f.argtypes = signature(name)
    return lib


class BlockDigestMatcher:
    """A block deduper made for match by digest (mscomp_amd_deduper_create_match_digest): ``n_src`` (0 .. 3) stores and one new container of
    one ``block_size`` with at most ``n_res_total`` resources and ``n_blocks_total`` table rows in all of them together, the new container
    bringing at most ``n_blocks_new`` rows. All scratch is reserved here, by BlockDeduper.for_match's formula: 48 bytes per resource, 40
    per row, 4 per new row and 64 per SPLICE_ROW_TILE of them, + 848. match() enqueues ten kernels on the ctx stream and nothing else (legal
    inside a capture of that stream). Arguments are torch CUDA tensors: int64 / uint64 tables and lists, int32 digest words and statuses.
    The object lives in its context as the handle classes do (Context.close closes it) without being one of them."""

    def __init__(self, ctx, block_size, n_src, n_res_total, n_blocks_total, n_blocks_new):
        self.ctx, self._h = ctx, C.c_void_p()
        bind(ctx.lib)
        self.block_size, self.n_src, self.n_res_total = int(block_size), int(n_src), int(n_res_total)
        self.n_blocks_total, self.n_blocks_new = int(n_blocks_total), int(n_blocks_new)
        _run(ctx, "mscomp_amd_deduper_create_match_digest", ctx._h, self.block_size, self.n_src, self.n_res_total, self.n_blocks_total, self.n_blocks_new,
             0, C.byref(self._h))
        ctx._handles.add(self)

    def match(self, stores, store_digests, new, new_digest, d_delta_ext_first, d_delta_ext, d_patch_ext_first, d_patch_ext, d_class, d_count, d_status):
        """``stores``: n_src sources as BlockSplicer.splice takes them, ``new``: one more; a source's d_packed may be None with any
        packed_len -- no stored byte is read -- and its d_block_crc is ignored. ``store_digests``: per store its digest column, ``new_digest``
        the new container's: int32, four words per table row, as BlockDigester.blocks writes them (None only for a source without a
        resource). A block of ``new`` is found when a block of the same data length and the same digest lies anywhere in a store, shared
        when one lies earlier in ``new``, fresh otherwise. The seven outputs are BlockDeduper.match's, word for word: the delta extent
        lists over [new], the patch extent lists over stores + [the delta container] -- a container only between sources of one format,
        a read recipe otherwise --, d_class, d_count (6; the last: rows that share 64 bits of key with a smaller row that is not equal) and
        d_status."""
        if len(stores) != self.n_src or len(store_digests) != self.n_src:
            raise ValueError("one store and one digest column per n_src")
        views = _blocks_views(list(stores) + [new])
        cols = (C.c_void_p * max(1, self.n_src))(*[None if t is None else t.data_ptr() for t in store_digests])
        _run(self.ctx, "mscomp_amd_deduper_match_digest", self._h, views if self.n_src else None, cols if self.n_src else None, C.byref(views[self.n_src]),
             new_digest, d_delta_ext_first, d_delta_ext, d_patch_ext_first, d_patch_ext, d_class, d_count, d_status)

    def close(self):
        if self._h:
            self.ctx.lib.mscomp_amd_deduper_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _tables_only(con):
    """a container (packed or None, block_first, block_off, lengths, ...[, packed_len]) as _upload_containers takes one, without payload and
    without checksums, and the packed length it states: given, the length of its packed bytes, or what its offset table ends at"""
    packed, first, off, lens = con[:4]
    if len(con) > 5 and con[5] is not None:
        plen = int(con[5])
    elif packed is not None:
        plen = len(packed)
    else:
        end = int(np.asarray(first, dtype=np.uint64).reshape(-1)[len(lens)])
        off_h = np.asarray(off, dtype=np.uint64).reshape(-1)
        plen = int(off_h[end]) if end < len(off_h) else 0
    return (b"", first, off, lens, None), plen


def blocks_match_digest(stores, new, block_size, store_digests, new_digest, ctx=None):
    """blocks_match decided by digest (BlockDigestMatcher.match): ``stores`` (0 .. 3) and ``new`` are containers (packed, block_first,
    block_off, lengths, block_crc or None) of one ``block_size`` and of ANY formats; ``store_digests`` / ``new_digest`` their digest columns
    as blocks_digest returns them. No payload is uploaded, so a store may be given with packed=None: tables only, its packed length
    taken from a sixth entry of the tuple or else from the end of its offset table. Returns what blocks_match returns: host lists
    (delta_resources, patch_resources, classes, counts, statuses). blocks_splice_extents([new], delta_resources, block_size) is the delta
    container; between containers of one format blocks_match_patch rebuilds ``new``, across formats patch_resources is a read recipe of
    (source, resource, first block, count) extents."""
    B = int(block_size)
    if len(store_digests) != len(stores):
        raise ValueError("one digest column per store")
    cons, plens = zip(*[_tables_only(c) for c in list(stores) + [new]])
    with _call(ctx) as f:
        srcs, n_all, rows_all = _upload_containers(cons, f.dev, False)
        srcs = [(None,) + s[1:5] + (plen,) + s[6:] for s, plen in zip(srcs, plens)]
        d_dig = [_dev_block_digest(d, s[7], f.dev) for d, s in zip(list(store_digests) + [new_digest], srcs)]
        n, nbn = srcs[-1][6], srcs[-1][7]
        dd = f.make(BlockDigestMatcher, B, len(stores), n_all, rows_all, nbn)
        d_df, d_de, d_pf, d_pe = f.alloc(n + 1), f.alloc(4 * nbn), f.alloc(n + 1), f.alloc(4 * nbn)
        d_cl, d_cnt, d_st = f.alloc(3 * n), f.alloc(6), f.alloc(n_all, "int32")
        dd.match(srcs[:-1], d_dig[:-1], srcs[-1], d_dig[-1], d_df, d_de, d_pf, d_pe, d_cl, d_cnt, d_st)
        f.sync()
        delta, patch = _extent_lists(f.fetch(d_df), f.fetch(d_de), n), _extent_lists(f.fetch(d_pf), f.fetch(d_pe), n)
        classes = [tuple(int(x) for x in row) for row in f.fetch(d_cl, 3 * n).reshape(-1, 3)]
        counts, st = [int(x) for x in f.fetch(d_cnt)], [int(x) for x in f.fetch(d_st, n_all, signed=True)]
    return delta, patch, classes, counts, st


def blocks_match_digest_delta(stores, new, block_size, store_digests, new_digest, ctx=None):
    """The delta container of ``new`` against the ``stores`` by digest -- per resource the blocks no store holds and ``new`` has not held
    before, in order, in ``new``'s format -- together with the recipe over stores + [delta]: blocks_match_digest, then
    blocks_splice_extents over [new], whose payload this step needs. Returns (delta, patch_resources, classes, counts, statuses),
    delta = (packed, block_first, block_off, lengths, block_crc or None)."""
    with _call(ctx, enter=False) as f:
        delta_res, patch_res, classes, counts, st = blocks_match_digest(stores, new, block_size, store_digests, new_digest, ctx=f.ctx)
        packed, first, off, lens, crc, _ = blocks_splice_extents([tuple(new[:5])], delta_res, block_size, ctx=f.ctx)
    return (packed, first, off, lens, crc), patch_res, classes, counts, st
