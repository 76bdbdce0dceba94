"""Block searchers (include/mscomp_amd_search.h): batched byte-pattern search in a block container. A module of its own beside the
binding of include/mscomp_amd.h: SIGNATURES below is the table of the second header (tests/test_search_abi.py holds it to that header),
bind() sets its entries on the library _abi.load_library() returns, BlockSearcher is the thin wrapper over device tensors and
blocks_search the host convenience. Nothing here touches a device or imports torch at import time."""
import ctypes as C
import re

import numpy as np

from ._abi import _CODES, MSCOMP_ARG_ERROR, MSCOMP_OK, load_library
from ._core import _byte_bounds, _call, _dev_block_crc, _dev_packed, _dev_u64, _run, _three_counts

MSCOMP_AMD_SEARCH_PAT_MAX = 64                                 # patterns per searcher
MSCOMP_AMD_SEARCH_LEN_MAX = 256                                # bytes per pattern

# every function include/mscomp_amd_search.h declares, in its order, in the codes of _abi._CODES
SIGNATURES = {
    "mscomp_amd_searcher_create":  "i:viuzqzquuquH",
    "mscomp_amd_searcher_destroy": "-:v",
    "mscomp_amd_searcher_search":  "i:vvqv12",
    "mscomp_amd_searcher_counts":  "i:vU",
}
EXPORTS = list(SIGNATURES)


def signature(name):
    """(restype, argtypes) of an export of the search header, as ctypes classes"""
    ret, _, args = SIGNATURES[name].partition(":")
    return _CODES[ret], [_CODES[c] for c, n in re.findall(r"(\D)(\d*)", args) for _ in range(int(n or 1))]


def bind(lib=None):
    """``lib`` (default: the loaded library) with every export of the search header bound to its signature; one the library lacks is an error"""
    lib = load_library() if lib is None else lib
    for name in SIGNATURES:
        f = getattr(lib, name)
        f.restype, f.argtypes = signature(name)
    return lib


class BlockSearcher:
    """A block searcher (mscomp_amd_searcher_create): where up to ``n_pat`` byte patterns of at most ``len_max`` bytes occur in byte ranges
    of a block container, by its tables alone. Made once for ``n_req`` requests per call that together cover at most ``blocks_max`` blocks,
    look-ahead included (counted per request, before any sharing), against the tables of a container of ``n_res`` resources whose
    d_block_off has ``n_blocks_table`` + 1 entries; d_hits has room for ``hits_max`` records. All scratch is reserved here: what a
    BlockReader of the same bounds reserves, 8 KiB of pattern tables and 8 bytes per 4096 bytes of blocks_max blocks. search() enqueues
    kernels on the ctx stream and nothing else (legal inside a capture of that stream). Arguments are torch CUDA tensors: uint8 data and
    patterns, int64 / uint64 tables, records and counts, int32 statuses and checksums. The object lives in its context as the handle
    classes do (Context.close closes it) without being one of them."""

    def __init__(self, ctx, fmt, block_size, n_res, n_blocks_table, n_req, blocks_max, n_pat, len_max, hits_max):
        self.ctx, self._h = ctx, C.c_void_p()
        bind(ctx.lib)
        self.fmt, self.block_size = int(fmt), int(block_size)
        self.n_res, self.n_blocks_table, self.n_req, self.blocks_max = int(n_res), int(n_blocks_table), int(n_req), int(blocks_max)
        self.n_pat, self.len_max, self.hits_max = int(n_pat), int(len_max), int(hits_max)
        _run(ctx, "mscomp_amd_searcher_create", ctx._h, self.fmt, self.block_size, self.n_res, self.n_blocks_table, self.n_req, self.blocks_max,
             self.n_pat, self.len_max, self.hits_max, 0, C.byref(self._h))
        ctx._handles.add(self)

    def search(self, d_packed, packed_len, d_block_first, d_block_off, d_res_len, d_block_crc, d_req, d_pat, d_pat_off, d_hits, d_req_hits, d_count,
               d_pat_status, d_status):
        """Request q = (resource, offset, length) = d_req[3 q .. 3 q + 2], clipped as BlockReader.read clips it; pattern p = the bytes
        d_pat[d_pat_off[p] .. d_pat_off[p + 1]). Writes d_pat_status[p] (MSCOMP_OK, or MSCOMP_ARG_ERROR for a pattern that is empty, longer
        than len_max or has offsets running backwards: it never hits), d_status[q] (as the reader's, without the capacity rule and with the
        look-ahead's blocks in the budget), d_req_hits[q] and d_count[0] (exact), and d_count[1] = min(d_count[0], hits_max) records
        d_hits[2 i] = position, d_hits[2 i + 1] = q << 32 | p in ascending (q, position, p) order. ``packed_len``: the valid bytes of
        d_packed (None: all of it); ``d_block_crc`` may be None."""
        plen, _ = _byte_bounds(d_packed, packed_len)
        _run(self.ctx, "mscomp_amd_searcher_search", self._h, d_packed, plen, d_block_first, d_block_off, d_res_len, d_block_crc, d_req, d_pat, d_pat_off,
             d_hits, d_req_hits, d_count, d_pat_status, d_status)

    def counts(self):
        """(units, distinct blocks, blocks decoded rather than raw) of the last search(); synchronizes the stream."""
        return _three_counts(self, "mscomp_amd_searcher_counts")

    def close(self):
        if self._h:
            self.ctx.lib.mscomp_amd_searcher_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _pieces(ranges, lens, B, span):
    """the ranges clipped to their resources and cut at block boundaries into requests of at most ``span`` blocks each: a list of
    (range index, resource, offset, length); a range of a resource that does not exist stays one request, for the device to refuse"""
    out = []
    for i, (r, o, ln) in enumerate(ranges):
        if not 0 <= r < len(lens):
            out.append((i, r, o, ln))
            continue
        o = min(o, lens[r])
        end = o + min(ln, lens[r] - o)
        while o < end:
            cut = min(end, (o // B + span) * B)
            out.append((i, r, o, cut - o))
            o = cut
    return out


def blocks_search(fmt, packed, block_first, block_off, lengths, block_size, patterns, ranges=None, block_crc=None, ctx=None, blocks_max=None, hits_max=None):
    """Search a block container on the GPU for the byte strings ``patterns`` (at most 64): in the (resource, offset, length) ``ranges``,
    each clipped to its resource -- default: every whole resource. The ranges are cut into requests that fit ``blocks_max`` blocks per call
    (default: 256; 2 at least), as many calls are run as that takes, and a call whose records did not fit ``hits_max`` (default: 4096) is
    repeated with the room its exact count asks for. ``block_crc`` (optional, as blocks_crc returns it): every block read is held to its
    checksum. Returns (hits: (resource, position, pattern) triples in ascending order, those of a range that is not MSCOMP_OK left out;
    statuses: one per range, the first that is not MSCOMP_OK among its requests; pattern statuses: MSCOMP_ARG_ERROR for a pattern that
    is empty or longer than 256 bytes, which never hits)."""
    M64 = (1 << 64) - 1
    n, B = len(lengths), int(block_size)
    lens = [int(x) for x in lengths]
    pats = [bytes(p) for p in patterns]
    if not 1 <= len(pats) <= MSCOMP_AMD_SEARCH_PAT_MAX:
        raise ValueError("1 to %d patterns" % MSCOMP_AMD_SEARCH_PAT_MAX)
    len_max = max(1, min(MSCOMP_AMD_SEARCH_LEN_MAX, max(len(p) for p in pats)))
    budget = 256 if blocks_max is None else int(blocks_max)
    if budget < 2:
        raise ValueError("blocks_max: a request needs its block and the look-ahead's")
    ranges = [(r, 0, lens[r]) for r in range(n)] if ranges is None else [(int(r), int(o) & M64, int(ln) & M64) for r, o, ln in ranges]
    pieces = _pieces(ranges, lens, B, budget - 1)
    calls, used = [[]], 0                                        # every piece covers at most budget blocks with its look-ahead
    for pc in pieces:
        r, o, ln = pc[1:]
        cnt = ((min(lens[r], o + ln + len_max - 1) - 1) // B - o // B + 1) if 0 <= r < n and ln else 0
        if used + cnt > budget:
            calls.append([])
            used = 0
        calls[-1].append(pc)
        used += cnt
    pat_status = [MSCOMP_OK if 1 <= len(p) <= len_max else MSCOMP_ARG_ERROR for p in pats]
    status, hits = [MSCOMP_OK] * len(ranges), []
    if not pieces:
        return hits, status, pat_status
    nq = max(len(c) for c in calls)
    nbt = max(0, len(np.asarray(block_off).reshape(-1)) - 1)
    room = 4096 if hits_max is None else int(hits_max)
    with _call(ctx) as f:
        dev = f.dev
        packed, d_packed = _dev_packed(packed, dev)
        d_first, d_boff, d_len = _dev_u64(block_first, n + 1, dev), _dev_u64(block_off, nbt + 1, dev), _dev_u64(lens, 1, dev)
        d_crc = None if block_crc is None else _dev_block_crc(block_crc, nbt, dev)
        _, d_pat = _dev_packed(b"".join(pats), dev)
        d_poff = _dev_u64(np.cumsum([0] + [len(p) for p in pats]), len(pats) + 1, dev)
        d_rh, d_cnt, d_pst, d_st = f.alloc(nq), f.alloc(2), f.alloc(len(pats), "int32"), f.alloc(nq, "int32")
        made = {}
        for reqs in calls:
            rows = [(r & M64, o, ln) for _, r, o, ln in reqs] + [(0, 0, 0)] * (nq - len(reqs))     # (the padding asks for nothing)
            d_req = _dev_u64(np.array(rows, dtype=np.uint64), 3, dev)
            while True:
                if room not in made:
                    made[room] = (f.make(BlockSearcher, fmt, B, n, nbt, nq, budget, len(pats), len_max, room), f.alloc(2 * room))
                sr, d_hits = made[room]
                sr.search(d_packed, len(packed), d_first, d_boff, d_len, d_crc, d_req, d_pat, d_poff, d_hits, d_rh, d_cnt, d_pst, d_st)
                f.sync()
                total, written = (int(x) for x in f.fetch(d_cnt, 2))
                if total == written:
                    break
                room = total                                       # (exact: the next run of this call fits)
            h, st = f.fetch(d_hits, 2 * written), f.fetch(d_st, len(reqs), signed=True)
            pat_status = [int(x) for x in f.fetch(d_pst, len(pats), signed=True)]
            for q, (i, r, _, _) in enumerate(reqs):
                if st[q] != MSCOMP_OK and status[i] == MSCOMP_OK:
                    status[i] = int(st[q])
            hits += [(reqs[int(w) >> 32][0], reqs[int(w) >> 32][1], int(x), int(w) & 0xFFFFFFFF) for x, w in zip(h[0::2], h[1::2])]
    return sorted((r, x, p) for i, r, x, p in hits if status[i] == MSCOMP_OK), status, pat_status
