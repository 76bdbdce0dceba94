"""The block objects of the library -- container, reader, writer, splicer, deduper, transcoder, syncer, digester, parity -- as thin
wrappers: every method passes its torch CUDA tensors straight through _run in the header's parameter order (tests/test_binding.py holds
them to it), enqueues on the context's stream and reads nothing back. Nothing here takes host bytes: that is blocks_host.py."""
import ctypes as C

from ._abi import BlocksView
from ._core import _byte_bounds, _Handle, _run, _three_counts


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


def res_crc_dev(ctx, block_size, n_res, n_blocks_table, d_block_first, d_res_len, d_block_crc, d_res_crc, d_status):
    """mscomp_amd_res_crc_dev on torch CUDA tensors: d_res_crc[r] (int32) = the CRC-32 of resource r from d_block_crc, d_status[r] MSCOMP_OK,
    MSCOMP_ARG_ERROR (a table entry beyond n_blocks_table) or MSCOMP_DATA_ERROR (a wrong block count). Kernels on the ctx stream only."""
    _run(ctx, "mscomp_amd_res_crc_dev", ctx._h, int(block_size), int(n_res), int(n_blocks_table), d_block_first, d_res_len, d_block_crc, d_res_crc, d_status)
