"""The host conveniences of the block objects: every blocks_* call and res_crc_from_blocks take host bytes and tables, upload them, run one
object of blocks.py once inside the frame of _core._call and fetch the results as numpy arrays and lists. Tests and tools use them; no
timed path does. A wrapper over device tensors does not belong here, and neither does a step the frame already takes."""
import numpy as np

from ._abi import MSCOMP_AMD_BLOCK_SKIPPED, MSCOMP_AMD_DIFF_NO_BASE, MSCOMP_DATA_ERROR, MSCOMP_OK, MSCompError
from ._core import (_call, _covering_blocks, _dev_block_crc, _dev_packed, _dev_u64, _fetch_container, _new_container, _outputs, _upload_containers,
                    _upload_unit_tables, _upload_units, pack_offsets)
from .blocks import (BlockContainer, BlockDeduper, BlockDigester, BlockParity, BlockReader, BlockSplicer, BlockSyncer, BlockTranscoder, BlockWriter,
                     res_crc_dev)


def blocks_compress(fmt, buffers, block_size, ctx=None):
    """The block container of a list of byte strings (one resource each), built on the GPU. Returns numpy arrays (packed uint8, block_first
    uint64 of n + 1, block_off uint64 of nb + 1, statuses int32): block j of resource r is
    packed[block_off[block_first[r] + j] : block_off[block_first[r] + j + 1]], the bytes of ms_compress for that block when they are
    shorter than the block, the block itself otherwise."""
    n = len(buffers)
    with _call(ctx) as f:
        d_in, d_off, d_len, lens = _upload_unit_tables(buffers, f.dev)
        total = int(sum(lens))
        bk = f.make(BlockContainer, fmt, block_size, n, total)
        d_packed, d_first, d_boff, d_st = f.alloc(total + 16, "uint8"), f.alloc(n + 1), f.alloc(bk.n_blocks_max + 1), f.alloc(n, "int32")
        bk.compress(d_in, d_off, d_len, d_packed, d_first, d_boff, d_st, packed_cap=total)
        f.sync()
        first = f.fetch(d_first)
        nb = int(first[n])
        boff = f.fetch(d_boff, nb + 1)
        return f.fetch(d_packed, int(boff[nb])), first, boff, f.fetch(d_st, n, signed=True)


def blocks_crc(fmt, buffers, block_size, ctx=None):
    """The checksums a block container keeps beside a list of byte strings (one resource each), computed on the GPU. Returns numpy uint32
    arrays (block_crc of nb entries, in the block order of blocks_compress; res_crc of n): zlib's crc32 of every block and of every resource."""
    n = len(buffers)
    with _call(ctx) as f:
        d_in, d_off, d_len, lens = _upload_unit_tables(buffers, f.dev)
        bk = f.make(BlockContainer, fmt, block_size, n, int(sum(lens)))
        d_bcrc, d_rcrc, d_st = f.alloc(bk.n_blocks_max, "int32"), f.alloc(n, "int32"), f.alloc(n, "int32")
        bk.crc(d_in, d_off, d_len, d_bcrc, d_st, d_res_crc=d_rcrc)
        f.sync()
        nb = sum((x + block_size - 1) // block_size for x in lens)
        return f.fetch(d_bcrc, nb), f.fetch(d_rcrc, n)


def blocks_decompress(fmt, packed, block_first, block_off, lengths, block_size, ranges=None, ctx=None, block_crc=None):
    """Decode resources of a block container on the GPU: ``lengths`` are the resources' original lengths, ``ranges`` (optional) one
    (first block, count) pair per resource, clipped to its blocks; default: whole resources. ``block_crc`` (optional, as blocks_crc returns
    it): the decoded blocks are held to these checksums, and a resource with a mismatch gets MSCOMP_DATA_ERROR. Returns (list of bytes, or
    None where the status is not MSCOMP_OK; list of status)."""
    n = len(lengths)
    lens = [int(x) for x in lengths]
    total = int(sum(lens))
    out_off, out_total = pack_offsets(lens)
    with _call(ctx) as f:
        dev = f.dev
        bk = f.make(BlockContainer, fmt, block_size, n, total)
        packed, d_packed = _dev_packed(packed, dev)
        d_first, d_boff = _dev_u64(block_first, n + 1, dev), _dev_u64(block_off, bk.n_blocks_max + 1, dev)
        d_len, d_ooff, d_ocap = _dev_u64(lens, 1, dev), _dev_u64(out_off, 1, dev), _dev_u64(lens, 1, dev)
        d_range = None if ranges is None else _dev_u64(np.asarray(ranges, dtype=np.uint64), 2, dev)
        d_out, d_olen, d_st = f.alloc(out_total + 16, "uint8"), f.alloc(n), f.alloc(n, "int32")
        bk.decompress(d_packed, d_first, d_boff, d_len, d_out, d_ooff, d_ocap, d_olen, d_st, d_range=d_range, packed_len=len(packed))
        if block_crc is not None:
            bk.check(d_out, d_ooff, d_len, d_first, _dev_block_crc(block_crc, bk.n_blocks_max, dev), d_olen, d_st, d_range=d_range)
        f.sync()
        h_out, h_len, h_st = f.fetch(d_out), f.fetch(d_olen, n), f.fetch(d_st, n, signed=True)
    return _outputs(h_out, out_off, h_len, h_st == MSCOMP_OK), [int(x) for x in h_st]


def blocks_salvage(fmt, packed, block_first, block_off, lengths, block_size, ctx=None, block_crc=None, only=None):
    """Salvage a block container on the GPU (BlockContainer.salvage): every block that can be decoded is, and the others are named.
    ``block_crc`` (optional, as blocks_crc returns it) holds the decoded blocks to their checksums; ``only`` (optional: the verdicts of a
    copy of the same shape) leaves out the rows it marks MSCOMP_AMD_BLOCK_GOOD. Returns (buffers: bytes of the resource's length with
    zeros in the bad rows and in the rows left out, or None for a resource refused as a whole; verdicts: a numpy uint32 array with one
    entry per row of block_off; bad: list; statuses: list; counts: list of 4)."""
    n = len(lengths)
    lens = [int(x) for x in lengths]
    total = int(sum(lens))
    out_off, out_total = pack_offsets(lens)
    with _call(ctx) as f:
        dev = f.dev
        bk = f.make(BlockContainer, fmt, block_size, n, total)
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
            d_only = _dev_block_crc(h_only, len(h_only), dev)
        d_out, d_olen, d_cnt = f.alloc(out_total + 16, "uint8"), f.alloc(n), f.alloc(4)
        d_bad, d_st, d_ver = f.alloc(n, "int32"), f.alloc(n, "int32"), f.alloc(nbm, "int32", fill=MSCOMP_AMD_BLOCK_SKIPPED)
        bk.salvage(d_packed, d_first, d_boff, d_len, d_out, d_ooff, d_ocap, d_olen, d_bad, d_ver, d_cnt, d_st, d_block_crc=d_crc, d_only=d_only,
                   packed_len=len(packed))
        f.sync()
        h_out, h_len, h_st, h_bad = f.fetch(d_out), f.fetch(d_olen, n), f.fetch(d_st, n, signed=True), f.fetch(d_bad, n, signed=True)
        rows = max(0, len(np.asarray(block_off).reshape(-1)) - 1)          # (one verdict per row the caller's table has)
        ver = np.full(rows, MSCOMP_AMD_BLOCK_SKIPPED, dtype=np.uint32)
        ver[: min(rows, nbm)] = f.fetch(d_ver, min(rows, nbm))
        counts = [int(x) for x in f.fetch(d_cnt)]
    accepted = (h_st == MSCOMP_OK) | ((h_st == MSCOMP_DATA_ERROR) & (h_bad > 0))
    return _outputs(h_out, out_off, h_len, accepted), ver, [int(x) for x in h_bad], [int(x) for x in h_st], counts


def blocks_read(fmt, packed, block_first, block_off, lengths, block_size, requests, ctx=None, block_crc=None):
    """Read byte ranges of a block container on the GPU: ``requests`` is a list of (resource, offset, length), each clipped to its resource
    as pread does; ``lengths`` are the resources' original lengths. ``block_crc`` (optional, as blocks_crc returns it): every block read is
    held to its checksum. Returns (list of bytes, or None where the status is not MSCOMP_OK; list of status)."""
    n, nq = len(lengths), len(requests)
    lens = [int(x) for x in lengths]
    B = int(block_size)
    M64 = (1 << 64) - 1
    reqs = [(int(r) & M64, int(o) & M64, int(ln) & M64) for r, o, ln in requests]
    wants, blocks = _covering_blocks(reqs, lens, B)            # (the capacities, and the budget)
    out_off, out_total = pack_offsets(wants)
    nbt = max(0, len(np.asarray(block_off).reshape(-1)) - 1)
    with _call(ctx) as f:
        dev = f.dev
        rd = f.make(BlockReader, fmt, B, n, nbt, nq, blocks)
        packed, d_packed = _dev_packed(packed, dev)
        d_first, d_boff, d_len = _dev_u64(block_first, n + 1, dev), _dev_u64(block_off, nbt + 1, dev), _dev_u64(lens, 1, dev)
        d_req = _dev_u64(np.array(reqs, dtype=np.uint64), 3, dev)
        d_ooff, d_ocap = _dev_u64(out_off, 1, dev), _dev_u64(wants, 1, dev)
        d_crc = None if block_crc is None else _dev_block_crc(block_crc, nbt, dev)
        d_out, d_olen, d_st = f.alloc(out_total + 16, "uint8"), f.alloc(nq), f.alloc(nq, "int32")
        rd.read(d_packed, d_first, d_boff, d_len, d_req, d_out, d_ooff, d_ocap, d_olen, d_st, d_block_crc=d_crc, packed_len=len(packed))
        f.sync()
        h_out, h_len, h_st = f.fetch(d_out), f.fetch(d_olen, nq), f.fetch(d_st, nq, signed=True)
    return _outputs(h_out, out_off, h_len, h_st == MSCOMP_OK), [int(x) for x in h_st]


def blocks_write(fmt, packed, block_first, block_off, lengths, block_size, writes, ctx=None, block_crc=None):
    """Write byte ranges into a block container on the GPU: ``writes`` is a list of (resource, offset, bytes), each clipped to its resource
    (a write never changes a resource's length); ``lengths`` are the resources' original lengths; ``block_crc`` (optional, as blocks_crc
    returns it): every block touched is held to its checksum first, and the new container gets checksums too. Returns numpy arrays and
    lists (new_packed uint8, new_block_off uint64, new_block_crc uint32 or None, written, statuses, res_statuses): the new container
    shares block_first and lengths with the old one."""
    n, nq = len(lengths), len(writes)
    lens = [int(x) for x in lengths]
    B = int(block_size)
    M64 = (1 << 64) - 1
    reqs = [(int(r) & M64, int(o) & M64, len(b)) for r, o, b in writes]
    _, blocks = _covering_blocks(reqs, lens, B)                # (the budget)
    nbt = max(0, len(np.asarray(block_off).reshape(-1)) - 1)
    total = int(sum(lens))
    with _call(ctx) as f:
        dev = f.dev
        wr = f.make(BlockWriter, fmt, B, n, nbt, nq, blocks)
        packed, d_packed = _dev_packed(packed, dev)
        d_src, src_off, _ = _upload_units([b for _, _, b in writes], dev)
        d_first, d_boff, d_len = _dev_u64(block_first, n + 1, dev), _dev_u64(block_off, nbt + 1, dev), _dev_u64(lens, 1, dev)
        d_req, d_soff = _dev_u64(np.array(reqs, dtype=np.uint64), 3, dev), _dev_u64(src_off, 1, dev)
        d_crc = None if block_crc is None else _dev_block_crc(block_crc, nbt, dev)
        d_new, _, d_noff, d_ncrc = _new_container(dev, None, nbt, total, block_crc is not None)
        d_wr, d_st, d_rst = f.alloc(nq), f.alloc(nq, "int32"), f.alloc(n, "int32")
        wr.write(d_packed, d_first, d_boff, d_len, d_req, d_src, d_soff, d_new, d_noff, d_wr, d_st, d_rst, d_block_crc=d_crc, d_new_block_crc=d_ncrc,
                 packed_len=len(packed), new_cap=total)
        f.sync()
        new_packed, _, noff, ncrc = _fetch_container(d_new, None, d_noff, d_ncrc, total)
        h_wr, h_st, h_rst = f.fetch(d_wr, nq), f.fetch(d_st, nq, signed=True), f.fetch(d_rst, n, signed=True)
    return new_packed, noff, ncrc, [int(x) for x in h_wr], [int(x) for x in h_st], [int(x) for x in h_rst]


def blocks_resize(fmt, packed, block_first, block_off, lengths, block_size, new_lengths, ctx=None, block_crc=None):
    """Cut or zero-extend the resources of a block container to ``new_lengths`` on the GPU (BlockWriter.resize); ``lengths`` are their
    lengths now, ``block_crc`` as blocks_crc returns it (optional: the block a cut falls into is held to its checksum first, and the new
    container gets checksums too). Returns numpy arrays and lists (new_packed uint8, new_block_off uint64, new_block_crc uint32 or None,
    new_first uint64 of n + 1, new_lengths, res_statuses); the tables have as many rows as the resized container needs."""
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
    with _call(ctx) as f:
        dev = f.dev
        wr = f.make(BlockWriter, fmt, B, n, nbt, 0, budget)
        packed, d_packed = _dev_packed(packed, dev)
        d_first, d_boff, d_len, d_want = _dev_u64(block_first, n + 1, dev), _dev_u64(block_off, nbt + 1, dev), _dev_u64(lens, 1, dev), _dev_u64(want, 1, dev)
        d_crc = None if block_crc is None else _dev_block_crc(block_crc, nbt, dev)
        d_new, d_nfirst, d_noff, d_ncrc = _new_container(dev, n, nbt, room, block_crc is not None)
        d_nlen, d_rst = f.alloc(n), f.alloc(n, "int32")
        wr.resize(d_packed, d_first, d_boff, d_len, d_want, d_new, d_nfirst, d_noff, d_nlen, d_rst, d_block_crc=d_crc, d_new_block_crc=d_ncrc,
                  packed_len=len(packed), new_cap=room)
        f.sync()
        new_packed, nfirst, noff, ncrc = _fetch_container(d_new, d_nfirst, d_noff, d_ncrc, room)
        h_len, h_rst = f.fetch(d_nlen, n), f.fetch(d_rst, n, signed=True)
    return new_packed, noff, ncrc, nfirst, [int(x) for x in h_len], [int(x) for x in h_rst]


def _splice_host(containers, n_new, nbt, room, ctx, make, run):
    """what blocks_splice and blocks_splice_extents share: the sources uploaded, the new arrays made, ``run`` called, the results fetched"""
    with_crc = all(c[4] is not None for c in containers)
    with _call(ctx) as f:
        sp = f.make(make)
        srcs, _, _ = _upload_containers(containers, f.dev, with_crc)
        d_new, d_nfirst, d_noff, d_ncrc = _new_container(f.dev, n_new, nbt, room, with_crc)
        d_nlen, d_st = f.alloc(n_new), f.alloc(n_new, "int32")
        run(sp, srcs, f.dev, d_new, d_nfirst, d_noff, d_nlen, d_st, d_ncrc)
        f.sync()
        new_packed, nfirst, noff, ncrc = _fetch_container(d_new, d_nfirst, d_noff, d_ncrc, room)
        h_len, h_st = f.fetch(d_nlen, n_new), f.fetch(d_st, n_new, signed=True)
    return new_packed, nfirst, noff, [int(x) for x in h_len], ncrc, [int(x) for x in h_st]


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
    B = int(block_size)
    pr = _diff_pairs(base, new, pairs)
    n = len(pr)
    new_lens = [int(x) for x in new[3]]
    nbn = sum((new_lens[b] + B - 1) // B for _, b in pr if b < len(new_lens))
    with_crc = base[4] is not None and new[4] is not None
    with _call(ctx) as f:
        srcs, _, _ = _upload_containers((base, new), f.dev, with_crc)
        dd = f.make(BlockDeduper.for_diff, B, n, nbn)
        d_pair = _dev_u64(np.array(pr, dtype=np.uint64).reshape(-1), 2, f.dev)
        d_df, d_de, d_pf, d_pe = f.alloc(n + 1), f.alloc(4 * nbn), f.alloc(n + 1), f.alloc(4 * nbn)
        d_ch, d_cnt, d_st = f.alloc(n), f.alloc(4), f.alloc(n, "int32")
        dd.diff(srcs[0], srcs[1], d_pair, d_df, d_de, d_pf, d_pe, d_ch, d_cnt, d_st)
        f.sync()
        delta, patch = _extent_lists(f.fetch(d_df), f.fetch(d_de), n), _extent_lists(f.fetch(d_pf), f.fetch(d_pe), n)
        changed, counts, st = [int(x) for x in f.fetch(d_ch, n)], [int(x) for x in f.fetch(d_cnt)], [int(x) for x in f.fetch(d_st, n, signed=True)]
    return delta, patch, changed, counts, st


def blocks_delta(base, new, block_size, pairs=None, ctx=None):
    """The delta container of ``new`` against ``base`` -- per pair the changed blocks of the new resource, in order -- together with the
    recipe that rebuilds the new resources from base + delta: blocks_diff, then blocks_splice_extents over [new]. Returns (delta,
    patch_resources, changed, counts, statuses), delta = (packed, block_first, block_off, lengths, block_crc or None): a container as
    blocks_patch and blocks_splice take one."""
    with _call(ctx, enter=False) as f:
        delta_res, patch_res, changed, counts, st = blocks_diff(base, new, block_size, pairs=pairs, ctx=f.ctx)
        with_crc = base[4] is not None and new[4] is not None
        packed, first, off, lens, crc, _ = blocks_splice_extents([new if with_crc else tuple(new[:4]) + (None,)], delta_res, block_size, ctx=f.ctx)
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
    B = int(block_size)
    with_crc = all(c[4] is not None for c in containers)
    lens0 = [int(x) for x in containers[0][3]]
    n = len(lens0)
    nbn = sum((L + B - 1) // B for L in lens0)
    with _call(ctx, enter=False) as outer:                         # (three calls in one context: salvage, repair, splice)
        ctx, verdicts = outer.ctx, []
        for i, (packed, first, off, lens, crc) in enumerate(containers):
            same = i > 0 and [int(x) for x in lens] == lens0
            if i == 0 and _verdicts0 is not None:                   # (blocks_rebuild has salvaged the primary already)
                verdicts.append(_verdicts0)
                continue
            verdicts.append(blocks_salvage(fmt, packed, first, off, lens, B, ctx=ctx, block_crc=crc, only=verdicts[0] if same else None)[1])
        with _call(ctx) as f:
            srcs, _, _ = _upload_containers(containers, f.dev, with_crc)
            d_ver = [_dev_block_crc(v, len(v), f.dev) for v in verdicts]
            dd = f.make(BlockDeduper.for_repair, B, len(containers), n, nbn)
            d_ef, d_ext, d_fix, d_lost, d_cnt, d_st = f.alloc(n + 1), f.alloc(4 * nbn), f.alloc(n), f.alloc(n), f.alloc(4), f.alloc(n, "int32")
            dd.repair(srcs, d_ver, d_ef, d_ext, d_fix, d_lost, d_cnt, d_st)
            f.sync()
            resources = _extent_lists(f.fetch(d_ef), f.fetch(d_ext), n)
            report = {"verdicts": verdicts, "resources": resources, "fixed": [int(x) for x in f.fetch(d_fix, n)],
                      "lost": [int(x) for x in f.fetch(d_lost, n)], "counts": [int(x) for x in f.fetch(d_cnt)],
                      "statuses": [int(x) for x in f.fetch(d_st, n, signed=True)]}
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
    B = int(block_size)
    cons = list(stores) + [new]
    with_crc = all(c[4] is not None for c in cons)
    with _call(ctx) as f:
        srcs, n_all, rows_all = _upload_containers(cons, f.dev, with_crc)
        n, nbn = srcs[-1][6], srcs[-1][7]
        dd = f.make(BlockDeduper.for_match, B, len(stores), n_all, rows_all, nbn)
        d_df, d_de, d_pf, d_pe = f.alloc(n + 1), f.alloc(4 * nbn), f.alloc(n + 1), f.alloc(4 * nbn)
        d_cl, d_cnt, d_st = f.alloc(3 * n), f.alloc(6), f.alloc(n_all, "int32")
        dd.match(srcs[:-1], srcs[-1], d_df, d_de, d_pf, d_pe, d_cl, d_cnt, d_st)
        f.sync()
        delta, patch = _extent_lists(f.fetch(d_df), f.fetch(d_de), n), _extent_lists(f.fetch(d_pf), f.fetch(d_pe), n)
        classes = [tuple(int(x) for x in row) for row in f.fetch(d_cl, 3 * n).reshape(-1, 3)]
        counts, st = [int(x) for x in f.fetch(d_cnt)], [int(x) for x in f.fetch(d_st, n_all, signed=True)]
    return delta, patch, classes, counts, st


def blocks_match_delta(stores, new, block_size, ctx=None):
    """The delta container of ``new`` against the ``stores`` -- per resource the blocks no store holds and ``new`` has not held before, in
    order -- together with the recipe that rebuilds ``new`` from stores + delta: blocks_match, then blocks_splice_extents over [new].
    Returns (delta, patch_resources, classes, counts, statuses), delta = (packed, block_first, block_off, lengths, block_crc or None)."""
    with _call(ctx, enter=False) as f:
        delta_res, patch_res, classes, counts, st = blocks_match(stores, new, block_size, ctx=f.ctx)
        with_crc = all(c[4] is not None for c in list(stores) + [new])
        packed, first, off, lens, crc, _ = blocks_splice_extents([new if with_crc else tuple(new[:4]) + (None,)], delta_res, block_size, ctx=f.ctx)
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
    with_crc = all(c[4] is not None for c in containers)
    with _call(ctx) as f:
        srcs, n, rows_all = _upload_containers(containers, f.dev, with_crc)
        dd = f.make(BlockDeduper, block_size, len(containers), n, rows_all)
        d_rep, d_idx, d_pick, d_cnt, d_st = f.alloc(n), f.alloc(n), f.alloc(2 * n), f.alloc(4), f.alloc(n, "int32")
        dd.dedup(srcs, d_rep, d_idx, d_pick, d_cnt, d_st)
        f.sync()
        counts = [int(x) for x in f.fetch(d_cnt)]
        picks = f.fetch(d_pick, 2 * counts[0]).reshape(-1, 2)
        rep, idx, st = f.fetch(d_rep, n), f.fetch(d_idx, n), f.fetch(d_st, n, signed=True)
    return [int(x) for x in rep], [int(x) for x in idx], [(int(s), int(r)) for s, r in picks], counts, [int(x) for x in st]


def blocks_transcode(container, block_size, new_block_size, new_fmt=None, ctx=None, groups_max=None, n_blocks_new=None, new_cap=None):
    """Bring a block container to another block size and / or codec on the GPU (BlockTranscoder). ``container`` is (fmt, packed,
    block_first, block_off, lengths, block_crc or None) as blocks_compress and blocks_crc return them; ``new_fmt`` defaults to fmt. The new
    container gets checksums exactly when the old one has them. ``groups_max`` (default: every group of the container), ``n_blocks_new``
    (default: what the lengths need) and ``new_cap`` (default: the sum of the lengths) are the transcoder's bounds. Returns numpy arrays
    and lists (new_packed uint8, new_block_first uint64 of n + 1, new_block_off uint64, new_block_crc uint32 or None, statuses, counts)."""
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
    with _call(ctx) as f:
        dev = f.dev
        tc = f.make(BlockTranscoder, fmt, B1, new_fmt, B2, n, nbt, nbn, gmax)
        packed, d_packed = _dev_packed(packed, dev)
        d_first, d_boff, d_len = _dev_u64(block_first, n + 1, dev), _dev_u64(block_off, nbt + 1, dev), _dev_u64(lens, 1, dev)
        d_crc = None if block_crc is None else _dev_block_crc(block_crc, nbt, dev)
        d_new, d_nfirst, d_noff, d_ncrc = _new_container(dev, n, nbn, room, block_crc is not None)
        d_st = f.alloc(n, "int32")
        tc.transcode(d_packed, d_first, d_boff, d_len, d_new, d_nfirst, d_noff, d_st, d_block_crc=d_crc, d_new_block_crc=d_ncrc,
                     packed_len=len(packed), new_cap=room)
        counts = tc.counts()                                     # (synchronizes the stream)
        new_packed, nfirst, noff, ncrc = _fetch_container(d_new, d_nfirst, d_noff, d_ncrc, room)
        h_st = f.fetch(d_st, n, signed=True)
    return new_packed, nfirst, noff, ncrc, [int(x) for x in h_st], counts


def blocks_digest(buffers, block_size, ctx=None):
    """The digest column of a list of byte strings (one resource each), computed on the GPU (BlockDigester): a numpy uint32 array of
    shape (nb, 4) in the block order of blocks_compress; row j viewed as bytes is the BLAKE2s tree digest of block j."""
    n = len(buffers)
    with _call(ctx) as f:
        d_in, d_off, d_len, lens = _upload_unit_tables(buffers, f.dev)
        dg = f.make(BlockDigester, block_size, n, int(sum(lens)))
        d_dig, d_st = f.alloc(4 * dg.n_blocks_max, "int32"), f.alloc(n, "int32")
        dg.blocks(d_in, d_off, d_len, d_dig, d_st)
        f.sync()
        nb = sum((x + block_size - 1) // block_size for x in lens)
        return f.fetch(d_dig, 4 * nb).reshape(nb, 4)


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
    if fmt is None and block_digest is None:
        raise ValueError("fmt: the format the store was written in (its blocks are decoded)")
    B = int(block_size)
    bufs = [bytes(b) for b in buffers]
    nu, total = len(bufs), sum(len(b) for b in bufs)
    nc = 2 * (total // B) + 8 * nu if n_cand_max is None else int(n_cand_max)
    with _call(ctx) as f:
        dev = f.dev
        srcs, n, rows = _upload_containers([store], dev, True)
        d_in, in_off, lens = _upload_units(bufs, dev)
        d_off, d_len = _dev_u64(in_off, 1, dev), _dev_u64(lens, 1, dev)
        sy = f.make(BlockSyncer, fmt, B, n, rows, nu, total, nc) if block_digest is None else f.make(BlockSyncer.for_digest, B, n, rows, nu, total, nc)
        d_hf, d_req, d_roff, d_lf, d_lit, d_cnt = f.alloc(nu + 1), f.alloc(3 * nc), f.alloc(nc), f.alloc(nu + 1), f.alloc(2 * (nc + nu)), f.alloc(8)
        d_rst, d_st = f.alloc(n, "int32"), f.alloc(nu, "int32")
        if block_digest is None:
            sy.sync(srcs[0], d_in, d_off, d_len, d_hf, d_req, d_roff, d_lf, d_lit, d_cnt, d_rst, d_st)
        else:
            sy.sync_digest(srcs[0], _dev_block_digest(block_digest, rows, dev), d_in, d_off, d_len, d_hf, d_req, d_roff, d_lf, d_lit, d_cnt, d_rst, d_st)
        f.sync()
        hf, req, roff, lf, lit, cnt = [f.fetch(t) for t in (d_hf, d_req, d_roff, d_lf, d_lit, d_cnt)]
        rst, st = [int(x) for x in f.fetch(d_rst, n, signed=True)], [int(x) for x in f.fetch(d_st, nu, signed=True)]
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


def blocks_parity(container, block_size, k, m, ctx=None):
    """The parity set of ``container`` = (packed, block_first, block_off, lengths, ...) on the GPU (BlockParity.build): (par, par_off,
    par_crc, row_len, head) as numpy arrays -- par (uint8) cut to its length par_off[-1], par_off (uint64, m G + 1), par_crc (uint32,
    m G), row_len (uint32, one per table row), head (uint64: nb, G, k, m). Keep it beside the container; blocks_rebuild takes it."""
    packed, first, off, lens = container[:4]
    with _call(ctx) as f:
        srcs, _, nbt = _upload_containers([(packed, first, off, lens, None)], f.dev, False)
        pr = f.make(BlockParity, block_size, nbt, k, m)
        rows, room = pr.bound()
        d_par, d_off, d_crc = f.alloc(room + 16, "uint8"), f.alloc(rows + 1), f.alloc(rows, "int32")
        d_rl, d_head, d_st = f.alloc(nbt, "int32"), f.alloc(4), f.alloc(1, "int32")
        pr.build(srcs[0], d_par, d_off, d_crc, d_rl, d_head, d_st, par_cap=room)
        f.sync()
        status = int(f.fetch(d_st, signed=True)[0])             # (the status build wrote on the device)
        if status != MSCOMP_OK:
            raise MSCompError(status, "mscomp_amd_parity_build")
        par_off = f.fetch(d_off)
        return f.fetch(d_par, int(par_off[-1])), par_off, f.fetch(d_crc, rows), f.fetch(d_rl, nbt), f.fetch(d_head)


def blocks_rebuild(fmt, container, parity, block_size, ctx=None, mirrors=()):
    """Mend a damaged block container from its parity set on the GPU, without a second copy: ``container`` = (packed, block_first,
    block_off, lengths, block_crc or None), ``parity`` as blocks_parity returned it. The container is salvaged (blocks_salvage),
    BlockParity.rebuild writes the sparse mirror of the rows it can give back, and blocks_repair over [container, mirror, *mirrors] --
    which salvages the mirror in the rows the container lacks, holding every rebuilt row to its CRC-32 -- and blocks_splice_extents
    build the container. ``mirrors``: up to two real copies, asked only for what parity could not give. Returns (container, report):
    blocks_repair's, plus "rebuild_counts" (rows missing, rows rebuilt, groups with a missing row, groups unrecoverable, parity rows
    unusable, stored bytes rebuilt) and "rebuild_status"."""
    B = int(block_size)
    packed, first, off, lens, crc = container
    par, par_off, par_crc, row_len, head = parity
    k, m = int(head[2]), int(head[3])
    with _call(ctx, enter=False) as outer:                         # (three calls in one context: salvage, rebuild, repair)
        ctx = outer.ctx
        ver0 = blocks_salvage(fmt, packed, first, off, lens, B, ctx=ctx, block_crc=crc)[1]
        with _call(ctx) as f:
            dev = f.dev
            srcs, _, nbt = _upload_containers([(packed, first, off, lens, None)], dev, False)
            pr = f.make(BlockParity, B, nbt, k, m)
            rows = pr.bound()[0]
            par, d_par = _dev_packed(par, dev)
            d_poff, d_pcrc, d_rl = _dev_u64(par_off, rows + 1, dev), _dev_block_crc(par_crc, rows, dev), _dev_block_crc(row_len, nbt, dev)
            d_head, d_ver = _dev_u64(head, 4, dev), _dev_block_crc(ver0, nbt, dev)
            room = int(np.asarray(row_len, dtype=np.uint64).sum())
            d_fix, d_foff, d_fver = f.alloc(room + 16, "uint8"), f.alloc(nbt + 1), f.alloc(nbt, "int32", fill=MSCOMP_AMD_BLOCK_SKIPPED)
            d_cnt, d_st = f.alloc(6), f.alloc(1, "int32")
            pr.rebuild(srcs[0], d_ver, d_par, d_poff, d_pcrc, d_rl, d_head, d_fix, d_foff, d_fver, d_cnt, d_st, par_len=len(par), fix_cap=room)
            f.sync()
            fix_off = f.fetch(d_foff)
            fix = (f.fetch(d_fix, int(fix_off[-1])), first, fix_off, lens, crc)
            counts, status = [int(x) for x in f.fetch(d_cnt)], int(f.fetch(d_st, signed=True)[0])
        new, report = blocks_repair(fmt, [container, fix] + list(mirrors), B, ctx=ctx, _verdicts0=ver0)
    report["rebuild_counts"], report["rebuild_status"] = counts, status
    return new, report


def res_crc_from_blocks(block_first, lengths, block_crc, block_size, ctx=None):
    """zlib's crc32 of every whole resource of a block container from its block checksums alone (mscomp_amd_res_crc_dev): no data is read.
    Returns (numpy uint32 array of n, list of status)."""
    n = len(lengths)
    nbt = len(np.asarray(block_crc).reshape(-1))
    with _call(ctx) as f:
        d_first, d_len = _dev_u64(block_first, n + 1, f.dev), _dev_u64([int(x) for x in lengths], 1, f.dev)
        d_bcrc, d_rcrc, d_st = _dev_block_crc(block_crc, nbt, f.dev), f.alloc(n, "int32"), f.alloc(n, "int32")
        res_crc_dev(f.ctx, block_size, n, nbt, d_first, d_len, d_bcrc, d_rcrc, d_st)
        f.sync()
        return f.fetch(d_rcrc, n), [int(x) for x in f.fetch(d_st, n, signed=True)]
