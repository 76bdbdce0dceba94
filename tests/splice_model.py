"""The block splicer (include/mscomp_amd.h, mscomp_amd_splicer_*) restated over plain lists and bytes: a new container made of picks
(source, resource) out of source containers, with the header's rules 1-7 in their order. Splice never encodes or decodes, so no oracle is
called. Not collected as a test.

A source is (packed, packed_len, block_first, block_off, lengths, block_crc or None, n_res, n_blocks_table).
"""
import numpy as np

import blocks_model as M
import read_model as R
import write_model as W

OK, ARG, DATA, BUF = M.OK, M.ARG, M.DATA, M.BUF
M64 = M.M64


def picked(sources_bufs, picks):
    """the data a pick list stands for: the buffers of the picked resources, in pick order"""
    return [sources_bufs[s][r] for s, r in picks]


def model_splice(sources, picks, B, n_blocks_table, new_cap, with_crc=True):
    """{"packed": the bytes written, "first" [n_pick + 1], "off" [n_blocks_table + 1], "crc" [n_blocks_table] or None, "new_len", "status",
    "reached": the rules that decided something}"""
    first, off, crc, new_len, status, pieces, reached = [0], [0], [], [], [], [], set()
    run = 0
    for s, r in picks:
        s, r = int(s) & M64, int(r) & M64
        st, L, rows = OK, 0, []
        if s >= len(sources) or r >= int(sources[s][6]):
            st = ARG
            reached.add(1)
        else:
            packed, plen, sfirst, soff, lens, scrc, _, snbt = sources[s]
            f0, f1 = int(sfirst[r]), int(sfirst[r + 1])
            if f0 > f1 or f1 > int(snbt):
                st = ARG
                reached.add(1)
            elif f1 - f0 != int(lens[r]) // B + (1 if int(lens[r]) % B else 0):
                st = DATA
                reached.add(2)
            else:
                run = min(run + (f1 - f0), M64)                # rule 3: the total includes this pick, and the picks it refuses
                if f1 > f0 and run > n_blocks_table:
                    st = ARG
                    reached.add(3)
                else:
                    L, rows = int(lens[r]), list(range(f0, f1))
        if st != OK:
            reached.add(4)
        for j in rows:                                         # rule 5: verbatim, an unreadable entry as an empty one
            o0, o1 = int(soff[j]), int(soff[j + 1])
            ok = o0 <= o1 <= plen
            if not ok:
                reached.add(5)
            off.append(off[-1] + (o1 - o0 if ok else 0))
            crc.append(int(scrc[j]) if with_crc else 0)
            if off[-1] <= new_cap:
                pieces.append(bytes(packed[o0:o1]) if ok else b"")
            elif st == OK:                                     # rule 7
                st = BUF
                reached.add(7)
        first.append(len(off) - 1)
        new_len.append(L)
        status.append(st)
    nb = len(off) - 1
    reached.add(6)
    off += [off[-1]] * (n_blocks_table - nb)
    crc += [0] * (n_blocks_table - nb)
    return {"packed": b"".join(pieces), "first": np.array(first, dtype=np.uint64), "off": np.array(off, dtype=np.uint64),
            "crc": np.array(crc, dtype=np.uint32) if with_crc else None, "new_len": new_len, "status": status, "reached": reached}


# ---- the cases the CPU and the GPU tests share ----
MIXED = 5                                                      # row of R.RECIPES: 3 B + 17, raw and compressed blocks
ORDER2 = [7, 0, 9, 3, 5, 11, 1, 6, 10, 2, 8, 4]                  # the second container holds the same buffers in this order


def source(oracle, f, B, order=None):
    """(buffers, source tuple of splice_model) of R.RECIPES, in ``order``, as the container model compresses and checksums them"""
    if order is None:
        bufs, packed, first, off, nbt, crc = W.container(oracle, f, B)
    else:
        bufs = [R.buffers(B)[i] for i in order]
        total = sum(len(b) for b in bufs)
        packed, first, off, st = M.model_compress(oracle, f, bufs, B, total, total)
        assert not st.any()
        nbt = len(bufs) + total // B
        crc = R.block_crcs(bufs, B, nbt)
    return bufs, (packed, len(packed), first, off, [len(b) for b in bufs], crc, len(bufs), nbt)


def pick_lists(n):
    """identity; a permutation with a deletion and a duplicate; an interleaved merge of two containers"""
    perm = [(0, r) for r in (9, 2, 7, 7, 0, 11, 5, 3, 10, 1, 8, 4)]          # without 6, with 7 twice
    merge = [((k + 1) % 2, ORDER2.index(k) if (k + 1) % 2 else k) for k in range(n)] + [(1, 0), (0, MIXED)]
    return [(0, r) for r in range(n)], perm, merge


def expect(oracle, f, B, data, nbt):
    """the consequence: (packed, first, off [nbt + 1], crc [nbt]) of the container model over ``data``"""
    total = sum(len(b) for b in data)
    packed, first, off, st = M.model_compress(oracle, f, data, B, total, total)
    nb = int(first[-1])
    assert not st.any() and nb <= nbt
    off = np.concatenate([off[: nb + 1], np.full(max(0, nbt - nb), off[nb], dtype=np.uint64)])[: nbt + 1]
    return packed, first, off, R.block_crcs(data, B, nbt)
