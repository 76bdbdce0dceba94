"""Splice by block extents (include/mscomp_amd.h, mscomp_amd_splicer_splice_extents) restated over plain lists and bytes, beside
tests/splice_model.py: a new container whose resources are lists of extents (source, resource, first block, block count), with the
header's rules 0-9 in their order. Extents never encode or decode, so no oracle is called. Not collected as a test.

A source is splice_model's: (packed, packed_len, block_first, block_off, lengths, block_crc or None, n_res, n_blocks_table).
"""
import numpy as np

import blocks_model as M
import read_model as R

OK, ARG, DATA, BUF = M.OK, M.ARG, M.DATA, M.BUF
M64 = M.M64
END = M64                                                      # the block count "through the resource's last block"


def flat(resources):
    """(d_ext_first, d_ext rows) of a list -- one entry per new resource -- of lists of (s, r, k0, c), c = None for END"""
    ext_first, ext = [0], []
    for exts in resources:
        ext += [(s, r, k0, END if c is None else c) for s, r, k0, c in exts]
        ext_first.append(len(ext))
    return ext_first, ext


def extent_data(sources_bufs, resources, B):
    """the data an accepted extent list stands for: per new resource the concatenated blocks of its extents"""
    out = []
    for exts in resources:
        data = b""
        for s, r, k0, c in exts:
            buf = sources_bufs[s][r]
            data += buf[k0 * B:] if c is None or c == END else buf[k0 * B: (k0 + c) * B]
        out.append(data)
    return out


def model_splice_extents(sources, ext_first, ext, B, n_ext, n_blocks_table, new_cap, with_crc=True):
    """{"packed": the bytes written, "first" [n_res + 1], "off" [n_blocks_table + 1], "crc" [n_blocks_table] or None, "new_len", "status",
    "reached": the rules that decided something}"""
    n_res = len(ext_first) - 1
    ext_first = [int(x) & M64 for x in ext_first]
    reached = set()
    if any(ext_first[q] > ext_first[q + 1] for q in range(n_res)) or ext_first[n_res] > n_ext:      # rule 0
        reached.add(0)
        return {"packed": b"", "first": np.zeros(n_res + 1, dtype=np.uint64), "off": np.zeros(n_blocks_table + 1, dtype=np.uint64),
                "crc": np.zeros(n_blocks_table, dtype=np.uint32) if with_crc else None, "new_len": [0] * n_res, "status": [ARG] * n_res,
                "reached": reached}
    first, off, crc, new_len, status, pieces = [0], [0], [], [], [], []
    run = 0
    for q in range(n_res):
        judged = []                                            # per extent: (status, source, first source row, blocks, len_e)
        for e in range(ext_first[q], ext_first[q + 1]):
            s, r, k0, c = (int(x) & M64 for x in ext[e])
            if s >= len(sources) or r >= int(sources[s][6]):
                judged.append((ARG, 1)); continue
            _, _, sfirst, _, lens, _, _, snbt = sources[s]
            f0, f1, L = int(sfirst[r]), int(sfirst[r + 1]), int(lens[r])
            if f0 > f1 or f1 > int(snbt):
                judged.append((ARG, 1)); continue
            n = f1 - f0
            if n != L // B + (1 if L % B else 0):
                judged.append((DATA, 2)); continue
            if k0 > n or (c != END and c > n - k0):
                judged.append((ARG, 3)); continue
            cnt = n - k0 if c == END else c
            len_e = 0 if cnt == 0 else (L - k0 * B if k0 + cnt == n else cnt * B)
            judged.append((OK, 0, s, f0 + k0, cnt, len_e))
        nonempty = [i for i, x in enumerate(judged) if x[0] == OK and x[5] > 0]
        st = OK
        for i, x in enumerate(judged):                         # rules 4 and 5: the lowest-indexed refused extent decides
            if x[0] != OK:
                st = x[0]; reached.add(x[1]); reached.add(5); break
            if x[5] % B and i != nonempty[-1]:
                st = ARG; reached.add(4); reached.add(5); break
        rows, L = [], 0
        if st == OK:
            n_q = sum(x[4] for x in judged)
            run = min(run + n_q, M64)                          # rule 6: the total includes this resource, and the ones refused here
            if n_q and run > n_blocks_table:
                st = ARG; reached.add(6)
            else:
                L = sum(x[5] for x in judged)
                rows = [(x[2], x[3] + i) for x in judged for i in range(x[4])]
        if st != OK:
            reached.add(7)
        elif rows:
            reached.add(8)
        for s, j in rows:                                      # rule 8: verbatim, an unreadable entry as an empty row
            packed, plen, _, soff, _, scrc, _, _ = sources[s]
            o0, o1 = int(soff[j]), int(soff[j + 1])
            ok = o0 <= o1 <= plen
            off.append(off[-1] + (o1 - o0 if ok else 0))
            crc.append(int(scrc[j]) if with_crc else 0)
            if off[-1] <= new_cap:
                pieces.append(bytes(packed[o0:o1]) if ok else b"")
            elif st == OK:                                     # rule 9: capacity
                st = BUF
        first.append(len(off) - 1)
        new_len.append(L)
        status.append(st)
    nb = len(off) - 1
    reached.add(9)
    off += [off[-1]] * (n_blocks_table - nb)
    crc += [0] * (n_blocks_table - nb)
    return {"packed": b"".join(pieces), "first": np.array(first, dtype=np.uint64), "off": np.array(off, dtype=np.uint64),
            "crc": np.array(crc, dtype=np.uint32) if with_crc else None, "new_len": new_len, "status": status, "reached": reached}


# ---- the cases the CPU and the GPU tests share ----
ONE, BP1, MIXED, ZEROS5, TEXT, MIXED5 = 1, 4, 5, 6, 7, 9        # rows of R.RECIPES: 1 byte, B + 1, 3 B + 17, 5 B zeros, 3 B + 17, 5 B mixed
X3B, X3B5 = len(R.RECIPES), len(R.RECIPES) + 1                  # the two lengths R.RECIPES lacks: 3 B and 3 B + 5
EXTRA = [{"id": "text_3b", "kind": "text", "seed": 31, "mult": 3, "add": 0}, {"id": "mixed_3b5", "kind": "mixed", "seed": 32, "mult": 3, "add": 5}]


def buffers(B):
    """the resources of source 0: R.RECIPES (lengths 0, 1, B - 1, B, B + 1, 3 B + 17, 5 B) and the two extra ones; source 1 holds them reversed"""
    return R.buffers(B) + [M.build(r, B) for r in EXTRA]


def in1(r):
    return X3B5 - r                                            # resource r of source 0 is this resource of source 1


def source(oracle, f, B, bufs):
    total = sum(len(b) for b in bufs)
    packed, first, off, st = M.model_compress(oracle, f, bufs, B, total, total)
    assert not st.any()
    nbt = len(bufs) + total // B
    return (packed, len(packed), first, off, [len(b) for b in bufs], R.block_crcs(bufs, B, nbt), len(bufs), nbt)


def healthy_lists(n):
    """extent lists that every rule accepts, by name: each is a list of new resources"""
    return {
        "identity": [[(0, r, 0, None)] for r in range(n)],
        "join": [[(0, X3B, 0, None), (1, in1(X3B5), 0, None)]],
        "split": [[(0, X3B5, 0, 2)], [(0, X3B5, 2, None)]],
        "cut_middle": [[(0, X3B, 0, 1), (0, X3B, 2, None)]],
        "insert": [[(0, X3B5, 0, 1), (1, in1(MIXED5), 2, 1), (0, X3B5, 1, None)]],
        "duplicate": [[(0, X3B5, 1, 1), (0, X3B5, 1, 1), (1, in1(X3B5), 3, None)]],
        "empties": [[], [(0, X3B, 0, 0), (0, X3B, 3, None), (0, ONE, 0, None)], [(1, in1(X3B), 3, 0)], [(0, 0, 0, None)], []],
        "short_last": [[(0, X3B, 1, 2), (0, BP1, 0, None)], [(0, ZEROS5, 0, 2)], [(0, BP1, 0, None), (0, X3B, 0, 0)]],
    }
