"""The block reader (include/mscomp_amd.h, mscomp_amd_reader_*) restated over tests/blocks_model.py: batched byte-range requests against a
container's tables, with the header's six rules in their order. Not collected as a test.

RECIPES are the resources the reader's tests read from (blocks_model.build recipes): the lengths 0, 1, B - 1, B, B + 1, 3 B + 17 and 5 B in the
kinds zeros, text, random and mixed, so that raw and compressed blocks sit side by side, in one resource too.
"""
import zlib

import numpy as np

import blocks_model as M

OK, ARG, DATA, BUF = M.OK, M.ARG, M.DATA, M.BUF
M64 = M.M64
RECIPES = [
    {"id": "empty", "kind": "zeros", "seed": 1, "mult": 0, "add": 0},
    {"id": "one", "kind": "random", "seed": 2, "mult": 0, "add": 1},
    {"id": "short_text", "kind": "text", "seed": 3, "mult": 1, "add": -1},
    {"id": "one_block_random", "kind": "random", "seed": 4, "mult": 1, "add": 0},
    {"id": "block_and_one", "kind": "text", "seed": 5, "mult": 1, "add": 1},
    {"id": "mixed_3b17", "kind": "mixed", "seed": 6, "mult": 3, "add": 17},
    {"id": "zeros_5b", "kind": "zeros", "seed": 7, "mult": 5, "add": 0},
    {"id": "text_3b17", "kind": "text", "seed": 8, "mult": 3, "add": 17},
    {"id": "random_3b17", "kind": "random", "seed": 9, "mult": 3, "add": 17},
    {"id": "mixed_5b", "kind": "mixed", "seed": 10, "mult": 5, "add": 0},
    {"id": "one_block_zeros", "kind": "zeros", "seed": 11, "mult": 1, "add": 0},
    {"id": "empty_again", "kind": "text", "seed": 12, "mult": 0, "add": 0},
]


def buffers(B):
    return [M.build(r, B) for r in RECIPES]


def covering(off, want, B):
    """the resource's blocks that hold [off, off + want), want > 0"""
    return range(off // B, (off + want - 1) // B + 1)


def model_read(loader, fmt, packed, packed_len, block_first, block_off, lengths, B, n_blocks_table, requests, out_caps, blocks_max,
               block_crc=None):
    """(outputs: bytes, or None where the status is not OK; statuses; (units, distinct blocks, decoded blocks))"""
    n = len(lengths)
    first, off = [int(x) for x in block_first], [int(x) for x in block_off]
    verdict = {}                                               # container block -> (bytes or None, decoded)

    def block(j, e):
        if j not in verdict:
            o0, o1 = off[j], off[j + 1]
            data, dec = None, False
            if not (o1 < o0 or o1 > packed_len or o1 - o0 > e or o1 == o0):
                if o1 - o0 == e:
                    data = bytes(packed[o0:o1])
                else:
                    dec = True
                    ds, got, _ = loader.oracle_decompress_ex(fmt, bytes(packed[o0:o1]), e)
                    data = got if ds == OK and len(got) == e else None
                if data is not None and block_crc is not None and zlib.crc32(data) != int(block_crc[j]):
                    data = None
            verdict[j] = (data, dec)
        return verdict[j][0]
    outs, status, run, units = [], [], 0, 0
    for q, (r, o, ln) in enumerate(requests):
        r, o, ln = int(r) & M64, int(o) & M64, int(ln) & M64
        if r >= n or first[r] > n_blocks_table or first[r + 1] > n_blocks_table:
            st, out = ARG, None
        elif (first[r + 1] - first[r]) & M64 != (int(lengths[r]) + B - 1) // B:
            st, out = DATA, None
        else:
            L = int(lengths[r])
            o = min(o, L)
            want = min(ln, L - o)
            if want == 0:
                st, out = OK, b""
            elif want > int(out_caps[q]):
                st, out = BUF, None
            else:
                cov = covering(o, want, B)
                run += len(cov)
                if run > blocks_max:
                    st, out = ARG, None
                else:
                    units += len(cov)
                    parts = [block(first[r] + jb, min(B, L - jb * B)) for jb in cov]
                    if any(p is None for p in parts):
                        st, out = DATA, None
                    else:
                        st, out = OK, b"".join(parts)[o - cov[0] * B: o - cov[0] * B + want]
        outs.append(out)
        status.append(st)
    return outs, status, (units, len(verdict), sum(1 for d, dec in verdict.values() if dec))


def block_crcs(buffers_, B, n_blocks_table):
    """what mscomp_amd_blocks_crc keeps beside a container: zlib's crc32 of every block, 0 behind the last one"""
    out = [zlib.crc32(b[at: at + B]) for b in buffers_ for at in range(0, len(b), B)]
    return np.array(out + [0] * (n_blocks_table - len(out)), dtype=np.uint32)
