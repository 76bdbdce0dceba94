"""CRC-32 as the library computes it on the GPU (mscomp_amd_plan_execute_crc_dev, mscomp_amd_blocks_crc / _check; include/mscomp_amd.h), restated
over zlib.crc32, with the container's numbering and statuses from tests/blocks_model.py. Not collected as a test."""
import re
import os
import zlib

import numpy as np

import blocks_model as M

OK, ARG, DATA = M.OK, M.ARG, M.DATA
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mscomp_amd.h")


def crc(b):
    return zlib.crc32(bytes(b)) & 0xFFFFFFFF


def kernel_sizes():
    """(row bytes, slice granule) of the CRC kernel, as the header documents them"""
    txt = open(HEADER).read()
    return tuple(int(re.search(r"#define\s+%s\s+(\d+)u" % k, txt).group(1)) for k in ("MSCOMP_AMD_CRC_ROW_BYTES", "MSCOMP_AMD_CRC_SLICE_BYTES"))


def units(mem, offs, lens, in_total_max):
    """(crc uint32 [n], status int32 [n]) of the units mem[off : off + len]: a unit whose running total exceeds in_total_max is rejected"""
    out, st, run = [], [], 0
    for o, n in zip(offs, lens):
        run += int(n)
        rej = run > in_total_max
        st.append(ARG if rej else OK)
        out.append(0 if rej else crc(mem[int(o): int(o) + int(n)]))
    return np.array(out, dtype=np.uint32), np.array(st, dtype=np.int32)


def blocks(buffers, B, in_total_max):
    """(block_crc uint32 [n_blocks_max], res_crc uint32 [n], status [n]): blocks numbered as model_compress numbers them"""
    n = len(buffers)
    bc, rc, st, run = [], [], [], 0
    for buf in buffers:
        run += len(buf)
        if run > in_total_max:
            st.append(ARG); rc.append(0)
            continue
        st.append(OK); rc.append(crc(buf))
        bc += [crc(buf[at: at + B]) for at in range(0, len(buf), B)]
    bc += [0] * (n + in_total_max // B - len(bc))
    return np.array(bc, dtype=np.uint32), np.array(rc, dtype=np.uint32), np.array(st, dtype=np.int32)


def check(out, out_off, lengths, block_first, block_crc, status, out_len, B, in_total_max, ranges=None):
    """(status, out_len) after mscomp_amd_blocks_check of the decoded bytes in `out`"""
    n = len(lengths)
    nbmax = n + in_total_max // B
    first = [int(x) for x in block_first]
    status, out_len, run = [int(s) for s in status], [int(x) for x in out_len], 0
    for r in range(n):
        ln = int(lengths[r])
        run += ln
        if status[r] != OK:
            continue
        nblk = (ln + B - 1) // B
        if run > in_total_max or first[r] > nbmax or first[r + 1] > nbmax:
            status[r], out_len[r] = ARG, 0
            continue
        if (first[r + 1] - first[r]) & M.M64 != nblk:
            status[r], out_len[r] = DATA, 0
            continue
        f, c = (0, nblk) if ranges is None else (min(int(ranges[r][0]), nblk), int(ranges[r][1]))
        c = min(c, nblk - f)
        for k in range(c):
            e = min(B, ln - (f + k) * B)
            at = int(out_off[r]) + k * B
            if crc(out[at: at + e]) != int(block_crc[first[r] + f + k]):
                status[r], out_len[r] = DATA, 0
                break
    return status, out_len


def find_raw_block(first, off, lengths, B):
    """(resource, block number j) of the first block stored raw (stored length = data length), or None"""
    for r, ln in enumerate(lengths):
        for jb in range((ln + B - 1) // B):
            j = int(first[r]) + jb
            if int(off[j + 1]) - int(off[j]) == min(B, ln - jb * B):
                return r, j
    return None


def find_accepted_corruption(loader, fmt, packed, first, off, buffers, B):
    """(resource, position in packed, new byte) of a one-byte change inside a compressed block that the oracle's decoder still answers with
    MSCOMP_OK, the block's length and other data -- with defined behaviour -- or None"""
    for r, buf in enumerate(buffers):
        for jb in range((len(buf) + B - 1) // B):
            j = int(first[r]) + jb
            o0, o1, e = int(off[j]), int(off[j + 1]), min(B, len(buf) - jb * B)
            if o1 - o0 >= e:
                continue
            blk = bytes(packed[o0:o1])
            for p in list(range(len(blk) - 1, max(len(blk) - 200, -1), -1)):
                for x in (1, 2, 32):
                    hurt = bytearray(blk); hurt[p] ^= x
                    ds, got, undefined = loader.oracle_decompress_ex(fmt, bytes(hurt), e)
                    if ds == OK and not undefined and len(got) == e and got != buf[jb * B: jb * B + e]:
                        return r, o0 + p, hurt[p]
    return None
