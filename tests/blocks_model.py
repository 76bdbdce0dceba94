"""The block container (include/mscomp_amd.h, mscomp_amd_blocks_*) restated over the oracle's one-shot codecs, and the recipes of its fixture
(tests/golden/blocks.json, written by tools/make_golden_blocks.py). Not collected as a test.

A recipe is one resource: ``kind`` with ``seed`` and a length given as ``mult * B + add`` (so that the same recipe lands on the block
boundaries of every block size); the threshold recipes ("prefix": k random bytes, then zeros) have a fixed length ``blen`` and belong to one
format, and to one block size unless blen is below the smallest one (a short lone block of any container).
"""
import hashlib
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "blocks.json")
BLOCK_SIZES = (4096, 32768, 65536, 524288)
OK, ARG, DATA, BUF = 0, -2, -3, -5
M64 = (1 << 64) - 1


def load():
    with open(PATH) as f:
        return json.load(f)


def _text(rs, n):
    words = [rs.bytes(int(rs.randint(3, 20))) for _ in range(32)]
    out = bytearray()
    while len(out) < n:
        out += words[int(rs.randint(0, 32))]
    return bytes(out[:n])


def build(recipe, B):
    """the bytes of a recipe at block size B"""
    n = recipe["blen"] if "blen" in recipe else recipe["mult"] * B + recipe["add"]
    rs = np.random.RandomState(recipe["seed"])
    kind = recipe["kind"]
    if kind == "zeros":
        return bytes(n)
    if kind == "random":
        return rs.bytes(n)
    if kind == "text":
        return _text(rs, n)
    if kind == "prefix":                                       # k random bytes, then zeros: the compressed length moves with k
        return rs.bytes(recipe["k"]) + bytes(n - recipe["k"])
    assert kind == "mixed", kind                               # blocks by turns random and text
    out = b""
    while len(out) < n:
        m = min(B, n - len(out))
        out += rs.bytes(m) if (len(out) // B) % 2 == 0 else _text(rs, m)
    return out


def recipes_for(fixture, fmt, B):
    """the recipes that take part in a (format, block size) batch, in fixture order"""
    return [r for r in fixture["recipes"] + fixture["thresholds"]
            if "blen" not in r or (r["fmt"] == fmt and (r["blen"] == B or r["blen"] < BLOCK_SIZES[0]))]


def stored(loader, fmt, block):
    """the stored form of one block: ms_compress's bytes when they are shorter, the block otherwise"""
    st, c = loader.oracle_compress(fmt, block)
    assert st == 0
    return c if len(c) < len(block) else block


def model_compress(loader, fmt, buffers, B, in_total_max, packed_cap):
    """(packed bytes that were written, block_first [n + 1], block_off [n_blocks_max + 1], statuses [n])"""
    n = len(buffers)
    nbmax = n + in_total_max // B
    first, off, status, pieces, run = [0], [0], [], [], 0
    for buf in buffers:
        run += len(buf)
        st = ARG if run > in_total_max else OK
        if st == OK:
            for at in range(0, len(buf), B):
                s = stored(loader, fmt, buf[at: at + B])
                off.append(off[-1] + len(s))
                if off[-1] <= packed_cap:
                    pieces.append(s)
                else:
                    st = BUF
        first.append(len(off) - 1)
        status.append(st)
    off += [off[-1]] * (nbmax + 1 - len(off))
    return b"".join(pieces), np.array(first, dtype=np.uint64), np.array(off, dtype=np.uint64), np.array(status, dtype=np.int32)


def model_decompress(loader, fmt, packed, packed_len, block_first, block_off, lengths, B, in_total_max, out_caps, ranges=None):
    """(outputs: bytes, or None where the status is not OK; statuses), with the checks in the header's order"""
    n = len(lengths)
    nbmax = n + in_total_max // B
    first, off = [int(x) for x in block_first], [int(x) for x in block_off]
    outs, status, run = [], [], 0
    for r in range(n):
        ln = int(lengths[r])
        run += ln
        nblk = (ln + B - 1) // B
        if run > in_total_max or first[r] > nbmax or first[r + 1] > nbmax:
            st, out = ARG, None
        elif (first[r + 1] - first[r]) & M64 != nblk:
            st, out = DATA, None
        else:
            f, c = (0, nblk) if ranges is None else (min(int(ranges[r][0]), nblk), int(ranges[r][1]))
            c = min(c, nblk - f)
            want = min(ln, (f + c) * B) - f * B if c else 0
            st, out = (BUF, None) if want > int(out_caps[r]) else (OK, b"")
            for jb in range(f, f + c if st == OK else f):
                j = first[r] + jb
                e, o0, o1 = min(B, ln - jb * B), off[j], off[j + 1]
                if o1 < o0 or o1 > packed_len or o1 - o0 > e or o1 == o0:
                    st = DATA
                elif o1 - o0 == e:
                    out += bytes(packed[o0:o1])
                else:
                    ds, got, _ = loader.oracle_decompress_ex(fmt, bytes(packed[o0:o1]), e)
                    if ds != OK or len(got) != e:
                        st = DATA
                    else:
                        out += got
                if st != OK:
                    out = None
                    break
            assert st != OK or len(out) == want
        outs.append(out)
        status.append(st)
    return outs, status


def digest(packed, first, off):
    h = hashlib.sha256()
    h.update(bytes(packed)); h.update(np.asarray(first, dtype="<u8").tobytes()); h.update(np.asarray(off, dtype="<u8").tobytes())
    return h.hexdigest()
