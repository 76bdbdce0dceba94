"""The block writer (include/mscomp_amd.h, mscomp_amd_writer_*) restated over tests/blocks_model.py and tests/read_model.py: batched byte-range
writes into a container's tables, out of place, with the header's rules 0-9 in their order. Not collected as a test.

A request is (resource, offset, length) and comes with a source: a byte string that holds at least the clipped length.
"""
import zlib

import numpy as np

import blocks_model as M
import read_model as R

OK, ARG, DATA, BUF = M.OK, M.ARG, M.DATA, M.BUF
M64 = M.M64
_containers = {}


def container(loader, fmt, B):
    """(buffers, packed, block_first, block_off, n_blocks_table, block_crc) of R.RECIPES as the container model compresses them; made once"""
    if (fmt, B) not in _containers:
        bufs = R.buffers(B)
        total = sum(len(b) for b in bufs)
        packed, first, off, st = M.model_compress(loader, fmt, bufs, B, total, total)
        assert not st.any()
        nbt = len(bufs) + total // B
        _containers[(fmt, B)] = (bufs, packed, first, off, nbt, R.block_crcs(bufs, B, nbt))
    return _containers[(fmt, B)]


def clip(req, lengths):
    """(off', want) of a request, (0, 0) where there is no such resource"""
    r, o, ln = (int(x) & M64 for x in req)
    if r >= len(lengths):
        return 0, 0
    L = int(lengths[r])
    o = min(o, L)
    return o, min(ln, L - o)


def patched(buffers, reqs, srcs, applied=None):
    """the resources with the requests applied by plain slicing, in request order (applied: one flag per request, default all)"""
    out = [bytearray(b) for b in buffers]
    lens = [len(b) for b in buffers]
    for q, (req, src) in enumerate(zip(reqs, srcs)):
        o, want = clip(req, lens)
        if want and (applied is None or applied[q]):
            out[int(req[0])][o: o + want] = src[:want]
    return [bytes(b) for b in out]


def model_write(loader, fmt, packed, packed_len, block_first, block_off, lengths, B, n_blocks_table, reqs, srcs, blocks_max, new_cap,
                block_crc=None):
    """dict: packed (the bytes written: the blocks that end within new_cap), off (n_blocks_table + 1), crc (n_blocks_table, or None),
    written, status (per request), res_status (per resource), counts (units, distinct blocks touched, blocks encoded again)"""
    n, nbt = len(lengths), n_blocks_table
    first, off = [int(x) for x in block_first], [int(x) for x in block_off]
    nb = first[n]
    # 0. the table as a whole
    if nb > nbt or any(first[i] > first[i + 1] for i in range(n)):
        return {"packed": b"", "off": np.zeros(nbt + 1, dtype=np.uint64), "crc": None if block_crc is None else np.zeros(nbt, dtype=np.uint32),
                "written": [0] * len(reqs), "status": [ARG] * len(reqs), "res_status": [ARG] * n, "counts": (0, 0, 0)}
    verdict = {}                                               # container block -> its data, or None: read once

    def block(j, e):
        if j not in verdict:
            o0, o1 = off[j], off[j + 1]
            data = None
            if not (o1 < o0 or o1 > packed_len or o1 - o0 > e or o1 == o0):
                if o1 - o0 == e:
                    data = bytes(packed[o0:o1])
                else:
                    ds, got, _ = loader.oracle_decompress_ex(fmt, bytes(packed[o0:o1]), e)
                    data = got if ds == OK and len(got) == e else None
                if data is not None and block_crc is not None and zlib.crc32(data) != int(block_crc[j]):
                    data = None
            verdict[j] = data
        return verdict[j]
    status, written, plans, run, units = [], [], [], 0, 0
    for q, req in enumerate(reqs):
        r = int(req[0]) & M64
        st, want, plan = OK, 0, None
        if r >= n:                                             # 1.
            st = ARG
        elif first[r + 1] - first[r] != (int(lengths[r]) + B - 1) // B:   # 2.
            st = DATA
        else:
            L = int(lengths[r])
            o, want = clip(req, lengths)                       # 3.
            if want:
                cov = R.covering(o, want, B)
                run += len(cov)                                # 4.
                if run > blocks_max:
                    st = ARG
                else:
                    units += len(cov)
                    parts = [block(first[r] + jb, min(B, L - jb * B)) for jb in cov]   # 5.
                    if any(p is None for p in parts):
                        st = DATA
                    else:
                        plan = (r, o, want, cov)
        status.append(st)                                      # 6.
        written.append(want if st == OK else 0)
        plans.append(plan)
    fresh = {}                                                 # 7. container block -> its new data
    for plan, src in zip(plans, srcs):
        if plan is None:
            continue
        r, o, want, cov = plan
        for jb in cov:
            j = first[r] + jb
            d = fresh.setdefault(j, bytearray(verdict[j]))
            lo, hi = max(o, jb * B), min(o + want, jb * B + len(d))
            d[lo - jb * B: hi - jb * B] = src[lo - o: hi - o]
    new_off, crc, pieces = [0], [], []                         # 8.
    for j in range(nb):
        if j in fresh:
            s, c = M.stored(loader, fmt, bytes(fresh[j])), zlib.crc32(bytes(fresh[j]))
        else:
            s = bytes(packed[off[j]: off[j + 1]]) if off[j] <= off[j + 1] <= packed_len else b""
            c = 0 if block_crc is None else int(block_crc[j])
        new_off.append(new_off[-1] + len(s))
        crc.append(c)
        if new_off[-1] <= new_cap:                             # 9.
            pieces.append(s)
    res_status = [BUF if first[r + 1] > first[r] and new_off[first[r + 1]] > new_cap else OK for r in range(n)]
    new_off += [new_off[-1]] * (nbt + 1 - len(new_off))
    return {"packed": b"".join(pieces), "off": np.array(new_off, dtype=np.uint64),
            "crc": None if block_crc is None else np.array(crc + [0] * (nbt - nb), dtype=np.uint32),
            "written": written, "status": status, "res_status": res_status, "counts": (units, len(verdict), len(fresh))}
