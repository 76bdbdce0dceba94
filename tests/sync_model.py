"""The block sync (include/mscomp_amd.h, mscomp_amd_syncer_sync) restated over zlib.crc32, numpy and the oracle's one-shot decoders: the
blocks of one store container found at any byte offset of raw units, with the header's rules 1-9 in their order. The window checksums
come from the rolling identity, vectorised -- zlib.crc32 at every offset of a 64 KiB-block case would be gigabytes of CRC work. Not
collected as a test.

A store is what splice_model.model_splice takes as a source: (packed, packed_len, block_first, block_off, lengths, block_crc, n_res,
n_blocks_table).
"""
import zlib

import numpy as np

import blocks_model as M
import dedup_model as D

OK, ARG, DATA = M.OK, M.ARG, M.DATA
POLY = 0xEDB88320
T0 = np.zeros(256, dtype=np.uint32)                              # raw() of one byte: zlib's table
for _b in range(256):
    _v = _b
    for _ in range(8):
        _v = (_v >> 1) ^ (POLY if _v & 1 else 0)
    T0[_b] = _v


def mul(a, b):
    """a * b mod the CRC polynomial, registers with the coefficient of x^0 in bit 31 (zlib's multmodp); a may be a uint32 array"""
    a = np.array(a, dtype=np.uint64)
    b = int(b)
    p = np.zeros_like(a)
    for _ in range(32):
        p ^= np.where(a >> np.uint64(31) & np.uint64(1), np.uint64(b), np.uint64(0))
        a = a << np.uint64(1) & np.uint64(0xFFFFFFFF)
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p.astype(np.uint32) if p.ndim else int(p)


def xpow8(n):
    """x^(8 n)"""
    r, sq, n = 0x80000000, 0x40000000, 8 * n                       # x^0, x^1: square and multiply
    while n:
        if n & 1:
            r = mul(r, sq)
        sq = mul(sq, sq)
        n >>= 1
    return r


def prefixes(buf):
    """R[p] = raw(buf[:p]) for p = 0 .. len(buf), uint32: the register after buf[:p] from an initial value of 0. The buffer is cut into
    columns that step together; a first sweep gives every column's raw(), a second one starts each column from what lies in front."""
    data = np.frombuffer(bytes(buf), dtype=np.uint8)
    n = len(data)
    if n == 0:
        return np.zeros(1, dtype=np.uint32)
    seg = max(1, int(np.ceil(np.sqrt(n))))
    cols = (n + seg - 1) // seg
    pad = np.zeros(cols * seg, dtype=np.uint8)
    pad[:n] = data
    grid = pad.reshape(cols, seg)

    def sweep(start, keep):
        r = start.copy()
        out = np.zeros((cols, seg + 1), dtype=np.uint32) if keep else None
        for j in range(seg):
            if keep:
                out[:, j] = r
            r = (r >> np.uint32(8)) ^ T0[(r ^ grid[:, j]) & np.uint32(255)]
        if keep:
            out[:, seg] = r
        return r, out
    tot, _ = sweep(np.zeros(cols, dtype=np.uint32), False)
    f = xpow8(seg)
    start, run = np.zeros(cols, dtype=np.uint32), 0
    for c in range(cols):
        start[c] = run
        run = mul(run, f) ^ int(tot[c])
    _, out = sweep(start, True)
    return np.concatenate([out[:, :seg].reshape(-1)[:n], out[(n - 1) // seg, (n - 1) % seg + 1: (n - 1) % seg + 2]])


def window_crcs(buf, B):
    """zlib.crc32(buf[p : p + B]) for every p with p + B <= len(buf), by the rolling identity: raw(M[:p + B]) ^ raw(M[:p]) x^(8B) ^ seed(B)"""
    if len(buf) < B:
        return np.zeros(0, dtype=np.uint32)
    R = prefixes(buf)
    return R[B:] ^ mul(R[: len(buf) - B + 1], xpow8(B)) ^ np.uint32(zlib.crc32(bytes(B)))


def forge(block):
    """``block`` with its first byte changed and its last four bytes solved so that zlib.crc32 is unchanged. CRC-32 is affine over GF(2):
    the register of the last four bytes is an invertible linear image of them, a 32 x 32 system."""
    block = bytes(block)
    assert len(block) >= 5
    raw = lambda m: zlib.crc32(m) ^ zlib.crc32(bytes(len(m)))                # the linear part
    head = bytes([block[0] ^ 0x5A]) + block[1:-4]
    target = raw(block) ^ raw(head + bytes(4))                               # what the last four bytes must contribute
    cols = [raw((1 << i).to_bytes(4, "little")) for i in range(32)]
    rows, sol = [(cols[i], 1 << i) for i in range(32)], 0
    for bit in range(32):                                                    # Gauss-Jordan on (image, combination) pairs
        piv = next(k for k in range(bit, 32) if rows[k][0] >> bit & 1)
        rows[bit], rows[piv] = rows[piv], rows[bit]
        for k in range(32):
            if k != bit and rows[k][0] >> bit & 1:
                rows[k] = (rows[k][0] ^ rows[bit][0], rows[k][1] ^ rows[bit][1])
    for bit in range(32):
        if target >> bit & 1:
            sol ^= rows[bit][1]
    return head + sol.to_bytes(4, "little")


def thin(cands, B):
    """rule 4 on one unit's raw candidates [(p, row)] in order of p: of a maximal run of consecutive positions with one row only
    p0 + i B survive"""
    out, p0, last, row0 = [], None, None, None
    for p, row in cands:
        if last is None or p != last + 1 or row != row0:
            p0, row0 = p, row
        if (p - p0) % B == 0:
            out.append((p, row))
        last = p
    return out


def greedy(cands, B):
    """what a greedy walk over ALL raw candidates [(p, row)] of one unit takes: the first candidate at or behind ``end``, end = p + B"""
    out, end = [], 0
    for p, row in cands:
        if p >= end:
            out.append((p, row))
            end = p + B
    return out


def store_rows(store, B):
    """rule 1: (statuses, rows): rows[u] = (r, k, offset, stored length, table row) of the accepted resources' rows, numbered densely"""
    status, rows = [], []
    for r in range(int(store[6])):
        st, rr = D.judge(store, r, B)
        status.append(st)
        if st == OK:
            rows += [(r, k, o, ln, j) for k, (o, ln, j) in enumerate(rr)]
    return status, rows


def key_table(store, rows, B):
    """CRC word -> the smallest eligible row that has it"""
    table = {}
    for u, (r, k, o, ln, j) in enumerate(rows):
        if (k + 1) * B <= int(store[4][r]):
            table.setdefault(int(store[5][j]), u)
    return table


def decode_row(loader, fmt, store, row, B):
    """the B bytes of an eligible row as the reader core gives them, or None: a failed table check, a failed decode, a wrong CRC-32"""
    r, k, o, ln, j = row
    if ln == 0 or ln > B:
        return None
    if ln == B:
        data = bytes(store[0][o: o + ln])
    else:
        ds, data, _ = loader.oracle_decompress_ex(fmt, bytes(store[0][o: o + ln]), B)
        if ds != OK or len(data) != B:
            return None
    return data if zlib.crc32(data) == int(store[5][j]) else None


def model_sync(loader, fmt, store, units, offsets, B, in_total_max, n_cand_max):
    """{"res_status", "status", "hit_first", "req" (rows of three), "req_off", "lit_first", "lit" (rows of two), "count" [8], "hits":
    per unit [(p, r, k)], "literals": per unit [(p, length)], "kept": [(unit, p, row)]}"""
    res_status, rows = store_rows(store, B)
    table = key_table(store, rows, B)
    status, run, thinned, n_raw = [], 0, [], 0
    for u, buf in enumerate(units):
        run += len(buf)
        status.append(ARG if run > in_total_max else OK)
        if status[-1] != OK:
            continue
        w = window_crcs(buf, B)
        hit = np.nonzero(np.isin(w, np.fromiter(table.keys(), dtype=np.uint32, count=len(table))))[0] if len(table) and len(w) else []
        raw = [(int(p), table[int(w[p])]) for p in hit]
        n_raw += len(raw)
        thinned += [(u, p, row) for p, row in thin(raw, B)]
    kept = thinned[:n_cand_max]
    decoded = {}
    for _, _, row in kept:
        if row not in decoded:
            decoded[row] = decode_row(loader, fmt, store, rows[row], B)
    hits, lits, n_conf = [[] for _ in units], [[] for _ in units], 0
    ends = [0] * len(units)
    for u, p, row in kept:
        conf = decoded[row] is not None and bytes(units[u][p: p + B]) == decoded[row]
        n_conf += conf
        if conf and p >= ends[u]:
            if p > ends[u]:
                lits[u].append((ends[u], p - ends[u]))
            hits[u].append((p, rows[row][0], rows[row][1]))
            ends[u] = p + B
    for u, buf in enumerate(units):
        if status[u] == OK and len(buf) > ends[u]:
            lits[u].append((ends[u], len(buf) - ends[u]))
    hit_first, lit_first = [0], [0]
    for u in range(len(units)):
        hit_first.append(hit_first[-1] + len(hits[u]))
        lit_first.append(lit_first[-1] + len(lits[u]))
    req = [(r, k * B, B) for hs in hits for _, r, k in hs]
    req_off = [int(offsets[u]) + p for u, hs in enumerate(hits) for p, _, _ in hs]
    lit = [(int(offsets[u]) + p, ln) for u, ls in enumerate(lits) for p, ln in ls]
    count = [n_raw, len(thinned), len(kept), n_conf, len(req), len(lit), sum(ln for _, ln in lit), len(decoded)]
    return {"res_status": res_status, "status": status, "hit_first": hit_first, "req": req, "req_off": req_off, "lit_first": lit_first, "lit": lit,
            "count": count, "hits": hits, "literals": lits, "kept": kept}


def holds_consequence(loader, fmt, store, units, mo, B):
    """the header's consequence in the model: the literal runs copied to their places and every hit's block decoded to its place give
    every accepted unit byte for byte; hits and runs tile the unit without overlap"""
    _, rows = store_rows(store, B)
    at = {(r, k): row for row in rows for r, k in [row[:2]]}
    for u, buf in enumerate(units):
        if mo["status"][u] != OK:
            assert not mo["hits"][u] and not mo["literals"][u]
            continue
        out, seen = bytearray(len(buf)), np.zeros(len(buf), dtype=np.uint8)
        for p, ln in mo["literals"][u]:
            assert ln > 0
            out[p: p + ln] = buf[p: p + ln]
            seen[p: p + ln] += 1
        for p, r, k in mo["hits"][u]:
            out[p: p + B] = decode_row(loader, fmt, store, at[(r, k)], B)
            seen[p: p + B] += 1
        assert bytes(out) == bytes(buf) and (seen == 1).all(), ("unit", u)


# ---- the cases of tests/test_gpu_sync.py, which tests/test_sync_model.py holds to the consequence without a device ----
TILE = 4096                                                      # MSCOMP_AMD_SYNC_TILE


def rnd(seed, n):
    return np.random.RandomState(seed).bytes(n)


def store_buffers(B):
    """three resources: 3 B + 17 mixed, 5 B zeros, one raw block"""
    import read_model as R
    return [M.build(R.RECIPES[i], B) for i in (5, 6, 3)]


def cases(B):
    """name -> the raw units of a call against the store of store_buffers(B)"""
    A, Z, X = store_buffers(B)
    h = B // 2
    return {
        "edits": [b"\x07" + A[: B + h] + A[B + h + 5:], Z[: 2 * B + 100] + rnd(21, 4096) + Z[2 * B + 100 + 4096:], X],
        "seams": [X[: B - 1], X, X + b"x", b"", rnd(22, TILE - 1) + X, rnd(23, TILE) + A[:B] + b"yz", rnd(24, TILE + 1) + X + rnd(25, 3),
                  rnd(26, 2 * TILE - 7) + A[2 * B: 3 * B + 17]],
        "zeros": [bytes(5 * B), rnd(27, TILE - 100) + bytes(5 * B) + rnd(28, 50)],
        "forged": [rnd(29, 33) + forge(X) + rnd(30, 5) + X],
        "short": [A[2 * B:], A[3 * B:] + rnd(31, B)],
    }
