"""The block digests (include/mscomp_amd.h, mscomp_amd_digester_* and mscomp_amd_syncer_sync_digest) restated over hashlib.blake2s, with the
container's numbering and statuses from tests/crc_model.py and the sync's rules from tests/sync_model.py. Not collected as a test."""
import hashlib

import numpy as np

import blocks_model as M
import sync_model as Y

OK, ARG, DATA = M.OK, M.ARG, M.DATA
LEAF = 1024


def block_digest(data):
    """BLAKE2s in tree mode: leaves of 1024 bytes, two levels, unlimited fan-out, 16 bytes inner and final, no key"""
    data = bytes(data)
    n = max(1, -(-len(data) // LEAF)); inner = b""
    for i in range(n):
        inner += hashlib.blake2s(data[i*LEAF:(i+1)*LEAF], digest_size=16, fanout=0, depth=2, leaf_size=LEAF,
                                 node_offset=i, node_depth=0, inner_size=16, last_node=(i == n-1)).digest()
    return hashlib.blake2s(inner, digest_size=16, fanout=0, depth=2, leaf_size=LEAF,
                           node_offset=0, node_depth=1, inner_size=16, last_node=True).digest()


def words(digest):
    """the 16 bytes as the device holds them: four uint32 words"""
    return np.frombuffer(digest, dtype="<u4")


def model_digests(buffers, B, in_total_max):
    """(block_digest uint32 [n_blocks_max, 4], status [n]): blocks numbered and resources refused as crc_model.blocks does it; the rows
    at and behind the real block count are zeros"""
    n = len(buffers)
    rows, st, run = [], [], 0
    for buf in buffers:
        run += len(buf)
        if run > in_total_max:
            st.append(ARG)
            continue
        st.append(OK)
        rows += [words(block_digest(buf[at: at + B])) for at in range(0, len(buf), B)]
    out = np.zeros((n + in_total_max // B, 4), dtype=np.uint32)
    if rows:
        out[: len(rows)] = np.array(rows, dtype=np.uint32)
    return out, np.array(st, dtype=np.int32)


def store_digests(buffers, B, nbt):
    """the digest column of a healthy store of ``buffers`` with ``nbt`` table rows"""
    out = np.zeros((nbt, 4), dtype=np.uint32)
    rows = [words(block_digest(buf[at: at + B])) for buf in buffers for at in range(0, len(buf), B)]
    out[: len(rows)] = np.array(rows, dtype=np.uint32).reshape(-1, 4)
    return out


def model_check(out, out_off, lengths, block_first, block_dig, status, out_len, B, in_total_max, ranges=None):
    """(status, out_len) after mscomp_amd_digester_check of the decoded bytes in ``out``: crc_model.check with a digest for a CRC word"""
    n = len(lengths)
    nbmax = n + in_total_max // B
    first = [int(x) for x in block_first]
    dig = np.asarray(block_dig, dtype=np.uint32).reshape(-1, 4)
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
            if not (words(block_digest(bytes(out[at: at + e]))) == dig[first[r] + f + k]).all():
                status[r], out_len[r] = DATA, 0
                break
    return status, out_len


def model_sync_digest(store, block_dig, units, offsets, B, in_total_max, n_cand_max):
    """sync_model.model_sync with rule 6 replaced: a kept candidate is confirmed when the digest of its window equals the four words at
    its table row; no stored byte is read (store[0] may be None), no decoder is asked. count[7] = the kept count."""
    dig = np.asarray(block_dig, dtype=np.uint32).reshape(-1, 4)
    res_status, rows = Y.store_rows(store, B)
    table = Y.key_table(store, rows, B)
    status, run, thinned, n_raw = [], 0, [], 0
    for u, buf in enumerate(units):
        run += len(buf)
        status.append(ARG if run > in_total_max else OK)
        if status[-1] != OK:
            continue
        w = Y.window_crcs(buf, B)
        hit = np.nonzero(np.isin(w, np.fromiter(table.keys(), dtype=np.uint32, count=len(table))))[0] if len(table) and len(w) else []
        raw = [(int(p), table[int(w[p])]) for p in hit]
        n_raw += len(raw)
        thinned += [(u, p, row) for p, row in Y.thin(raw, B)]
    kept = thinned[:n_cand_max]
    hits, lits, n_conf = [[] for _ in units], [[] for _ in units], 0
    ends = [0] * len(units)
    for u, p, row in kept:
        conf = bool((words(block_digest(units[u][p: p + B])) == dig[rows[row][4]]).all())
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
    count = [n_raw, len(thinned), len(kept), n_conf, len(req), len(lit), sum(ln for _, ln in lit), len(kept)]
    return {"res_status": res_status, "status": status, "hit_first": hit_first, "req": req, "req_off": req_off, "lit_first": lit_first, "lit": lit,
            "count": count, "hits": hits, "literals": lits, "kept": kept}
