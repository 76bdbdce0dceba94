"""Match by digest (include/mscomp_amd_match_digest.h, mscomp_amd_deduper_match_digest) restated over plain lists: tests/match_model.py with
rule 6 replaced -- two rows are equal when their data lengths and their four digest words are equal -- and the key tuple (data length,
h0, h1). The table rules, the numbering, the runs and the counts are match's and are taken from where match_model takes them; the
consequence and the two splices are match_model's own functions, used as they are. No stored byte is read: a source's packed bytes may be
None. Digests of real data come from tests/digest_model.py. Not collected as a test.

A source is what match_model takes: (packed or None, packed_len, block_first, block_off, lengths, block_crc or None, n_res,
n_blocks_table); its digest column is rows of four words, one per table row.
"""
import numpy as np

import dedup_model as D
import diff_model as F
import digest_model as G
import match_model as T

OK, ARG, DATA, M64 = T.OK, T.ARG, T.DATA, T.M64
FOUND, SHARED, FRESH = T.FOUND, T.SHARED, T.FRESH
model_delta_and_patch, holds_consequence = T.model_delta_and_patch, T.holds_consequence


def column(buffers, B, nbt=None):
    """the digest column of a healthy container of ``buffers`` (digest_model.store_digests), with ``nbt`` table rows (default: its blocks)"""
    nb = sum((len(b) + B - 1) // B for b in buffers)
    return G.store_digests(buffers, B, nb if nbt is None else nbt)


def model_match_digest(stores, store_digests, new, new_digest, B, n_blocks_total, n_blocks_new):
    """what match_model.model_match returns, from equality by (e, digest); "read": the (source, table row) pairs whose digest was read"""
    sources = list(stores) + [new]
    cols = [np.asarray(d, dtype=np.uint32).reshape(-1, 4) if d is not None else np.zeros((0, 4), dtype=np.uint32) for d in list(store_digests) + [new_digest]]
    where = [(s, r) for s, src in enumerate(sources) for r in range(int(src[6]))]
    n_store = len(where) - int(new[6])
    status, rows_of, run_all, run_new = [], [], 0, 0
    for g, (s, r) in enumerate(where):
        st, nb = F.table_rules(sources[s], r, B)                                 # rules 1 and 2
        if st == OK:
            run_all = min(run_all + nb, M64)                                     # rule 4
            if g >= n_store:
                run_new = min(run_new + nb, M64)
            if nb and (run_all > n_blocks_total or (g >= n_store and run_new > n_blocks_new)):
                st = ARG
        rows = None
        if st == OK:
            st, rows = D.judge(sources[s], r, B)                                 # rule 3: the offsets against packed_len, no byte read
        status.append(st); rows_of.append(rows if st == OK else None)
    numbering, whole, key, read = [], [], [], []
    for g, (s, r) in enumerate(where):
        L = int(sources[s][4][r])
        for k, (o, ln, j) in enumerate(rows_of[g] or []):
            e, d = min(B, L - k * B), tuple(int(x) for x in cols[s][j])
            numbering.append((g, k)); read.append((s, j))
            whole.append((e,) + d)
            key.append((e, d[0], d[1]))
    first_whole, first_key, rep, refuted = {}, {}, [], 0
    for u in range(len(numbering)):                                              # rule 6, and the refuted from the key tuple
        rep.append(first_whole.setdefault(whole[u], u))
        least = first_key.setdefault(key[u], u)
        if least != u and whole[least] != whole[u]:
            refuted += 1
    out = runs_and_counts(len(stores), where, n_store, int(new[6]), status, rows_of, numbering, rep, refuted)
    out["read"] = read
    return out


def runs_and_counts(n_src, where, n_store, n_new, status, rows_of, numbering, rep, refuted):
    """rules 7 and 8 from the representatives, as match_model.model_match states them"""
    row_at = {gk: u for u, gk in enumerate(numbering)}
    u0 = sum(len(rows_of[g] or []) for g in range(n_store))
    delta_first, patch_first, delta_ext, patch_ext, cls, classes = [0], [0], [], [], [], []
    count = [0, 0, 0, 0, 0, refuted]
    fresh_rank = {}
    for q in range(n_new):
        g = n_store + q
        per = [0, 0, 0]
        if rows_of[g] is None:
            classes.append(None)
        else:
            us = [row_at[(g, k)] for k in range(len(rows_of[g]))]
            kind = [FOUND if rep[u] < u0 else FRESH if rep[u] == u else SHARED for u in us]
            classes.append(kind)
            n_fresh, k = 0, 0
            while k < len(us):
                c = 1
                while k + c < len(us) and kind[k + c] == kind[k] and (kind[k] == FRESH or (
                        rep[us[k + c]] == rep[us[k + c - 1]] + 1 and numbering[rep[us[k + c]]][0] == numbering[rep[us[k + c - 1]]][0])):
                    c += 1
                if kind[k] == FRESH:
                    patch_ext.append((n_src, q, n_fresh, c)); delta_ext.append((0, q, k, c))
                    for i in range(c):
                        fresh_rank[us[k + i]] = n_fresh + i
                    n_fresh += c
                    count[4] += sum(rows_of[g][k + i][1] for i in range(c))       # the stored bytes, from new's offset table
                elif kind[k] == FOUND:
                    rg, rk = numbering[rep[us[k]]]
                    patch_ext.append((where[rg][0], where[rg][1], rk, c))
                else:
                    patch_ext.append((n_src, numbering[rep[us[k]]][0] - n_store, fresh_rank[rep[us[k]]], c))
                per[kind[k]] += c
                k += c
            count[3] += len(us)
        cls += per
        for i in range(3):
            count[i] += per[i]
        delta_first.append(len(delta_ext)); patch_first.append(len(patch_ext))
    return {"status": status, "cls": cls, "count": count, "delta_first": delta_first, "patch_first": patch_first, "delta_ext": delta_ext,
            "patch_ext": patch_ext, "rows": numbering, "rep": rep, "classes": classes, "n_store": n_store}


def brute_force(stores_data, new_data, B):
    """per block of new's buffers (resource, block) -> ("found", store, resource, block) / ("shared", resource, block) / ("fresh",): the
    smallest equal DECODED block, stores first in order, then the earlier blocks of new -- what the call must say of healthy containers"""
    seen, out = {}, {}
    for s, bufs in enumerate(stores_data):
        for r, buf in enumerate(bufs):
            for k in range((len(buf) + B - 1) // B):
                seen.setdefault(bytes(buf[k * B: (k + 1) * B]), ("found", s, r, k))
    for r, buf in enumerate(new_data):
        for k in range((len(buf) + B - 1) // B):
            blk = bytes(buf[k * B: (k + 1) * B])
            out[(r, k)] = seen.get(blk, ("fresh",))
            seen.setdefault(blk, ("shared", r, k))
    return out
