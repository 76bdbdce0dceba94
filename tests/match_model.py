"""The block match (include/mscomp_amd.h, mscomp_amd_deduper_match) restated over plain lists and bytes: for every block of the resources
of ``new``, whether an equal block lies in a store (found), earlier in new (shared) or nowhere (fresh), with the header's rules 1-8 in
their order, answered as the delta and the patch extent lists. Match never encodes or decodes, so no oracle is called. Not collected as a
test.

A source is what splice_model.model_splice takes: (packed, packed_len, block_first, block_off, lengths, block_crc or None, n_res,
n_blocks_table).
"""
import blocks_model as M
import dedup_model as D
import diff_model as F
import extents_model as X

OK, ARG, DATA = M.OK, M.ARG, M.DATA
M64 = M.M64
FOUND, SHARED, FRESH = 0, 1, 2


def model_match(stores, new, B, n_blocks_total, n_blocks_new, with_crc=True):
    """{"status" [N], "cls" [3 n_new], "count" [6], "delta_first" / "patch_first" [n_new + 1], "delta_ext" / "patch_ext": rows of four,
    "rows": per row of the numbering (g, k), "rep": per row its representative, "classes": per resource of new the list of its blocks'
    classes, None for a refused one}"""
    sources = list(stores) + [new]
    with_crc = with_crc and all(s[5] is not None for s in sources)
    where = [(s, r) for s, src in enumerate(sources) for r in range(int(src[6]))]
    n_store = len(where) - int(new[6])
    status, rows_of, run_all, run_new = [], [], 0, 0
    for g, (s, r) in enumerate(where):
        st, nb = F.table_rules(sources[s], r, B)                                 # rules 1 and 2
        if st == OK:
            run_all = min(run_all + nb, M64)                                     # rule 4: the totals include this resource, and the ones refused here
            if g >= n_store:
                run_new = min(run_new + nb, M64)
            if nb and (run_all > n_blocks_total or (g >= n_store and run_new > n_blocks_new)):
                st = ARG
        rows = None
        if st == OK:
            st, rows = D.judge(sources[s], r, B)                                 # rule 3
        status.append(st); rows_of.append(rows if st == OK else None)
    numbering, whole, key = [], [], []
    for g, (s, r) in enumerate(where):
        packed, crc, L = sources[s][0], sources[s][5], int(sources[s][4][r])
        for k, (o, ln, j) in enumerate(rows_of[g] or []):
            e, c = min(B, L - k * B), (int(crc[j]) if with_crc else None)
            numbering.append((g, k))
            whole.append((e, ln, c, bytes(packed[o: o + ln])))
            key.append((e, ln, c, bytes(packed[o: o + min(16, ln)]), bytes(packed[o + ln - min(16, ln): o + ln])))
    first_whole, first_key, rep, refuted = {}, {}, [], 0
    for u in range(len(numbering)):                                              # rule 6, and the refuted from the key tuple
        rep.append(first_whole.setdefault(whole[u], u))
        least = first_key.setdefault(key[u], u)
        if least != u and whole[least] != whole[u]:
            refuted += 1
    row_at = {gk: u for u, gk in enumerate(numbering)}
    u0 = sum(len(rows_of[g] or []) for g in range(n_store))
    n_new = int(new[6])
    delta_first, patch_first, delta_ext, patch_ext, cls, classes = [0], [0], [], [], [], []
    count = [0, 0, 0, 0, 0, refuted]
    fresh_rank = {}                                                              # row -> its rank among the fresh blocks of its resource
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
            while k < len(us):                                                   # rule 7: the runs
                c = 1
                while k + c < len(us) and kind[k + c] == kind[k] and (kind[k] == FRESH or (
                        rep[us[k + c]] == rep[us[k + c - 1]] + 1 and numbering[rep[us[k + c]]][0] == numbering[rep[us[k + c - 1]]][0])):
                    c += 1
                if kind[k] == FRESH:
                    patch_ext.append((len(stores), q, n_fresh, c)); delta_ext.append((0, q, k, c))
                    for i in range(c):
                        fresh_rank[us[k + i]] = n_fresh + i
                    n_fresh += c
                    count[4] += sum(rows_of[g][k + i][1] for i in range(c))
                elif kind[k] == FOUND:
                    rg, rk = numbering[rep[us[k]]]
                    patch_ext.append((where[rg][0], where[rg][1], rk, c))
                else:
                    patch_ext.append((len(stores), numbering[rep[us[k]]][0] - n_store, fresh_rank[rep[us[k]]], c))
                per[kind[k]] += c
                k += c
            count[3] += len(us)
        cls += per
        for i in range(3):
            count[i] += per[i]
        delta_first.append(len(delta_ext)); patch_first.append(len(patch_ext))
    return {"status": status, "cls": cls, "count": count, "delta_first": delta_first, "patch_first": patch_first, "delta_ext": delta_ext,
            "patch_ext": patch_ext, "rows": numbering, "rep": rep, "classes": classes, "n_store": n_store}


def model_delta_and_patch(stores, new, d, B, n_blocks_new, with_crc=True):
    """(delta container, rebuilt container) as model_splice_extents returns them: the delta lists over {new}, the patch lists over
    {stores..., delta}"""
    with_crc = with_crc and all(s[5] is not None for s in list(stores) + [new])
    cut = lambda s: s if with_crc else tuple(s[:5]) + (None,) + tuple(s[6:])
    delta = X.model_splice_extents([cut(new)], d["delta_first"], d["delta_ext"], B, n_blocks_new, n_blocks_new, 1 << 60, with_crc=with_crc)
    built = X.model_splice_extents([cut(s) for s in stores] + [F.as_source(delta)], d["patch_first"], d["patch_ext"], B, n_blocks_new, n_blocks_new, 1 << 60,
                                   with_crc=with_crc)
    return delta, built


def holds_consequence(stores, new, d, B, n_blocks_new, with_crc=True):
    """the header's consequence, with the extents model as the splicer: the delta container holds the fresh blocks and nothing else, and
    resource q of the rebuilt container has the length, the rows, the stored bytes and the CRC words of resource q of new, for every
    accepted q; returns (delta, rebuilt)"""
    with_crc = with_crc and all(s[5] is not None for s in list(stores) + [new])
    delta, built = model_delta_and_patch(stores, new, d, B, n_blocks_new, with_crc)
    n_new, n_store = int(new[6]), d["n_store"]
    assert len(delta["packed"]) == d["count"][4] and int(delta["first"][n_new]) == d["count"][2]
    for q in range(n_new):
        if d["status"][n_store + q] != OK:
            assert delta["new_len"][q] == 0 and built["new_len"][q] == 0 and d["cls"][3 * q: 3 * q + 3] == [0, 0, 0]
            assert d["delta_first"][q] == d["delta_first"][q + 1] and d["patch_first"][q] == d["patch_first"][q + 1]
            continue
        assert delta["status"][q] == OK and built["status"][q] == OK, ("splice statuses of resource", q)
        assert int(delta["first"][q + 1]) - int(delta["first"][q]) == d["cls"][3 * q + 2]
        st, rows = D.judge(new, q, B)
        assert st == OK
        f0, f1 = int(built["first"][q]), int(built["first"][q + 1])
        assert int(built["new_len"][q]) == int(new[4][q]) and f1 - f0 == len(rows), ("length or rows of resource", q)
        for k, (o, ln, j) in enumerate(rows):
            n0, n1 = int(built["off"][f0 + k]), int(built["off"][f0 + k + 1])
            assert n1 - n0 == ln and bytes(built["packed"][n0:n1]) == bytes(new[0][o: o + ln]), ("row", k, "of resource", q)
            assert not with_crc or int(built["crc"][f0 + k]) == int(new[5][j]), ("CRC word of row", k, "of resource", q)
    return delta, built
