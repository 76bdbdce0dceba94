"""The block diff (include/mscomp_amd.h, mscomp_amd_deduper_diff) restated over plain lists and bytes: which blocks of the new resources
differ from the blocks at the same index of the base resources, with the header's rules 1-7 in their order, answered as the delta and the
patch extent lists. Diff never encodes or decodes, so no oracle is called. Not collected as a test.

A source is what splice_model.model_splice takes: (packed, packed_len, block_first, block_off, lengths, block_crc or None, n_res,
n_blocks_table).
"""
import blocks_model as M
import dedup_model as D
import extents_model as X

OK, ARG, DATA = M.OK, M.ARG, M.DATA
M64 = M.M64
NO_BASE = M64


def default_pairs(base, new):
    """(r, r) for the common resources, (NO_BASE, r) for the new resources behind the base's last"""
    return [(r if r < int(base[6]) else NO_BASE, r) for r in range(int(new[6]))]


def table_rules(source, r, B):
    """dedup's rules 1 and 2 on resource r: (status, block count)"""
    first, lens, nbt = source[2], source[4], source[7]
    f0, f1 = int(first[r]), int(first[r + 1])
    if f0 > f1 or f1 > int(nbt):
        return ARG, 0
    L = int(lens[r])
    return (OK, f1 - f0) if f1 - f0 == L // B + (1 if L % B else 0) else (DATA, 0)


def row_ok(source, j):
    o0, o1 = int(source[3][j]), int(source[3][j + 1])
    return o0 <= o1 <= int(source[1])


def model_diff(base, new, pairs, B, n_blocks_new, with_crc=True):
    """{"status" [n_pair], "changed" [n_pair], "count" [4], "delta_first" / "patch_first" [n_pair + 1], "delta_ext" / "patch_ext": rows of
    four, "verdicts": per pair the list of its blocks' verdicts (True = changed), None for a refused pair}"""
    with_crc = with_crc and base[5] is not None and new[5] is not None
    status, verdicts, run = [], [], 0
    for a, b in pairs:
        a, b = int(a) & M64, int(b) & M64
        if b >= int(new[6]) or (a != NO_BASE and a >= int(base[6])):            # rule 1
            status.append(ARG); verdicts.append(None); continue
        (sb, nb), (sa, na) = table_rules(new, b, B), (table_rules(base, a, B) if a != NO_BASE else (OK, 0))
        st = next((s for rule in (ARG, DATA) for s in (sb, sa) if s == rule), OK)   # rule 2, dedup's 1 and 2: the first rule that refuses, b before a
        if st != OK:
            status.append(st); verdicts.append(None); continue
        run = min(run + nb, M64)                                                # rule 3: the total includes this pair, and the ones refused here
        if nb and run > n_blocks_new:
            status.append(ARG); verdicts.append(None); continue
        fb, fa = int(new[2][b]), (int(base[2][a]) if a != NO_BASE else 0)
        if not all(row_ok(new, fb + k) for k in range(nb)) or not all(row_ok(base, fa + k) for k in range(min(na, nb))):   # rule 2, dedup's 3
            status.append(DATA); verdicts.append(None); continue
        status.append(OK)
        Lb, La = int(new[4][b]), (int(base[4][a]) if a != NO_BASE else 0)
        v = []
        for k in range(nb):                                                     # rule 5
            same = a != NO_BASE and k < na and min(B, Lb - k * B) == min(B, La - k * B)
            tables = same
            if same:
                ob, oa = int(new[3][fb + k]), int(base[3][fa + k])
                sb_, sa_ = int(new[3][fb + k + 1]) - ob, int(base[3][fa + k + 1]) - oa
                tables = sb_ == sa_ and (not with_crc or int(new[5][fb + k]) == int(base[5][fa + k]))
                same = tables and bytes(new[0][ob: ob + sb_]) == bytes(base[0][oa: oa + sa_])
            v.append((not same, tables and not same, (int(new[3][fb + k + 1]) - int(new[3][fb + k]))))
        verdicts.append(v)
    delta_first, patch_first, delta_ext, patch_ext, changed = [0], [0], [], [], []
    count = [0, 0, 0, 0]
    for p, ((a, b), v) in enumerate(zip(pairs, verdicts)):
        n_changed = 0
        if v is not None:
            a, b = int(a) & M64, int(b) & M64
            k = 0
            while k < len(v):                                                   # rule 6: the runs
                c = 1
                while k + c < len(v) and v[k + c][0] == v[k][0]:
                    c += 1
                if v[k][0]:
                    patch_ext.append((1, p, n_changed, c)); delta_ext.append((0, b, k, c)); n_changed += c
                else:
                    patch_ext.append((0, a, k, c))
                k += c
            count[0] += n_changed; count[1] += len(v)
            count[2] += sum(x[2] for x in v if x[0]); count[3] += sum(1 for x in v if x[1])
        changed.append(n_changed)
        delta_first.append(len(delta_ext)); patch_first.append(len(patch_ext))
    return {"status": status, "changed": changed, "count": count, "delta_first": delta_first, "patch_first": patch_first,
            "delta_ext": delta_ext, "patch_ext": patch_ext, "verdicts": [None if v is None else [x[0] for x in v] for v in verdicts]}


def as_source(new, nbt=None):
    """a container model_splice_extents returned as a source tuple"""
    n = len(new["new_len"])
    nbt = len(new["off"]) - 1 if nbt is None else nbt
    return (new["packed"], len(new["packed"]), new["first"], new["off"], list(new["new_len"]), new["crc"], n, nbt)


def model_delta_and_patch(base, new, pairs, d, B, n_blocks_new, with_crc=True):
    """(delta container, rebuilt container) as model_splice_extents returns them: the delta lists over {new}, the patch lists over {base, delta}"""
    with_crc = with_crc and base[5] is not None and new[5] is not None
    delta = X.model_splice_extents([new], d["delta_first"], d["delta_ext"], B, n_blocks_new, n_blocks_new, 1 << 60, with_crc=with_crc)
    built = X.model_splice_extents([base, as_source(delta)], d["patch_first"], d["patch_ext"], B, n_blocks_new, n_blocks_new, 1 << 60, with_crc=with_crc)
    return delta, built


def holds_consequence(base, new, pairs, d, B, n_blocks_new, with_crc=True):
    """the header's consequence, with the extents model as the splicer: the delta container holds the changed blocks and nothing else, and
    resource p of the rebuilt container has the length, the rows, the stored bytes and the CRC words of new resource b, for every accepted
    pair; returns (delta, rebuilt)"""
    with_crc = with_crc and base[5] is not None and new[5] is not None
    delta, built = model_delta_and_patch(base, new, pairs, d, B, n_blocks_new, with_crc)
    assert len(delta["packed"]) == d["count"][2] and int(delta["first"][len(pairs)]) == d["count"][0]
    for p, (a, b) in enumerate(pairs):
        if d["status"][p] != OK:
            assert delta["new_len"][p] == 0 and built["new_len"][p] == 0 and d["changed"][p] == 0
            assert d["delta_first"][p] == d["delta_first"][p + 1] and d["patch_first"][p] == d["patch_first"][p + 1]
            continue
        assert delta["status"][p] == OK and built["status"][p] == OK, ("splice statuses of pair", p)
        assert int(delta["first"][p + 1]) - int(delta["first"][p]) == d["changed"][p]
        st, rows = D.judge(new, int(b), B)
        assert st == OK
        f0, f1 = int(built["first"][p]), int(built["first"][p + 1])
        assert int(built["new_len"][p]) == int(new[4][int(b)]) and f1 - f0 == len(rows), ("length or rows of pair", p)
        for k, (o, ln, j) in enumerate(rows):
            n0, n1 = int(built["off"][f0 + k]), int(built["off"][f0 + k + 1])
            assert n1 - n0 == ln and bytes(built["packed"][n0:n1]) == bytes(new[0][o: o + ln]), ("row", k, "of pair", p)
            assert not with_crc or int(built["crc"][f0 + k]) == int(new[5][j]), ("CRC word of row", k, "of pair", p)
    return delta, built


def same_container(built, new, with_crc=True):
    """the rebuilt container against the new one byte for byte: packed bytes, block_first, the block_off and CRC entries in use"""
    n, nb = int(new[6]), int(new[2][int(new[6])])
    assert bytes(built["packed"]) == bytes(new[0][: int(new[1])])
    assert [int(x) for x in built["first"][: n + 1]] == [int(x) for x in new[2][: n + 1]]
    assert [int(x) for x in built["off"][: nb + 1]] == [int(x) for x in new[3][: nb + 1]]
    assert [int(x) for x in built["new_len"]] == [int(x) for x in new[4]]
    if with_crc:
        assert [int(x) for x in built["crc"][:nb]] == [int(x) for x in new[5][:nb]]
