"""The block searcher (include/mscomp_amd_search.h, mscomp_amd_searcher_*) restated over tests/blocks_model.py: the reader's request rules
with the look-ahead in the budget and without the capacity rule, the pattern rules, and the hits by bytes.find in a loop. Not collected as
a test.

EDGES names the corners of the contract; model_search says which of them a call reached (under "edges"), so that a test can assert that
its data reaches them.
"""
import zlib

import blocks_model as M

OK, ARG, DATA = M.OK, M.ARG, M.DATA
M64 = M.M64
PAT_MAX, LEN_MAX = 64, 256
EDGES = ("hit_spans_blocks", "hit_ends_at_resource_end", "cut_by_resource_end", "filter_past_end", "tail_outside_range", "start_at_range_end_not_found",
         "pattern_refused_empty", "pattern_refused_long", "pattern_refused_backwards", "equal_patterns", "overlapping_hits", "overflow",
         "lookahead_block_only", "budget_by_lookahead", "shared_block", "request_not_ok")


def patterns_of(blob, pat_off, len_max):
    """(patterns: bytes, or None for a refused one; statuses) by the header's pattern rules"""
    pats, status = [], []
    for a, b in zip(pat_off[:-1], pat_off[1:]):
        a, b = int(a), int(b)
        ok = a < b and b - a <= len_max
        pats.append(bytes(blob[a:b]) if ok else None)
        status.append(OK if ok else ARG)
    return pats, status


def pack_patterns(patterns):
    """byte strings back to back: (blob, pat_off)"""
    off = [0]
    for p in patterns:
        off.append(off[-1] + len(p))
    return b"".join(patterns), off


def find_all(data, pat, lo, hi):
    """every x in [lo, hi) with data[x : x + len(pat)] == pat, by bytes.find: overlapping occurrences included"""
    out, x = [], data.find(pat, lo, hi + len(pat) - 1)
    while x != -1 and x < hi:
        out.append(x)
        x = data.find(pat, x + 1, hi + len(pat) - 1)
    return out


def model_search(loader, fmt, packed, packed_len, block_first, block_off, lengths, B, n_blocks_table, requests, blob, pat_off, len_max, blocks_max, hits_max,
                 block_crc=None):
    """{"records": [(x, q << 32 | p), ...] (the first hits_max in (q, x, p) order), "req_hits", "count": [total, written], "pat_status",
    "status", "counts": (units, distinct blocks, decoded blocks), "edges": the names of EDGES the call reached}"""
    n = len(lengths)
    first, off = [int(x) for x in block_first], [int(x) for x in block_off]
    pats, pat_status = patterns_of(blob, pat_off, len_max)
    edges = set()
    for a, b in zip(pat_off[:-1], pat_off[1:]):
        edges |= {"pattern_refused_empty"} if a == b else {"pattern_refused_backwards"} if b < a else {"pattern_refused_long"} if b - a > len_max else set()
    live = [p for p in pats if p is not None]
    if len(set(live)) < len(live):
        edges.add("equal_patterns")
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
        else:
            edges.add("shared_block")
        return verdict[j][0]
    records, req_hits, status, run, units = [], [], [], 0, 0
    for q, (r, o, ln) in enumerate(requests):
        r, o, ln = int(r) & M64, int(o) & M64, int(ln) & M64
        found = []
        if r >= n or first[r] > n_blocks_table or first[r + 1] > n_blocks_table:
            st = ARG
        elif (first[r + 1] - first[r]) & M64 != (int(lengths[r]) + B - 1) // B:
            st = DATA
        else:
            L = int(lengths[r])
            o = min(o, L)
            want = min(ln, L - o)
            st = OK
            if want:
                cov = range(o // B, (min(L, o + want + len_max - 1) - 1) // B + 1)
                plain = (o + want - 1) // B - o // B + 1
                run += len(cov)
                if run > blocks_max:
                    st = ARG
                    if run - len(cov) + plain <= blocks_max:
                        edges.add("budget_by_lookahead")
                else:
                    units += len(cov)
                    if len(cov) > plain:
                        edges.add("lookahead_block_only")
                    parts = [block(first[r] + jb, min(B, L - jb * B)) for jb in cov]
                    if any(p is None for p in parts):
                        st = DATA
                    else:
                        base = cov[0] * B
                        data = bytes(base) + b"".join(parts)       # (indexed by position in the resource; the bytes in front are never looked at)
                        for p, pat in enumerate(pats):
                            if pat is None:
                                continue
                            hi = min(o + want, L - len(pat) + 1)
                            xs = find_all(data, pat, o, hi) if hi > o else []
                            found += [(x, p) for x in xs]
                            if any(x // B != (x + len(pat) - 1) // B for x in xs):
                                edges.add("hit_spans_blocks")
                            if any(x + len(pat) == L for x in xs):
                                edges.add("hit_ends_at_resource_end")
                            if any(x + len(pat) > o + want for x in xs):
                                edges.add("tail_outside_range")
                            if any(x + 4 > L for x in xs):
                                edges.add("filter_past_end")
                            if L - len(pat) + 1 < o + want and data[L - len(pat) + 1: L] == pat[: len(pat) - 1] and len(pat) > 1:
                                edges.add("cut_by_resource_end")
                            if o + want + len(pat) <= L and data[o + want: o + want + len(pat)] == pat:
                                edges.add("start_at_range_end_not_found")
        if st != OK:
            edges.add("request_not_ok")
        found.sort()
        if any(a[0] < b[0] < a[0] + len(pats[a[1]]) for a, b in zip(found, found[1:])):
            edges.add("overlapping_hits")
        records += [(x, (q << 32) | p) for x, p in found]
        req_hits.append(len(found))
        status.append(st)
    total = len(records)
    if total > hits_max:
        edges.add("overflow")
    return {"records": records[:hits_max], "req_hits": req_hits, "count": [total, min(total, hits_max)], "pat_status": pat_status, "status": status,
            "counts": (units, len(verdict), sum(1 for d, dec in verdict.values() if dec)), "edges": edges}


# ---- the data of the searcher's tests ---------------------------------------------------------------------------------------------------------
NEEDLE = b"\xF1\xF2\xF3\xF4\xF5"                               # occurs in no block but where it is planted: soft bytes are below 8
ONE, THREE, B_LESS, B_EXACT, B_MORE, MIX, SOFT_FIRST, RANDOM_FIRST, RUN = 1, 2, 3, 4, 5, 6, 7, 8, 9   # rows of buffers()
END1, END3 = b"\xAB", b"\xCD\xEF\x99"                          # the resources of 1 and 3 bytes: stored raw, back to back


def soft(rs, n):
    """n bytes that every format compresses"""
    return bytes(rs.randint(0, 8, n).astype("uint8"))


def planted(buf, at, what=NEEDLE):
    return buf[:at] + what + buf[at + len(what):]


def buffers(B):
    """The resources of lengths 0, 1, 3, B - 1, B, B + 1 and 3 B + 5, soft and random blocks mixed so that decoded and raw blocks lie side
    by side; two of six blocks, soft and random by turns, one beginning with each kind, with NEEDLE at the splits 1|4 .. 4|1 across their
    block boundaries 1 .. 4, ending at boundary 5, and at their first and last five bytes; and three blocks of the letter a."""
    import numpy as np
    rs = np.random.RandomState(2024)
    turns = lambda k0, n: b"".join(soft(rs, B) if (k0 + k) % 2 == 0 else rs.bytes(B) for k in range(n))
    six = []
    for k0 in (0, 1):
        buf = turns(k0, 6)
        for s in (1, 2, 3, 4):
            buf = planted(buf, s * B - s)
        six.append(planted(planted(planted(buf, 5 * B - 5), 0), 6 * B - 5))
    mix = planted(turns(0, 3) + soft(rs, 5), 3 * B)               # (NEEDLE is the short last block)
    return [b"", END1, END3, soft(rs, B - 1), rs.bytes(B), planted(soft(rs, B + 1), B - 4), mix, six[0], six[1], b"a" * (3 * B)]


def brute(buffers, requests, patterns, len_max):
    """the hits of requests against plain resources, position by position and byte by byte: [(q, x, p), ...] in ascending order"""
    out = []
    for q, (r, o, ln) in enumerate(requests):
        data = buffers[r]
        L = len(data)
        o = min(o, L)
        for x in range(o, o + min(ln, L - o)):
            for p, pat in enumerate(patterns):
                if 1 <= len(pat) <= len_max and x + len(pat) <= L and all(data[x + k] == pat[k] for k in range(len(pat))):
                    out.append((q, x, p))
    return out
