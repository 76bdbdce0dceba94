"""The CPU model of what csrc/lznt1.hip does to a chunk, for the tests/test_gpu_lznt1_*.py case files: the kernels' geometry, the bucket hash and
the searches for keys of chosen buckets, the sorted bucket array with the greedy parse and the finishing steps on it, the small parts the unit
builders share, and the one walker of an LZNT1 stream. numpy only. tests/test_lznt1_geometry.py holds the constants to the kernel source."""
import functools

import numpy as np

CHUNK = 4096
BITS = 12                                  # LZ_TBL_BITS: the hash's width
SELF = 4                                   # LZ_SELF: candidates a lane scans by itself; the wave finishes the rest 64 per step
PART_FIRST = (0, 15 * 64, 39 * 64)         # LZ4_P1, LZ4_P2: first positions of the sort's three parts (batches of 64 positions)
SEG_FIRST_WINDOW = (0, 21, 38, 52, 64)     # LZ4_B1 .. LZ4_B3: first windows of the parse's four segments (LZ4_NSEG), and the chunk's end
MAXM = 22                                  # LZ4_MAXM: matches that can start in one window of 64 positions
HASH_MUL = 0x9E3779B1                      # lz_hash's multiplier

BUCKET, NKEYS = 3001, 160                  # the bucket the finishing-step units fill, and how many of its keys they may use
P34, P18 = 1500, 3000                      # target positions with max_len 34 (lane 28 of its window) and 18


# ---- the hash and the keys of chosen buckets -----------------------------------------------------------------------------
def raw_hash(key24):
    """the hash of a 3-byte key BEFORE 0 is mapped to 1"""
    return ((key24 * HASH_MUL) & 0xFFFFFFFF) >> (32 - BITS)


def bucket_of(key24):
    """the kernels' bucket of a 3-byte key (lznt1.hip lz_hash): bucket 0 stays empty, its keys go to bucket 1"""
    h = raw_hash(key24)
    return np.where(h == 0, 1, h)


@functools.lru_cache(maxsize=None)
def _raw_hash_of_every_key():
    """brute force, once per process: the raw hash of all 2^24 keys"""
    return raw_hash(np.arange(1 << 24, dtype=np.uint64)).astype(np.uint16)


def _le3(k):
    k = int(k)
    return bytes([k & 0xFF, (k >> 8) & 0xFF, (k >> 16) & 0xFF])


@functools.lru_cache(maxsize=None)
def keys_of_bucket(bucket, count, distinct_bytes=True):
    """the `count` smallest keys of `bucket` (as 3 bytes, little-endian), by default those with three different bytes each"""
    h = _raw_hash_of_every_key()
    out = []
    for k in np.flatnonzero((h == bucket) | (h == 0 if bucket == 1 else False)):
        b = _le3(k)
        if not distinct_bytes or len(set(b)) == 3:
            out.append(b)
        if len(out) == count:
            return out
    raise AssertionError("bucket %d has fewer than %d keys" % (bucket, count))


def keys_with_raw_hash(targets, per_bucket):
    """{target: the `per_bucket` smallest keys (3 bytes, little-endian)} for every target value of the hash BEFORE 0 is mapped to 1"""
    h = _raw_hash_of_every_key()
    out = {t: [_le3(k) for k in np.flatnonzero(h == t)[:per_bucket]] for t in targets}
    assert all(len(ks) == per_bucket for ks in out.values())
    return out


def keys_by_bucket(targets, per_bucket):
    """{target: up to `per_bucket` smallest keys (3 bytes, little-endian)} for every target bucket"""
    h = _raw_hash_of_every_key()
    return {t: [_le3(k) for k in np.flatnonzero((h == t) | (h == 0 if t == 1 else False))[:per_bucket]] for t in targets}


def straddling_buckets(count):
    """buckets h whose two ends (bits 12 (h - 1) .. 12 (h + 1) of the packed table) cross a dword boundary"""
    return [h for h in range(2, 1 << BITS) if (BITS * (h - 1)) % 32 + 2 * BITS > 32][:count]


# ---- the bucket array of a chunk and the parse on it ---------------------------------------------------------------------
def bucket_model(c):
    """the sorted bucket array of a chunk: (array of positions by (hash, position), slot of every key position in it, its rank in its bucket)"""
    c = np.asarray(c, dtype=np.uint32)
    k = c[:-2] | (c[1:-1] << 8) | (c[2:] << 16)
    h = bucket_of(k.astype(np.uint64))
    pos = np.arange(len(h))
    arr = np.lexsort((pos, h))
    slot = np.empty(len(h), dtype=np.int64)
    slot[arr] = pos
    rank = slot - np.searchsorted(h[arr], h)
    return arr, slot, rank


def lcp(c, q, p, lim):
    n = 0
    while n < lim and c[q + n] == c[p + n]:
        n += 1
    return n


def token_shift(pos):
    """bits of the length in a match token at position pos (lznt1.hip lz_shift: the token split depends on the position)"""
    return 12 if pos <= 16 else 12 - ((pos - 1).bit_length() - 4)


def max_len(n, p):
    """max_len of position p of a chunk of n bytes"""
    return min(n - p, (1 << token_shift(p)) + 2)


def best_key(l, q):
    """what the kernel maximises over a position's candidates: the longer match, on equal length the older candidate"""
    return (l << 12) | (q ^ 4095)


def greedy_match(c):
    """f(p) -> the length of position p's best match, 0 for a literal: the longest, at least 3 bytes, among the older entries of its bucket"""
    n = len(c)
    arr, slot, rank = bucket_model(c)
    c = np.concatenate([np.asarray(c, dtype=np.int32), np.full(4200, -1, np.int32)])

    def match(p):
        best = 0
        if p > 0 and p + 3 <= n and rank[p]:
            q = arr[slot[p] - rank[p]:slot[p]]
            lim = max_len(n, p)
            while len(q) and best < lim:
                q = q[c[q + best] == c[p + best]]
                best += len(q) > 0
        return best if best >= 3 else 0
    return match


def parse(c):
    """the greedy parse of a chunk on the model: {token start: match length, 0 for a literal}"""
    match = greedy_match(c)
    out, p = {}, 0
    while p < len(c):
        out[p] = match(p)
        p += out[p] or 1
    return out


def greedy_token_starts(c):
    """the positions where a token of the greedy parse starts"""
    return set(parse(c))


def finish(c, p):
    """What the wave does when the greedy walk lands on position p, on the model of the bucket array: the eager scan of the four oldest
    candidates (up to 16 bytes), the cooperative extension of those that reached 16 with max_len beyond, then the finishing steps, 64 candidates
    each, the step that holds p's own entry the last. Per step: the threshold in bytes, the winners' lanes, whether the second compare stage
    and the tail beyond 16 bytes run."""
    n = len(c)
    arr, slot, rank = bucket_model(c)
    r = int(rank[p])
    cands = [int(q) for q in arr[slot[p] - r:slot[p]]]
    maxl = max_len(n, p)
    lens = [lcp(c, q, p, maxl) for q in cands]
    eager = list(zip(lens[:SELF], cands[:SELF]))
    prov = max([best_key(min(l, 16), q) for l, q in eager] + [0])            # the eager scan stops at 16 bytes
    pending = maxl > 16 and any(l >= 16 for l, _ in eager)
    unresolved = r > SELF and (prov >> 12) < maxl
    best = max([prov] + [best_key(l, q) for l, q in eager if l >= 16]) if pending else prov
    res = {"rank": r, "cands": cands, "lens": lens, "maxl": maxl, "provisional": prov, "raised": best, "pending": pending,
           "finish": unresolved and (best >> 12) < maxl, "steps": [], "left": 0}
    if not res["finish"]:
        res["best"] = best
        return res
    base = SELF
    while True:
        lanes = range(base, min(base + 64, r))
        need = max((best >> 12) + 1, 3)
        win = [j for j in lanes if lens[j] >= need]
        res["steps"].append({"need": need, "winners": [j - base for j in win], "valid": len(lanes),
                             "stage2": maxl > 8 and any(lens[j] >= 8 for j in lanes), "tail": maxl > 16 and any(lens[j] >= 16 for j in lanes)})
        if win:
            new = max(best_key(lens[j], cands[j]) for j in win)
            assert new > best
            best = new
        seen = max([res["raised"]] + [best_key(lens[j], cands[j]) for j in range(min(base + 64, r))])
        assert best == seen or (seen >> 12) < 3          # the same match as the maximum of the keys seen so far
        if (best >> 12) == maxl or r < base + 64:
            res["left"] = max(0, r - (base + 64))
            break
        base += 64
    res["best"] = best
    return res


# ---- the builders' small parts ---------------------------------------------------------------------------------------------
def filler(n, seed):
    """random bytes whose trigrams are all different: every position a literal, no bucket fuller than chance makes it"""
    for s in range(200):
        r = np.random.default_rng(seed * 1000 + s).integers(0, 256, n, dtype=np.uint8)
        if n < 3:
            return r
        k = r[:-2].astype(np.uint32) | (r[1:-1].astype(np.uint32) << 8) | (r[2:].astype(np.uint32) << 16)
        if len(np.unique(k)) == len(k):
            return r
    raise AssertionError("no filler with distinct trigrams")


def place(c, at, b):
    c[at:at + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)


def noise(seed, n=CHUNK):
    return bytearray(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes())


def place_key(seed, key, positions, n=CHUNK):
    """seeded bytes with the 3-byte key at the given positions (each followed by bytes that differ from occurrence to occurrence)"""
    d = noise(seed, n)
    for p in positions:
        d[p:p + 3] = key
    return bytes(d[:n])


# ---- the walker of an LZNT1 stream -----------------------------------------------------------------------------------------
def walk_stream(stream):
    """per chunk of an LZNT1 stream, up to its end or a zero header: (offset of the chunk's header, the header, whether the chunk is a raw copy,
    its tokens as [(position in the chunk, match length or 0 for a literal)]; a raw chunk has no tokens)"""
    i = 0
    while i + 2 <= len(stream):
        hdr = stream[i] | (stream[i + 1] << 8)
        if hdr == 0:
            break
        end = i + 2 + (hdr & 0xFFF) + 1
        raw = not hdr & 0x8000
        tokens, pos, j = [], 0, i + 2
        while j < end and not raw:
            flags = stream[j]
            j += 1
            for b in range(8):
                if j >= end:
                    break
                if (flags >> b) & 1:
                    tok = stream[j] | (stream[j + 1] << 8)
                    j += 2
                    tokens.append((pos, (tok & ((1 << token_shift(pos)) - 1)) + 3))
                    pos += tokens[-1][1]
                else:
                    tokens.append((pos, 0))
                    j += 1
                    pos += 1
        yield i, hdr, raw, tokens
        i = end


def chunk_streams(stream):
    """the chunks of a stream, each with its header"""
    return [stream[i:i + (hdr & 0xFFF) + 3] for i, hdr, _, _ in walk_stream(stream)]


def token_lengths(stream):
    """{token start: match length, 0 for a literal} of the first chunk of a stream"""
    return dict(next(walk_stream(stream))[3])
