"""The finishing steps of LZNT1's window parse (csrc/lznt1.hip lz_window) reduce their 64 candidates only when one of them beats the best
match so far: the candidates of a step are younger than the best's and the older one wins on equal length, so only a candidate strictly
longer than the best (and at least 3 bytes long) can change it. One compare and a ballot find those lanes -- the winners -- and a step
without one leaves the best alone.
The units here put one position of a chunk (the target, a token start of the greedy parse) on every path of that rule: no winner, one,
several, in the first finishing step and in a later one, with winners that end in the first compare stage, in the second, beyond 16 bytes, at
max_len and at the chunk's end, and behind a cooperative extension that has raised the best first. Every unit is one chunk, or two. Each
builder proves on a CPU model of the bucket array which path every finishing step of its target takes and fails if the unit is not what it
claims; the GPU tests (-m gpu) compare the units with the oracle byte for byte in both chunk-kernel modes, the CPU test checks that the
units cover every cell of {none, one, several winners} x {first step, later step}."""
import functools

import numpy as np
import pytest

LZNT1 = 2
BITS = 12
SELF = 4          # candidates a lane scans by itself; the wave finishes the rest 64 per step
BUCKET = 3001


def _hash(key24):
    """the kernels' bucket of a 3-byte key (lznt1.hip lz_hash): bucket 0 stays empty, its keys go to bucket 1"""
    h = ((key24 * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - BITS)
    return np.where(h == 0, 1, h)


NKEYS = 160


@functools.lru_cache(maxsize=None)
def _keys():
    """brute force over all 2^24 keys: NKEYS keys of BUCKET (as 3 bytes, little-endian) with three different bytes each"""
    ks = np.flatnonzero(_hash(np.arange(1 << 24, dtype=np.uint64)) == BUCKET).astype(np.uint32)
    out = []
    for k in ks:
        b = bytes([k & 0xFF, (k >> 8) & 0xFF, (k >> 16) & 0xFF])
        if len(set(b)) == 3:
            out.append(b)
        if len(out) == NKEYS:
            return out
    raise AssertionError("bucket %d has fewer than %d keys" % (BUCKET, NKEYS))


def _model(c):
    """the sorted bucket array of a chunk: (array of positions by (hash, position), slot of every key position in it, its rank in its bucket)"""
    c = np.asarray(c, dtype=np.uint32)
    k = c[:-2] | (c[1:-1] << 8) | (c[2:] << 16)
    h = _hash(k.astype(np.uint64))
    pos = np.arange(len(h))
    arr = np.lexsort((pos, h))
    slot = np.empty(len(h), dtype=np.int64)
    slot[arr] = pos
    rank = slot - np.searchsorted(h[arr], h)
    return arr, slot, rank


def _lcp(c, q, p, lim):
    n = 0
    while n < lim and c[q + n] == c[p + n]:
        n += 1
    return n


def _maxlen(n, p):
    """max_len of position p of a chunk of n bytes (lznt1.hip lz_shift: the token split depends on the position)"""
    shift = 12 if p <= 16 else 12 - ((p - 1).bit_length() - 4)
    return min(n - p, (1 << shift) + 2)


def _key(l, q):
    return (l << 12) | (q ^ 4095)


def _token_starts(c):
    """the greedy parse of a chunk: the positions where a token starts (the best match of a position is the longest, at least 3 bytes, among the
    older entries of its bucket)"""
    n = len(c)
    arr, slot, rank = _model(c)
    c = np.concatenate([np.asarray(c, dtype=np.int32), np.full(4200, -1, np.int32)])
    starts, p = set(), 0
    while p < n:
        starts.add(p)
        best = 0
        if p > 0 and p + 3 <= n and rank[p]:
            q = arr[slot[p] - rank[p]:slot[p]]
            lim = _maxlen(n, p)
            while len(q) and best < lim:
                q = q[c[q + best] == c[p + best]]
                best += len(q) > 0
        p += best if best >= 3 else 1
    return starts


def _finish(c, p):
    """What the wave does when the greedy walk lands on position p, on the model of the bucket array: the eager scan of the four oldest
    candidates (up to 16 bytes), the cooperative extension of those that reached 16 with max_len beyond, then the finishing steps, 64 candidates
    each, the step that holds p's own entry the last. Per step: the threshold in bytes, the winners' lanes, whether the second compare stage
    and the tail beyond 16 bytes run."""
    n = len(c)
    arr, slot, rank = _model(c)
    r = int(rank[p])
    cands = [int(q) for q in arr[slot[p] - r:slot[p]]]
    maxl = _maxlen(n, p)
    lens = [_lcp(c, q, p, maxl) for q in cands]
    eager = list(zip(lens[:SELF], cands[:SELF]))
    prov = max([_key(min(l, 16), q) for l, q in eager] + [0])            # the eager scan stops at 16 bytes
    pending = maxl > 16 and any(l >= 16 for l, _ in eager)
    unresolved = r > SELF and (prov >> 12) < maxl
    best = max([prov] + [_key(l, q) for l, q in eager if l >= 16]) if pending else prov
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
            new = max(_key(lens[j], cands[j]) for j in win)
            assert new > best
            best = new
        seen = max([res["raised"]] + [_key(lens[j], cands[j]) for j in range(min(base + 64, r))])
        assert best == seen or (seen >> 12) < 3          # the same match as the maximum of the keys seen so far
        if (best >> 12) == maxl or r < base + 64:
            res["left"] = max(0, r - (base + 64))
            break
        base += 64
    res["best"] = best
    return res


def _kind(step):
    return ("none", "one", "several")[min(len(step["winners"]), 2)]


def _filler(n, seed):
    """random bytes whose trigrams are all different: every position a literal, no bucket fuller than chance makes it"""
    for s in range(200):
        r = np.random.default_rng(seed * 1000 + s).integers(0, 256, n, dtype=np.uint8)
        if n < 3:
            return r
        k = r[:-2].astype(np.uint32) | (r[1:-1].astype(np.uint32) << 8) | (r[2:].astype(np.uint32) << 16)
        if len(np.unique(k)) == len(k):
            return r
    raise AssertionError("no filler with distinct trigrams")


def _place(c, at, b):
    c[at:at + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)


def _build(p, spec, seed, cut=None):
    """A chunk whose position p has len(spec) older entries in its bucket, oldest first: 0 = a position of another key of the bucket (it agrees
    with p on fewer than 3 bytes), L >= 3 = a position that agrees with p on exactly L bytes (on max_len and more where L is max_len).
    Between the candidates and p's window a 24-byte block repeats, so that the chunk is not stored raw; p's window holds filler in front of p.
    cut: the chunk ends cut bytes behind p, and the candidates' bytes from `cut` on are zeros (what a compare past the end would look at)."""
    n = p + 64
    nc = len(spec)
    ks = _keys()                                       # ks[j]: the colliding key of candidate j, ks[-1]: the position's own
    assert nc < NKEYS
    for s in range(60):
        sd = seed + 7919 * s
        c = _filler(n, sd).copy()
        x = np.concatenate([np.frombuffer(ks[-1], dtype=np.uint8), _filler(60, sd + 13)])   # the position's bytes
        at, where = 8, []
        for j, L in enumerate(spec):
            where.append(at)
            if L == 0:
                _place(c, at, ks[j])
                at += 6
            else:
                _place(c, at, x[:L])
                c[at + L] = x[L] ^ 0x55                                  # the first byte that differs
                if cut is not None:
                    c[at + cut:at + L + 1] = 0
                at += L + 4
        hi = p & ~63
        assert hi - (at + 8) >= 48, "no room for the repeats in front of position %d" % p
        c[at + 8:hi] = np.resize(_filler(24, sd + 5), hi - (at + 8))
        _place(c, p, x[:min(len(x), n - p)])
        if cut is not None:
            c = c[:p + cut].copy()
        f = _finish(c, p)
        want = [min(L, cut) if cut is not None and L else L for L in spec]
        if f["rank"] != nc or f["cands"] != where:
            continue                                   # (a filler trigram fell into the bucket: next filler)
        if not all(l == w if w else l < 3 for l, w in zip(f["lens"], want)):
            continue
        if p not in _token_starts(c):
            continue
        return c, f
    raise AssertionError("no unit for position %d, candidates %s" % (p, spec))


P34, P18 = 1500, 3000                                  # target positions with max_len 34 and 18


def _cases():
    """(name, position, candidates, expected kind of every finishing step, further conditions on the model's result, keyword arguments)"""
    Z = [0]
    cs = []

    def add(name, p, spec, kinds, check=None, **kw):
        cs.append((name, p, spec, kinds, check, kw))
    # -- no winner
    add("ties with the best's length: the eager, older candidate stays", P34, [5, 0, 4, 0, 5, 4, 3, 5, 0, 5], ["none"],
        lambda f: f["best"] == _key(5, f["cands"][0]))
    add("ties with an eager candidate that is not the oldest", P18, [0, 0, 7, 0, 7, 0, 7, 6], ["none"], lambda f: f["best"] == _key(7, f["cands"][2]))
    add("other trigrams of the bucket, the eager best below 3 bytes", P34, Z * 11, ["none"], lambda f: (f["best"] >> 12) < 3)
    add("the same over two steps", P34, Z * 70, ["none", "none"], lambda f: (f["best"] >> 12) < 3)
    add("ties in the second step", P34, [6, 0, 0, 0] + Z * 64 + [6, 5, 0], ["none", "none"], lambda f: f["best"] == _key(6, f["cands"][0]))
    # -- one winner
    add("one winner in lane 0", P34, Z * 4 + [6] + Z * 3, ["one"], lambda f: f["steps"][0]["winners"] == [0])
    add("one winner in lane 63", P34, Z * 4 + Z * 63 + [6] + Z * 2, ["one", "none"], lambda f: f["steps"][0]["winners"] == [63])
    add("one winner in the last valid lane, in front of the own entry", P34, Z * 4 + Z * 5 + [6], ["one"],
        lambda f: f["steps"][0]["winners"] == [5] and f["steps"][0]["valid"] == 6)
    add("one winner in the last valid lane of a full step", P18, Z * 4 + Z * 63 + [4], ["one", "none"],
        lambda f: f["steps"][0]["winners"] == [63] and f["steps"][1]["valid"] == 0)
    add("one winner in the second step", P34, Z * 4 + Z * 64 + [0, 0, 7, 0], ["none", "one"], lambda f: f["steps"][1]["winners"] == [2])
    add("one winner over an eager match", P18, [4, 0, 3, 0, 4, 5, 4, 3], ["one"], lambda f: f["best"] == _key(5, f["cands"][5]))
    # -- several winners
    add("several winners of equal length: the lowest lane", P34, Z * 4 + [0, 6, 0, 6, 6], ["several"], lambda f: f["best"] == _key(6, f["cands"][5]))
    add("winners of equal length in two steps: the first step's", P34, Z * 4 + Z * 10 + [6, 6] + Z * 52 + [6, 6, 0], ["several", "none"],
        lambda f: f["best"] == _key(6, f["cands"][14]))
    add("rising length across two steps, several in each", P34, [3, 0, 0, 0] + [5, 7] + Z * 62 + [6, 7, 8, 0, 9], ["several", "several"],
        lambda f: [s["need"] for s in f["steps"]] == [4, 8] and f["best"] == _key(9, f["cands"][72]))
    add("rising length across two steps, one in the second", P34, [3, 0, 0, 0] + [5, 7] + Z * 62 + [6, 7, 8, 0], ["several", "one"],
        lambda f: [s["need"] for s in f["steps"]] == [4, 8] and f["best"] == _key(8, f["cands"][70]))
    add("the longest of several is not the oldest", P18, Z * 4 + [4, 9, 6, 9, 3], ["several"], lambda f: f["best"] == _key(9, f["cands"][5]))
    # -- winners by stage
    for L in (9, 12, 16):
        add("second stage: %d bytes over an eager 8" % L, P34, [8, 0, 0, 0, 0, L, 8], ["one"],
            lambda f, L=L: f["steps"][0]["stage2"] and f["steps"][0]["need"] == 9 and (f["best"] >> 12) == L)
    add("second stage: 9 bytes do not beat an eager 9", P34, [9, 0, 0, 0, 0, 9, 8], ["none"], lambda f: f["steps"][0]["stage2"])
    for L in (17, 25, 33):
        add("beyond 16 bytes: %d" % L, P34, [9, 0, 0, 0, 0, L, 9], ["one"], lambda f, L=L: f["steps"][0]["tail"] and (f["best"] >> 12) == L)
    add("beyond 16 bytes: several, the older of the longest", P34, Z * 4 + [20, 17, 20], ["several"],
        lambda f: f["steps"][0]["tail"] and f["best"] == _key(20, f["cands"][4]))
    add("exactly max_len 34: the loop stops with candidates left behind", P34, Z * 4 + [0, 34, 0] + Z * 70, ["one"],
        lambda f: (f["best"] >> 12) == f["maxl"] == 34 and f["left"] > 0)
    add("exactly max_len 18: the loop stops with candidates left behind", P18, Z * 4 + [0, 18, 0] + Z * 70, ["one"],
        lambda f: (f["best"] >> 12) == f["maxl"] == 18 and f["left"] > 0)
    add("max_len reached by several", P34, Z * 4 + [34, 20, 34] + Z * 66, ["several"],
        lambda f: f["best"] == _key(34, f["cands"][4]) and f["left"] > 0)
    add("max_len reached in the second step", P18, [5, 0, 0, 0] + Z * 64 + [5, 18, 18] + Z * 64, ["none", "several"],
        lambda f: f["best"] == _key(18, f["cands"][69]) and f["left"] > 0)
    for m in (3, 5, 8, 12, 17):
        add("exactly n - p = %d" % m, 1500 - m, Z * 4 + [0, 30, 0], ["one"], lambda f, m=m: (f["best"] >> 12) == f["maxl"] == m, cut=m)
    add("n - p = 12 reached by several", 1488, Z * 4 + [30, 5, 30], ["several"], lambda f: f["best"] == _key(12, f["cands"][4]), cut=12)
    # -- behind a cooperative extension: the position is long-pending (an eager candidate reached 16 bytes, max_len 34) and unresolved
    add("the threshold follows the extension: 18 bytes lose to the raised 20", P34, [20, 0, 0, 0, 18, 0, 17], ["none"],
        lambda f: f["pending"] and (f["provisional"] >> 12) == 16 and (f["raised"] >> 12) == 20 and f["steps"][0]["need"] == 21)
    add("the threshold follows the extension: one of two longer than 16 wins", P34, [20, 0, 0, 0, 18, 25, 0], ["one"],
        lambda f: f["pending"] and f["steps"][0]["need"] == 21 and f["best"] == _key(25, f["cands"][5]))
    add("the extension raised the younger of two eager candidates", P34, [16, 22, 0, 0, 22, 21, 23, 23], ["several"],
        lambda f: f["pending"] and f["steps"][0]["need"] == 23 and f["best"] == _key(23, f["cands"][6]))
    return cs


@functools.lru_cache(maxsize=None)
def _built():
    """[(name, unit, index of the chunk that holds the target, kinds of its finishing steps)]"""
    out = []
    text = np.frombuffer(b"abcabcabdabcabcab" * 300, dtype=np.uint8)[:4096]
    for i, (name, p, spec, kinds, check, kw) in enumerate(_cases()):
        c, f = _build(p, spec, 100 + 10 * i, **kw)
        assert f["finish"], name
        got = [_kind(s) for s in f["steps"]]
        assert got == kinds, "%s: the finishing steps take %s" % (name, got)
        assert check is None or check(f), (name, f["steps"], hex(f["best"]))
        out.append((name, c, 0, got))
        if i % 4 == 0:                                   # as the second chunk of a unit
            out.append((name + " (second chunk)", np.concatenate([text, c]), 1, got))
    return out


@pytest.mark.parametrize("step", ["first", "later"])
@pytest.mark.parametrize("kind", ["none", "one", "several"])
def test_units_cover_every_path(kind, step):
    cells = set()
    for _, _, _, kinds in _built():
        cells |= {(k, "first" if j == 0 else "later") for j, k in enumerate(kinds)}
    assert (kind, step) in cells


def test_units_are_one_or_two_chunks():
    assert all(len(u) <= 4096 * (1 + k) and k <= 1 for _, u, k, _ in _built())


_expected = {}


def _oracle_outputs(oracle, units):
    """the oracle's bytes of every unit, computed once for both modes"""
    if "out" not in _expected:
        out = []
        for i, u in enumerate(units):
            es, exp = oracle.oracle_compress(LZNT1, u)
            assert es == 0, (i, len(u), es)
            out.append(exp)
        _expected["out"] = out
    return _expected["out"]


def _chunk_is_compressed(stream, k):
    """whether chunk k of an LZNT1 stream is a compressed chunk (header bit 15), not a raw copy"""
    at = 0
    for _ in range(k):
        at += 2 + (((stream[at] | stream[at + 1] << 8) & 0xFFF) + 1)
    return bool(stream[at + 1] & 0x80)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
def test_lznt1_finishing_steps_best(oracle, gpu_ctx, mode):
    import ms_compress_amd as m
    built = _built()
    units = [u for _, u, _, _ in built]
    expected = _oracle_outputs(oracle, units)
    gpu_ctx.lib.mscomp_amd_debug_set_lznt1(mode)
    try:
        got, st = m.compress_units(LZNT1, list(units), ctx=gpu_ctx)
    finally:
        gpu_ctx.lib.mscomp_amd_debug_set_lznt1(0)
    for (name, u, k, _), g, s, exp in zip(built, got, st, expected):
        assert s == 0, (name, len(u), s)
        assert _chunk_is_compressed(exp, k), "%s: the target's chunk is stored raw and tests nothing" % name
        assert g == exp, "mode %d, %s (len %d): GPU bytes differ from the oracle (%d vs %d B)" % (mode, name, len(u), len(g), len(exp))
