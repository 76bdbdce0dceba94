"""The interior-window copy of LZNT1's window parse (csrc/lznt1.hip lz_window<true, true, true>) takes the token split -- shift, max_len and
max_len << 12 -- from the window's base on the scalar unit, and its first compare stage keeps no cap. Inside a window 64 w .. 64 w + 63 the
split changes at lane 0 alone and only where 64 w is a power of two, so windows 1, 2, 4, 8, 16 and 32 stay with the full-chunk copy, as
windows 0 and 63 do. The units here stand on every edge of that: lanes 0, 1 and 63 of the power-of-two windows and of their neighbours, each
with a repeat longer than the position's max_len (the token must carry exactly max_len: 1026 at position 64 and 514 at 65, 34 at 2048 and 18
at 2049); matches of exactly max_len and of max_len - 1; the 16-bit token itself, offset above `shift` bits of length, at the first and last
lane of the windows around every power-of-two window; a finishing event in a uniform window that ends because its winner reached max_len,
with candidates left behind; long-pending stops whose cooperative extension has to clamp to max_len 258 (window 3) and 18 (window 40); and
for the first stage without a cap: a lane whose candidate agrees on exactly 8 bytes, the one lane of its window that starts the second
stage, beside lanes whose first bucket entry is their own position (it agrees on every bit and does not exist as a candidate), and a window
in which no candidate that exists reaches 8 bytes, so that the second stage does not run over such lanes -- one of them a position with
exactly four older entries, its own the fifth. Every unit is a full chunk followed by the same shape in a last chunk of 4095 bytes, which
runs the body for any length. Every claim is asserted on the CPU model of tests/lznt1_model.py first, the oracle's token starts and lengths
must equal the model's, and the GPU test compares byte for byte with the oracle in both kernel modes through a host-table plan, a
device-table plan and the serial-atomics instance, guard bytes around every capacity."""
import functools

import numpy as np
import pytest

import lznt1_model as M
import lznt1_run as R

N = M.CHUNK
POW2 = (1, 2, 4, 8, 16, 32)                           # windows whose lane 0 has the larger split: not the interior copy's
INTERIOR = tuple(w for w in range(1, 63) if w not in POW2)
EDGE_WINDOWS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 62)
EDGE_POSITIONS = tuple(64 * w + l for w in EDGE_WINDOWS for l in (0, 1, 63)) + (200, 2569)    # and a stop inside windows 3 and 40
ENC_WINDOWS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33)     # both sides of every power-of-two window, and those windows


def _body_size(t):
    return (len(t) + 7) // 8 + sum(2 if L else 1 for L in t.values())


def _search(build, ok, seed, what):
    """the first of 40 seeded chunks that the model parses as claimed and that is not stored raw"""
    for s in range(40):
        c = build(seed + 7919 * s)
        t = M.parse(c)
        if ok(c, t) and _body_size(t) < len(c):
            return c
    raise AssertionError("no unit: " + what)


def _base(n, seed, lo, hi):
    """n bytes with distinct trigrams, [lo, hi) periodic (so that the chunk is not stored raw)"""
    c = M.filler(n, seed).copy()
    if hi > lo:
        c[lo:hi] = np.resize(M.filler(24, seed + 5), hi - lo)
    return c


def _plant(c, q, p, L):
    """a copy of L bytes from q at p that stops there: the byte behind it differs from the source's"""
    for i in range(L):
        c[p + i] = c[q + i]
    if p + L < len(c):
        c[p + L] = c[q + L] ^ 0x55


# ---- the split itself ------------------------------------------------------------------------------------------------------
def test_the_split_is_the_windows_outside_the_power_of_two_windows():
    """what the interior copy computes from the window's base, against the per-position rule of the model"""
    for w in range(1, 63):
        base = 64 * w
        shifts = {M.token_shift(base + l) for l in range(64)}
        if w in POW2:
            assert len(shifts) == 2 and M.token_shift(base) == M.token_shift(base + 1) + 1 and len({M.token_shift(base + l) for l in range(1, 64)}) == 1
            continue
        clz = 32 - base.bit_length()
        assert shifts == {clz - 16} and clz - 16 < 12
        assert all(M.max_len(N, base + l) == (1 << (clz - 16)) + 2 >= 18 for l in range(64))
    assert all(M.max_len(N, 64 * w + l) == 18 for w in range(33, 63) for l in range(64))
    assert [M.max_len(N, p) for p in (64, 65, 2048, 2049)] == [1026, 514, 34, 18]
    assert all(bool(w & (w - 1)) == (w not in POW2) for w in range(1, 63))     # LZ4_WINDOW's test


# ---- repeats longer than max_len ---------------------------------------------------------------------------------------------
def _pack(positions, n):
    """the positions dealt to chunks: in one chunk every repeat (max_len + 3 bytes) ends 12 bytes in front of the next one's source"""
    chunks = []
    for p in sorted(positions):
        for ch in chunks:
            if p - 7 >= ch[-1] + M.max_len(n, ch[-1]) + 3 + 12:
                ch.append(p)
                break
        else:
            chunks.append([p])
    return chunks


def _repeat_chunk(n, at, seed):
    """at every position of `at` a run of period 7 that goes on for three bytes beyond max_len: one candidate, 7 bytes back, which agrees on more
    than max_len -- it reaches 16 bytes in the eager scan, the stop is long-pending and the whole wave extends it, up to max_len and no further"""
    used = [(p - 7, p + M.max_len(n, p) + 4) for p in at]
    gaps = [(b + 16, a - 16) for (_, b), (a, _) in zip([(0, 0)] + used, used + [(n, n)])]
    lo, hi = max(gaps, key=lambda g: g[1] - g[0])              # the widest stretch between the repeats gets a periodic block: the chunk is not stored raw

    def build(s):
        c = _base(n, s, lo, hi)
        for p in at:
            L = M.max_len(n, p) + 3
            for i in range(L):
                c[p + i] = c[p - 7 + i]
            c[p + L] = c[p + L - 7] ^ 0x55
        return c

    def ok(c, t):
        for p in at:
            f = M.finish(c, p)
            ml = M.max_len(n, p)
            if not (t.get(p) == ml and p + ml in t and (p - 1 in t or p == 0) and M.lcp(c, p - 7, p, ml + 3) == ml + 3):
                return False
            if not (ml >= 18 and f["pending"] and (f["provisional"] >> 12) == 16 and (f["best"] >> 12) == f["maxl"] == ml):
                return False
        return True
    return _search(build, ok, seed, "repeats beyond max_len at %s" % (at,))


# ---- exactly max_len, and one byte less ----------------------------------------------------------------------------------------
EXACT = ((578, 66), (660, 65), (2565, 18), (2600, 17), (3970, 18), (4000, 17))     # windows 9, 10, 40 and 62: max_len 66, 66, 18, 18, 18, 18


def _exact_chunk(n, seed):
    def build(s):
        c = _base(n, s, 900, 2400)
        for i, (p, L) in enumerate(EXACT):
            _plant(c, 20 + 80 * i, p, L)
        return c

    def ok(c, t):
        return all(t.get(p) == L and t.get(p - 1) == 0 and M.lcp(c, 20 + 80 * i, p, L + 1) == L and M.max_len(len(c), p) - L == (i & 1) and p // 64 in INTERIOR
                   for i, (p, L) in enumerate(EXACT))
    return _search(build, ok, seed, "matches of max_len and max_len - 1")


# ---- the token -----------------------------------------------------------------------------------------------------------------
def _enc_positions(lane):
    """that lane of the windows around the power-of-two windows; of window 0 lane 63 alone (position 0 has no match)"""
    return tuple(64 * w + lane for w in ((0,) if lane else ()) + ENC_WINDOWS)


def _enc_offset(i):
    return 20 + 2 * i


def _enc_chunk(n, lane, seed):
    """matches of 3 to 7 bytes at one lane of the windows around the power-of-two windows, 20 to 46 bytes back"""
    at = _enc_positions(lane)

    def build(s):
        c = _base(n, s, 2300, 3900)
        for i, p in enumerate(at):
            _plant(c, p - _enc_offset(i), p, 3 + i % 5)
        return c
    return _search(build, lambda c, t: all(t.get(p) == 3 + i % 5 and t.get(p - 1) == 0 for i, p in enumerate(at)), seed, "match starts at lane %d" % lane)


def _match_tokens(stream):
    """{position: the 16-bit match token} of the first chunk of an LZNT1 stream"""
    hdr = stream[0] | (stream[1] << 8)
    assert hdr & 0x8000
    end, j, pos, out = 3 + (hdr & 0xFFF), 2, 0, {}
    while j < end:
        flags = stream[j]
        j += 1
        for b in range(8):
            if j >= end:
                break
            if (flags >> b) & 1:
                out[pos] = stream[j] | (stream[j + 1] << 8)
                pos += (out[pos] & ((1 << M.token_shift(pos)) - 1)) + 3
                j += 2
            else:
                pos += 1
                j += 1
    return out


# ---- one position with chosen older entries of its bucket ---------------------------------------------------------------------------
def _bucket_chunk(n, p, spec, seed, check):
    """A chunk whose position p has len(spec) older entries in its bucket, oldest first: 0 = a position of another key of the bucket, L >= 3 = a
    position that agrees with p on exactly L bytes (the builder of tests/test_gpu_lznt1_event.py, in a chunk of n bytes: a 24-byte block repeats
    between the candidates and the start of p's window, and again from the window behind p's to the chunk's end)"""
    ks = M.keys_of_bucket(M.BUCKET, M.NKEYS)
    assert len(spec) < M.NKEYS
    for s in range(80):
        sd = seed + 7919 * s
        c = M.filler(n, sd).copy()
        x = np.concatenate([np.frombuffer(ks[-1], dtype=np.uint8), M.filler(60, sd + 13)]).copy()
        at, where = 8, []
        for j, L in enumerate(spec):
            where.append(at)
            if L == 0:
                M.place(c, at, ks[j])
                at += 6
            else:
                M.place(c, at, x[:L])
                c[at + L] = x[L] ^ 0x55
                at += L + 4
        hi = p & ~63
        assert hi - (at + 8) >= 48, "no room for the repeats in front of position %d" % p
        c[at + 8:hi] = np.resize(M.filler(24, sd + 5), hi - (at + 8))
        M.place(c, p, x[:40])
        c[hi + 128:n] = np.resize(M.filler(24, sd + 7), n - (hi + 128))
        f = M.finish(c, p)
        if f["rank"] != len(spec) or f["cands"] != where or not all(l == w if w else l < 3 for l, w in zip(f["lens"], spec)):
            continue
        t = M.parse(c)
        if p not in t or t[p] != ((f["best"] >> 12) if (f["best"] >> 12) >= 3 else 0) or _body_size(t) >= n:
            continue
        if check(f, c, t):
            return c
    raise AssertionError("no unit for position %d, candidates %s" % (p, spec))


P_EVENT = M.P18                                       # 3000: window 46, max_len 18 in all 64 lanes
Z = [0]
EVENT_SPEC = Z * 4 + [0, 5, 0] + Z * 61 + [18] + Z * 70     # step 1 (entries 4 to 67) has a winner of 5 bytes, step 2 one of max_len; 7 entries wait for a third


def _event_ok(f, c, t):
    st = f["steps"]
    return (f["finish"] and len(st) == 2 and len(st[0]["winners"]) == 1 and st[0]["need"] == 3 and st[1]["need"] == 6 and len(st[1]["winners"]) == 1
            and st[1]["tail"] and (f["best"] >> 12) == f["maxl"] == 18 and f["left"] > 0 and P_EVENT // 64 in INTERIOR)


P_FIFTH = 2700                                        # window 42


def _eager(c, p):
    """(the common bytes, up to 16, of position p and its up to four oldest candidates; how many older entries its bucket holds)"""
    arr, slot, rank = M.bucket_model(c)
    r = int(rank[p])
    return [M.lcp(c, int(q), p, 16) for q in arr[slot[p] - r:slot[p]][:M.SELF]], r


def _window_stage2(c, w):
    """(lanes of window w with an existing candidate of 8 bytes or more: those that start the second stage; lanes with fewer than four older entries,
    whose own position is one of the four entries they compare: it agrees on every bit and does not exist)"""
    keys = [p for p in range(64 * w, 64 * w + 64) if p + 3 <= len(c)]
    e = {p: _eager(c, p) for p in keys}
    return [p for p in keys if any(l >= 8 for l in e[p][0])], [p for p in keys if e[p][1] < M.SELF]


def _fifth_ok(f, c, t):
    """position P_FIFTH has exactly four older entries, so its own is the fifth of its bucket, and no existing candidate of its window reaches 8 bytes"""
    trig, own = _window_stage2(c, P_FIFTH // 64)
    return f["rank"] == 4 and not f["finish"] and not trig and len(own) >= 50 and P_FIFTH not in own and P_FIFTH // 64 in INTERIOR


STAGE = ((1290, 8), (1407, 12))                       # window 20: the one lane with 8 bytes exactly; window 21: lane 63, 12 bytes


def _stage_chunk(n, seed):
    def build(s):
        c = _base(n, s, 1800, 3900)
        for i, (p, L) in enumerate(STAGE):
            _plant(c, 30 + 40 * i, p, L)
        return c

    def ok(c, t):
        for i, (p, L) in enumerate(STAGE):
            trig, own = _window_stage2(c, p // 64)
            if not (t.get(p) == L and trig == [p] and len(own) >= 50 and M.lcp(c, 30 + 40 * i, p, L + 1) == L and p // 64 in INTERIOR):
                return False
        return True
    return _search(build, ok, seed, "one lane that starts the second stage")


REPEAT_SETS = tuple(tuple(at) for at in _pack(EDGE_POSITIONS, N - 1))


# ---- the units ---------------------------------------------------------------------------------------------------------------------
def _shapes():
    """[(name, builder(n, seed))]"""
    out = []
    for k, at in enumerate(REPEAT_SETS):
        out.append(("repeats beyond max_len, set %d" % k, lambda n, s, at=at: _repeat_chunk(n, at, s)))
    out.append(("matches of max_len and of max_len - 1", _exact_chunk))
    out.append(("tokens at lane 0", lambda n, s: _enc_chunk(n, 0, s)))
    out.append(("tokens at lane 63", lambda n, s: _enc_chunk(n, 63, s)))
    out.append(("an event that ends on max_len", lambda n, s: _bucket_chunk(n, P_EVENT, EVENT_SPEC, s, _event_ok)))
    out.append(("no candidate of the window reaches 8 bytes", lambda n, s: _bucket_chunk(n, P_FIFTH, Z * 4, s, _fifth_ok)))
    out.append(("one lane starts the second stage", _stage_chunk))
    return out


@functools.lru_cache(maxsize=None)
def _built():
    """[(name, unit bytes, (full chunk, last chunk of 4095 bytes))]"""
    out = []
    for i, (name, build) in enumerate(_shapes()):
        a, b = build(N, 1000 + 20 * i), build(N - 1, 1010 + 20 * i)
        assert len(a) == N and len(b) == N - 1
        out.append((name, a.tobytes() + b.tobytes(), (a, b)))
    return out


def test_units_are_what_they_claim():
    built = {name: chunks for name, _, chunks in _built()}            # (the builders assert their claims on the model)
    assert all(len(u) == 2 * N - 1 for _, u, _ in _built())
    assert sorted(p for at in REPEAT_SETS for p in at) == sorted(EDGE_POSITIONS) and len(set(EDGE_POSITIONS)) == len(EDGE_POSITIONS)
    took = {}
    for k, at in enumerate(REPEAT_SETS):
        for c in built["repeats beyond max_len, set %d" % k]:
            t = M.parse(c)
            for p in at:
                assert t[p] == M.max_len(len(c), p) and p + t[p] in t, (k, p)
                took[p] = t[p]
    assert (took[64], took[65], took[2048], took[2049]) == (1026, 514, 34, 18)
    assert took[200] == 258 and took[2569] == 18 and 200 // 64 == 3 and 2569 // 64 == 40     # the long-pending stops of windows 3 and 40
    for lane in (0, 63):                              # every power-of-two window has a token on each side
        ws = {p // 64 for p in _enc_positions(lane)}
        assert all((w - 1 in ws or (w, lane) == (1, 0)) and w + 1 in ws for w in POW2)


def test_the_oracle_parses_the_units_as_the_model_does(oracle):
    for name, u, chunks in _built():
        streams = M.chunk_streams(R.expected(oracle, u))
        assert len(streams) == 2, name
        for k, (st, c) in enumerate(zip(streams, chunks)):
            assert st[1] & 0x80, "%s: chunk %d is stored raw and tests nothing" % (name, k)
            assert M.token_lengths(st) == M.parse(c), (name, k)


def test_the_oracles_tokens_carry_the_offset_above_shift_bits_of_length(oracle):
    built = {name: (u, chunks) for name, u, chunks in _built()}
    for lane in (0, 63):
        u, chunks = built["tokens at lane %d" % lane]
        for st, c in zip(M.chunk_streams(R.expected(oracle, u)), chunks):
            toks = _match_tokens(st)
            for i, p in enumerate(_enc_positions(lane)):
                sh = M.token_shift(p)
                if p // 64 in INTERIOR:                  # the split the interior copy makes of the window's base
                    assert sh == 32 - (64 * (p // 64)).bit_length() - 16
                assert toks[p] == ((_enc_offset(i) - 1) << sh) | (3 + i % 5 - 3), (lane, p, hex(toks[p]))


@pytest.mark.gpu
@pytest.mark.parametrize("path", R.PATHS)
@pytest.mark.parametrize("mode", [1, 2])
def test_lznt1_window_split(oracle, gpu_ctx, mode, path):
    built = _built()
    R.check_plan(oracle, gpu_ctx, [u for _, u, _ in built], mode, path, "window split", names=[name for name, _, _ in built])
