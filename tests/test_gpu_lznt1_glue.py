"""The glue of the four-wave LZNT1 kernel's window loops (csrc/lznt1.hip lznt1_chunk4_kernel): a window's two arms -- skipped, because a match
covers it whole, or parsed -- only produce the token mask, the match mask and the parse position, and one store sequence behind their join writes
the control words, every lane the same value; and the speculative parse of a full chunk runs windows 1 to 62 through a copy of the window code
without the edges only windows 0 and 63 have (position 0, the lanes that are no keys, a max_len the chunk's end cuts or that lies below 18).
The units here, each at most two chunks, walk what that touches: a match from position 8 that covers every window up to a segment's last (20,
37, 51) and up to the next segment's first (21, 38, 52), so the skip arm runs for many windows in a row, in the speculative loop and in the seam
repair; chunks whose speculative parse of segment 1 differs from the true one for one window, for two, for eleven and for the whole segment
(seam repair, a long repair, the cascade); match starts at lanes 0 and 63 of windows 0, 1, 31, 32, 62 and 63, literal token starts at position 0
and 4095, a match at position 1; matches whose max_len the chunk's end cuts (18, 17, 6 and 3 bytes in front of the end), a match of max_len 18
from window 62 into window 63; matches of exactly 8, 16, 17 and 18 bytes at the first and last position of interior windows; and the same
shapes in a last chunk of 4095 bytes and in one of 65 bytes, which run the body for any length. Every claim is asserted on the CPU model of
tests/lznt1_model.py first, the oracle's token starts and lengths must equal the model's, and the GPU test compares byte for byte with the
oracle in both kernel modes through a host-table plan, a device-table plan and the serial-atomics instance, guard bytes around every capacity."""
import functools

import numpy as np
import pytest

import lznt1_model as M
import lznt1_run as R

N = M.CHUNK
SEG = M.SEG_FIRST_WINDOW


def _base(n, seed, lo, hi):
    """n bytes with distinct trigrams, [lo, hi) periodic (so that the chunk is not stored raw): elsewhere every token is a literal until a builder
    plants a copy"""
    c = M.filler(n, seed).copy()
    c[lo:hi] = np.resize(M.filler(24, seed + 5), hi - lo)
    return c


def _plant(c, q, p, L):
    """a copy of L bytes from q at p that stops there: the byte behind it differs from the source's"""
    for i in range(L):
        c[p + i] = c[q + i]
    if p + L < len(c):
        c[p + L] = c[q + L] ^ 0x55


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


def _after_windows(c, entry, w0, w1):
    """the greedy parse from `entry` over windows [w0, w1): (the parse position after each window, as the kernel records it; the token starts)"""
    match = M.greedy_match(c)
    out, starts, p = [], set(), entry
    for w in range(w0, w1):
        wend = min(64 * w + 64, len(c))
        while p < wend:
            starts.add(p)
            p += match(p) or 1
        out.append(p)
    return out, starts


def _repair_walk(c, j):
    """(windows the repair of the seam in front of segment j walks until the position behind a window equals the speculative parse's -- through
    segment j at the most --, whether it met it, whether the two parses' token starts differ in the first window)"""
    nw = (len(c) + 63) // 64
    true, tstarts = _after_windows(c, 0, 0, nw)
    entry = true[SEG[j] - 1]
    if entry == 64 * SEG[j]:
        return 0, True, False
    last = min(SEG[j + 1], nw)
    spec, sstarts = _after_windows(c, 64 * SEG[j], SEG[j], last)
    w0 = range(64 * SEG[j], 64 * SEG[j] + 64)
    differ = {p for p in tstarts if p in w0} != {p for p in sstarts if p in w0}
    for k, w in enumerate(range(SEG[j], last)):
        if true[w] == spec[k]:
            return k + 1, True, differ
    return last - SEG[j], False, differ


# ---- the skip arm ----------------------------------------------------------------------------------------------------------
def _skip_unit(n, last, seed):
    """a match at position 8, 7 bytes back, that ends 30 bytes into window last + 1: windows 1 to `last` are covered whole"""
    p, L = 8, 64 * (last + 1) + 30 - 8

    def build(s):
        c = M.filler(n, s).copy()
        for i in range(L):
            c[p + i] = c[p - 7 + i]
        c[p + L] = c[p + L - 7] ^ 0x55
        return c

    def ok(c, t):
        return t.get(p) == L and M.max_len(len(c), p) > L and all(t.get(i) == 0 for i in range(p)) and p + L in t
    return _search(build, ok, seed, "a match over windows 1 to %d" % last)


# ---- speculative parse and true parse apart ----------------------------------------------------------------------------------
def _run_unit(n, lo, hi, seed):
    """one byte value over [lo, hi) around the first position of segment 1 (1344): back-to-back matches of max_len 34 from lo + 1 on in the true
    parse, from 1344 on in the speculative one, out of step until the run ends. [2500, 3300) is periodic, inside segment 2."""
    def build(s):
        c = _base(n, s, 2500, 3300)
        c[lo:hi] = 0x41
        return c
    return _search(build, lambda c, t: t.get(lo + 1) == 34 and t.get(lo) == 0, seed, "a run over [%d, %d)" % (lo, hi))


def _cascade_unit(n, seed):
    """one byte value from 1100 to the end: the speculative parse of segment 1 never meets the true one, the repair runs through the whole segment
    and wave 0's cascade takes over behind it"""
    c = M.filler(n, seed).copy()
    c[1100:] = 0x41
    return c


# ---- lanes 0 and 63 ----------------------------------------------------------------------------------------------------------
LANES_A = (63, 127, 2047, 2111, 4031)          # match starts, chunk A: lane 63 of windows 0, 1, 31, 32 and 62
LANES_B = (64, 1984, 2048, 3968, 4032)         # chunk B: lane 0 of windows 1, 31, 32, 62 and 63


def _lanes_unit(n, at, seed):
    """matches of 3 to 7 bytes at the given positions, sources from 10 on, and a match of 3 at position 1 (bytes 0..3 alike)"""
    def build(s):
        c = _base(n, s, 2200, 3900)
        c[0:4] = c[0]
        c[4] = c[0] ^ 0x55
        for i, p in enumerate(at):
            _plant(c, 10 + 8 * i, p, 3 + i)
        return c

    def ok(c, t):
        return t.get(0) == 0 and t.get(1) == 3 and all(t.get(p) == 3 + i and t.get(p - 1) == 0 for i, p in enumerate(at)) and (len(c) - 1 in t) == (len(c) - 1 not in range(at[-1], at[-1] + 7))
    return _search(build, ok, seed, "match starts at %s" % (at,))


# ---- the chunk's end -----------------------------------------------------------------------------------------------------------
def _cut_unit(n, back, seed):
    """a match `back` bytes in front of the chunk's end whose source goes on: max_len is what the chunk has left"""
    p = n - back

    def build(s):
        c = _base(n, s, 300, 2300)
        _plant(c, 150, p, back)
        return c
    return _search(build, lambda c, t: t.get(p) == back == M.max_len(len(c), p) and t.get(p - 1) == 0, seed, "a match %d bytes in front of the end" % back)


def _w62_unit(n, seed):
    """a match of max_len 18 at 4020 (window 62) that ends at 4038 (window 63); the source agrees on a 19th byte"""
    def build(s):
        c = _base(n, s, 300, 2300)
        _plant(c, 150, 4020, 19)
        return c
    return _search(build, lambda c, t: t.get(4020) == 18 == M.max_len(len(c), 4020) and M.lcp(c, 150, 4020, 19) == 19 and t.get(4019) == 0 and 4038 in t,
                   seed, "max_len 18 from window 62 into 63")


# ---- the compare stages' caps --------------------------------------------------------------------------------------------------
AGREE = ((640, 16), (703, 8), (2560, 8), (2623, 16), (2880, 18), (2943, 17), (3200, 17), (3263, 18))   # lanes 0 and 63 of windows 10, 40, 45 and 50


def _agree_unit(n, seed):
    """matches of exactly 8, 16, 17 and 18 bytes at the first and last position of interior windows (max_len 66 at 640 and 703, 18 from 2560 on)"""
    def build(s):
        c = _base(n, s, 900, 2400)
        for i, (p, L) in enumerate(AGREE):
            _plant(c, 20 + 24 * i, p, L)
        return c

    def ok(c, t):
        return all(t.get(p) == L and t.get(p - 1) == 0 and M.lcp(c, 20 + 24 * i, p, L + 1) == L for i, (p, L) in enumerate(AGREE) if p + L < len(c))
    return _search(build, ok, seed, "agreements of 8, 16, 17 and 18 bytes")


# ---- 65 bytes ------------------------------------------------------------------------------------------------------------------
def _tiny_unit(covered, seed):
    """65 bytes: a match of 3 at position 1, one of 40 at 10, and a match that ends at the chunk's end -- at 62 (max_len 3: window 1, the one
    position 64, is covered and skipped) -- or at 60 of 4 bytes, so that position 64 is a literal token at lane 0 of window 1"""
    def build(s):
        c = M.filler(65, s).copy()
        c[0:4] = c[0]
        c[4] = c[0] ^ 0x55
        for i in range(40):
            c[10 + i] = c[5 + i]
        c[50] = c[45] ^ 0x55
        if covered:
            _plant(c, 52, 62, 3)
        else:
            _plant(c, 52, 60, 4)
        return c

    def ok(c, t):
        return t.get(1) == 3 and t.get(10) == 40 and (t.get(62) == 3 and 64 not in t and M.max_len(65, 62) == 3 if covered else t.get(60) == 4 and t.get(64) == 0)
    return _search(build, ok, seed, "65 bytes")


@functools.lru_cache(maxsize=None)
def _built():
    """[(name, unit bytes)]: full chunks first, then the same shapes as units that end in a chunk of 4095 bytes, then 65 bytes"""
    out = []
    for last in (20, 21, 37, 38, 51, 52):
        out.append(("a match over windows 1 to %d" % last, _skip_unit(N, last, 100 + last).tobytes()))
    out.append(("speculative and true parse apart for one window", _run_unit(N, 1300, 1400, 200).tobytes()))
    out.append(("apart for two windows", _run_unit(N, 1300, 1460, 210).tobytes()))
    out.append(("apart for eleven windows", _run_unit(N, 1300, 2000, 220).tobytes()))
    out.append(("apart for a whole segment, then the cascade", _cascade_unit(N, 230).tobytes()))
    out.append(("match starts at lane 63 of windows 0, 1, 31, 32, 62 | at lane 0 of windows 1, 31, 32, 62, 63",
                _lanes_unit(N, LANES_A, 300).tobytes() + _lanes_unit(N, LANES_B, 310).tobytes()))
    out.append(("max_len cut at 4078 | at 4079", _cut_unit(N, 18, 400).tobytes() + _cut_unit(N, 17, 410).tobytes()))
    out.append(("max_len cut at 4090 | at 4093", _cut_unit(N, 6, 420).tobytes() + _cut_unit(N, 3, 430).tobytes()))
    out.append(("max_len 18 from window 62 into window 63", _w62_unit(N, 500).tobytes()))
    out.append(("agreements of 8, 16, 17 and 18 bytes at lanes 0 and 63", _agree_unit(N, 600).tobytes()))
    # a last chunk of 4095 bytes behind a full one
    n = N - 1
    out.append(("4095: a match over windows 1 to 21 | to 52", _skip_unit(N, 21, 121).tobytes() + _skip_unit(n, 52, 700).tobytes()))
    out.append(("4095: apart for two windows | then the cascade", _run_unit(N, 1300, 1460, 210).tobytes() + _cascade_unit(n, 710).tobytes()))
    out.append(("4095: apart for one window", _run_unit(n, 1300, 1400, 720).tobytes()))
    out.append(("4095: match starts at lane 63", _lanes_unit(n, LANES_A, 730).tobytes()))
    out.append(("4095: match starts at lane 0", _lanes_unit(n, LANES_B, 740).tobytes()))
    out.append(("4095: max_len cut 18 in front of the end", _cut_unit(n, 18, 750).tobytes()))
    out.append(("4095: max_len cut 17 | 6 in front of the end", _cut_unit(N, 17, 410).tobytes() + _cut_unit(n, 6, 760).tobytes()))
    out.append(("4095: max_len cut 3 in front of the end", _cut_unit(n, 3, 770).tobytes()))
    out.append(("4095: max_len 18 from window 62 into window 63", _w62_unit(n, 780).tobytes()))
    out.append(("4095: agreements", _agree_unit(n, 790).tobytes()))
    out.append(("65: window 1 covered", _tiny_unit(True, 800).tobytes()))
    out.append(("65: a literal at position 64", _tiny_unit(False, 810).tobytes()))
    out.append(("4096 + 65", _agree_unit(N, 600).tobytes() + _tiny_unit(True, 800).tobytes()))
    return out


def _chunks(u):
    return [np.frombuffer(u[k:k + N], np.uint8) for k in range(0, len(u), N)]


def test_units_are_what_they_claim():
    built = dict(_built())                            # (the builders assert their claims on the model)
    assert all(0 < len(u) <= 2 * N for u in built.values())
    assert sorted({len(u) % N for u in built.values()}) == [0, 65, N - 1]
    # the skip arm: windows 1 to `last` lie inside the match; `last` is a segment's last window or the next segment's first
    for last in (20, 21, 37, 38, 51, 52):
        c = _chunks(built["a match over windows 1 to %d" % last])[0]
        t = M.parse(c)
        assert 8 + t[8] == 64 * (last + 1) + 30 and (last in SEG or last + 1 in SEG)
        assert not any(64 <= p < 64 * (last + 1) for p in t)
    # the seam in front of segment 1: how many windows the repair walks, and that the two parses differ in the first of them
    for name, walked, met in (("speculative and true parse apart for one window", 1, True), ("apart for two windows", 2, True), ("apart for eleven windows", 11, True),
                              ("apart for a whole segment, then the cascade", SEG[2] - SEG[1], False)):
        c = _chunks(built[name])[0]
        k, m, differ = _repair_walk(c, 1)
        assert (k, m, differ) == (walked, met, True), (name, k, m, differ)
    c = _chunks(built["apart for a whole segment, then the cascade"])[0]
    assert _repair_walk(c, 2)[0] > 0, "nothing left for the cascade behind the repaired segment"
    for name in ("4095: apart for one window",):
        assert _repair_walk(_chunks(built[name])[0], 1) == (1, True, True)
    assert _repair_walk(_chunks(built["4095: apart for two windows | then the cascade"])[1], 1)[:2] == (SEG[2] - SEG[1], False)
    # lanes: every listed window has a match start at lane 0 and one at lane 63 (window 0: a literal at lane 0, window 63: a literal at lane 63)
    a, b = (M.parse(c) for c in _chunks(built["match starts at lane 63 of windows 0, 1, 31, 32, 62 | at lane 0 of windows 1, 31, 32, 62, 63"]))
    assert all(a[64 * w + 63] >= 3 for w in (0, 1, 31, 32, 62)) and all(b[64 * w] >= 3 for w in (1, 31, 32, 62, 63))
    assert a[0] == 0 and a[1] == 3 and a[4095] == 0 and b[0] == 0 and b[1] == 3
    for p, L in AGREE:                                 # interior windows all
        assert 1 <= p // 64 <= 62 and p % 64 in (0, 63) and L in (8, 16, 17, 18) and M.max_len(N, p) >= 18


def test_the_oracle_parses_the_units_as_the_model_does(oracle):
    for name, u in _built():
        streams = M.chunk_streams(R.expected(oracle, u))
        assert len(streams) == (len(u) + N - 1) // N, name
        for k, (st, c) in enumerate(zip(streams, _chunks(u))):
            assert st[1] & 0x80, "%s: chunk %d is stored raw and tests nothing" % (name, k)
            assert M.token_lengths(st) == M.parse(c), (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("path", R.PATHS)
@pytest.mark.parametrize("mode", [1, 2])
def test_lznt1_window_glue(oracle, gpu_ctx, mode, path):
    built = _built()
    R.check_plan(oracle, gpu_ctx, [u for _, u in built], mode, path, "window glue", names=[name for name, _ in built])
