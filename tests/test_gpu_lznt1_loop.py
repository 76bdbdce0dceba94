"""The window loops of the four-wave LZNT1 kernel (csrc/lznt1.hip lznt1_chunk4_kernel) run on the scalar unit: the window number, the parse
position, the "window already behind the position" test, the recorded positions a seam repair compares with and the loops' back edges are
wave-uniform. The units here walk those loops' edges: a match that covers one, two and twenty whole windows (the skip path), a match that ends
exactly at a window's end and one byte behind it, chunks of 1, 21, 22, 38, 52 and 64 windows (the segment boundaries and their neighbours),
two chunks in which a match crosses every segment boundary (all three seams repaired), and one adversarial chunk whose speculative parse of
segment 1 never meets the true one, so that the repair runs through the whole segment and wave 0's cascade re-walk takes over behind it.
Every claim is shown on the CPU model of the bucket array that tests/lznt1_model.py keeps (the speculative parse of a segment is the
same greedy parse started at the segment's first position); the oracle's token starts and lengths must equal the model's, and the GPU tests
compare byte for byte with the oracle in both kernel modes through a host-table plan, a device-table plan and the serial-atomics instance."""
import functools

import numpy as np
import pytest

import lznt1_model as M
import lznt1_run as R

SEG = M.SEG_FIRST_WINDOW                             # first windows of the segments, and the chunk's end


def _text(n, seed):
    """n bytes of words drawn from a small dictionary: short matches everywhere, full buckets, finishing steps"""
    r = np.random.default_rng(seed)
    words = [bytes(r.integers(97, 123, int(r.integers(3, 13)), dtype=np.uint8)) for _ in range(40)]
    out = bytearray()
    while len(out) < n:
        out += words[int(r.integers(0, 40))] + b" "
    return np.frombuffer(bytes(out[:n]), np.uint8).copy()


def _periodic(c, p, L, d=7):
    """a match of exactly L bytes at p, d bytes back (the source overlaps the target)"""
    for i in range(L):
        c[p + i] = c[p - d + i]
    c[p + L] = c[p + L - d] ^ 0x55


def _after_windows(c, entry, w0, w1):
    """the greedy parse from `entry` over windows [w0, w1): the parse position after each window, as the kernel records it"""
    match = M.greedy_match(c)
    out, p = [], entry
    for w in range(w0, w1):
        wend = min(64 * w + 64, len(c))
        while p < wend:
            p += match(p) or 1
        out.append(p)
    return out


def _skip_unit(windows, seed):
    """a match that covers `windows` whole windows; returns (chunk, its start, its length)"""
    for s in range(40):
        c = M.filler(2200, seed + 7919 * s).copy()
        p, L = (124, 64 * windows + 10) if windows <= 2 else (17, 64 * windows + 80)   # (max_len 514 at 124, 2050 at 17)
        _periodic(c, p, L)
        c[p + L + 40:] = np.resize(M.filler(24, seed + 5), len(c) - (p + L + 40))
        t = M.parse(c)
        whole = [w for w in range(len(c) // 64) if p < 64 * w and 64 * w + 64 <= p + L]
        if t.get(p) == L and len(whole) == windows and (p + L) % 64 not in (0, 1):
            return c, p, L
    raise AssertionError("no unit with a match over %d windows" % windows)


def _end_unit(behind, seed):
    """a match that ends exactly at a window's end (behind = 0) or one byte behind it (1)"""
    for s in range(40):
        c = M.filler(1024, seed + 7919 * s).copy()
        p = 300
        L = 320 + behind - p
        _periodic(c, p, L)
        c[400:] = np.resize(M.filler(24, seed + 5), len(c) - 400)
        t = M.parse(c)
        if t.get(p) == L and (p + L) % 64 == behind:
            return c, p, L
    raise AssertionError("no unit")


def _seams_unit(seed):
    """two chunks of text in which a match crosses every segment boundary"""
    for s in range(200):
        u = _text(8192, seed + s)
        ok = True
        for k in range(2):
            t = M.parse(u[4096 * k: 4096 * k + 4096])
            ok = ok and all(64 * w not in t for w in SEG[1:4])
        if ok:
            return u
    raise AssertionError("no text whose matches cross all seams")


def _cascade_unit(seed):
    """filler, then one byte repeated from position 1100 on: back-to-back matches of max_len, so a parse that starts at another position never
    meets the true one. The speculative parse of segment 1 (from position 64 * 21) differs from the true parse behind EVERY window of the segment."""
    c = M.filler(4096, seed).copy()
    c[1100:] = 0x41
    true = _after_windows(c, 0, 0, 64)
    spec = _after_windows(c, 64 * SEG[1], SEG[1], SEG[2])
    assert all(a != b for a, b in zip(spec, true[SEG[1]:SEG[2]])), "the speculative parse of segment 1 meets the true one"
    spec2 = _after_windows(c, 64 * SEG[2], SEG[2], SEG[3])
    assert spec2[0] != true[SEG[2]], "nothing left for the cascade behind the repaired segment"
    return c


@functools.lru_cache(maxsize=None)
def _built():
    """[(name, unit bytes)]"""
    out = []
    for wn in (1, 2, 20):
        c, p, L = _skip_unit(wn, 100 + wn)
        out.append(("a match over %d whole windows" % wn, c.tobytes()))
    for b in (0, 1):
        out.append(("a match that ends %d bytes behind a window's end" % b, _end_unit(b, 300 + b)[0].tobytes()))
    for wn in (1, 21, 22, 38, 52, 64):
        out.append(("a chunk of %d windows" % wn, _text(64 * wn - (5 if wn in (22, 52) else 0), 400 + wn).tobytes()))
    out.append(("two chunks, all three seams repaired", _seams_unit(500).tobytes()))
    out.append(("a repair through a whole segment, then the cascade", _cascade_unit(600).tobytes()))
    return out


def _expected(oracle):
    return {name: R.expected(oracle, u) for name, u in _built()}


def test_units_are_what_they_claim():
    built = _built()                                 # (the builders assert their claims on the model)
    assert len(built) == 13 and all(0 < len(u) <= 8192 for _, u in built)
    assert [len(u) for n_, u in built[5:11]] == [64, 1344, 1403, 2432, 3323, 4096]


def test_the_oracle_parses_the_units_as_the_model_does(oracle):
    for name, u in _built():
        streams = M.chunk_streams(_expected(oracle)[name])
        assert len(streams) == (len(u) + 4095) // 4096, name
        for k, st in enumerate(streams):
            assert st[1] & 0x80, "%s: chunk %d is stored raw and tests nothing" % (name, k)
            assert M.token_lengths(st) == M.parse(np.frombuffer(u[4096 * k: 4096 * (k + 1)], np.uint8)), (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("path", R.PATHS)
@pytest.mark.parametrize("mode", [1, 2])
def test_lznt1_window_loops(oracle, gpu_ctx, mode, path):
    built = _built()
    R.check_plan(oracle, gpu_ctx, [u for _, u in built], mode, path, "window loops", names=[name for name, _ in built])
