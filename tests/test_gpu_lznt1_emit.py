"""Section D of the four-wave LZNT1 kernel (csrc/lznt1.hip lznt1_chunk4_kernel): the emission loop reads its control words -- a window's token
mask and match mask, the tokens and token bytes in front of it -- from the lanes with v_readlane, tests and branches on the scalar unit, runs
ONE region under the token mask (literal byte and token word read unconditionally, the low byte selected by the match mask, the match lanes'
high byte and flag bit inside it) and stores through global pointers with a scalar base. The units here stand on the loop's edges: a window with
no token, one with 64 literal tokens, one whose only token is a match at lane 0 and one at lane 63; flag groups (8 tokens) that straddle a
window seam and the seams between the waves' pieces (windows 16, 32, 48); chunks whose token count is a multiple of 8 and one more; the
largest number of matches a window can hold (22: 21 of 3 bytes and one at lane 63) in the first and the last window of a wave's piece; chunks
stored raw with n + 2 at every residue modulo 4 and n of 1, 2 and 3; and the recipes of tests/golden/thresholds.json that lie one byte under
the raw threshold and on it. Every case is placed on the CPU model that tests/lznt1_model.py keeps and asserted there first; the oracle's token
starts and lengths must equal the model's, and the GPU tests compare byte for byte with the oracle in both kernel modes through a host-table
plan, a device-table plan and the serial-atomics instance (guard bytes around every capacity: lznt1_run.run_plan)."""
import functools

import numpy as np
import pytest

import lznt1_model as M
import lznt1_run as R
import thresholds as TH

PIECE = 16                                           # windows per wave in the emission


def _windows(c):
    """per window of the chunk: (tokens that start in it, matches among them, tokens in front of it) on the model's parse"""
    t = M.parse(c)
    out, before = [], 0
    for w in range((len(c) + 63) // 64):
        tk = [p for p in t if 64 * w <= p < 64 * w + 64]
        out.append((len(tk), sum(1 for p in tk if t[p]), before))
        before += len(tk)
    return t, out


def _compressible(c, lo, hi, seed):
    c[lo:hi] = np.resize(M.filler(24, seed), hi - lo)


def _copy(c, q, p, L):
    for i in range(L):
        c[p + i] = c[q + i]


def _lanes_unit(seed):
    """window 2 (positions 128..191) without a token: a match from 124 on covers it. Window 8 (512..575): its only token a match at lane 0.
    Window 10 (640..703): its only token a match at lane 63. Window 20: 64 literals."""
    for s in range(60):
        c = M.filler(4096, seed + 7919 * s).copy()
        for i in range(100):                                  # a match of exactly 100 bytes at 124, 7 back (max_len 258)
            c[124 + i] = c[117 + i]
        c[224] = c[217] ^ 0x55
        _copy(c, 20, 512, 70)                                 # 512..581 from 20: lane 0 of window 8, over the whole window (max_len 130 there)
        c[582] = c[90] ^ 0x55
        _copy(c, 240, 638, 65)                                # 638..702: covers lanes 0..62 of window 10 (max_len 66 there)
        _copy(c, 330, 703, 9)                                 # a match at lane 63
        c[712] = c[339] ^ 0x55
        _compressible(c, 2000, 3900, seed + 5)
        t, wins = _windows(c)
        first10 = [p for p in t if 640 <= p < 704]
        if (t.get(124) == 100 and wins[2][0] == 0 and wins[8][:2] == (1, 1) and t.get(512) == 70
                and first10 == [703] and t.get(703) == 9 and wins[20][:2] == (64, 0)):
            return c
    raise AssertionError("no unit for the lane cases")


def _text(n, seed):
    r = np.random.default_rng(seed)
    words = [bytes(r.integers(97, 123, int(r.integers(3, 13)), dtype=np.uint8)) for _ in range(40)]
    out = bytearray()
    while len(out) < n:
        out += words[int(r.integers(0, 40))] + b" "
    return np.frombuffer(bytes(out[:n]), np.uint8).copy()


def _seam_unit(seed):
    """text: a flag group straddles the seams in front of windows 16, 32 and 48 (and some seam inside a piece), with tokens on both sides"""
    for s in range(200):
        c = _text(4096, seed + s)
        _, wins = _windows(c)
        if all(wins[w][2] % 8 not in (0,) and wins[w][0] and wins[w - 1][0] and (wins[w][2] % 8) + wins[w][0] >= 8 for w in (16, 32, 48)) \
                and any(wins[w][2] % 8 and wins[w][0] for w in range(1, 16)):
            return c
    raise AssertionError("no text whose flag groups straddle the piece seams")


def _count_unit(rem, seed):
    """a chunk whose token count is rem modulo 8: literals behind a periodic stretch, the length chosen"""
    c = M.filler(2300, seed).copy()
    _compressible(c, 300, 2000, seed + 5)
    for n in range(2200, 2300):
        t = M.parse(c[:n])
        if len(t) % 8 == rem:
            return c[:n].copy()
    raise AssertionError("no length with %d tokens modulo 8" % rem)


def _full_window_unit(ws, seed):
    """22 matches start in each window of ws: 21 of exactly 3 bytes from the window's first position on, and one at lane 63"""
    for s in range(200):
        c = M.filler(4096, seed + 7919 * s).copy()
        _compressible(c, 100, 900, seed + 5)                  # (so that the chunk is not stored raw)
        bank = 910
        for w in ws:
            for k in range(22):                               # trigram k of the window from the bank, five bytes apart
                _copy(c, bank, 64 * w + 3 * k, 3)
                bank += 5
        t, wins = _windows(c)
        if all(wins[w][:2] == (22, 22) and all(t.get(64 * w + 3 * k) == 3 for k in range(22)) for w in ws):
            return c
    raise AssertionError("no unit with 22 matches in windows %s" % (ws,))


def _raw_units():
    """incompressible units: n of 1, 2, 3 and n + 2 at every residue modulo 4, short and long"""
    return [("raw, n = %d" % n, M.filler(n, 900 + n).tobytes()) for n in (1, 2, 3, 30, 31, 32, 33, 4093, 4094, 4095, 4096)]


THRESHOLD_IDS = ("lznt1-1000-only-d-1-s43000", "lznt1-1000-only-d+0-s43003", "lznt1-4096-only-d-1-s45004", "lznt1-4096-only-d+0-s45002")


@functools.lru_cache(maxsize=None)
def _built():
    """[(name, unit bytes, stored raw?)]"""
    out = [("windows without a token, with a match at lane 0 / 63 alone, with 64 literals", _lanes_unit(100).tobytes(), False),
           ("flag groups across the piece seams", _seam_unit(200).tobytes(), False),
           ("token count 0 modulo 8", _count_unit(0, 300).tobytes(), False),
           ("token count 1 modulo 8", _count_unit(1, 301).tobytes(), False),
           ("22 matches in windows 16 and 31", _full_window_unit((16, 31), 400).tobytes(), False),
           ("22 matches in windows 32 and 47", _full_window_unit((32, 47), 401).tobytes(), False)]
    out += [(name, u, True) for name, u in _raw_units()]
    cases = {c["id"]: c for c in TH.load()["cases"]}
    for i in THRESHOLD_IDS:
        out.append((i, TH.build(cases[i]), cases[i]["want"] >= 0))
    return out


def test_units_are_what_they_claim():
    built = _built()                                 # (the builders assert their claims on the model)
    assert len(built) == 6 + 11 + 4
    assert sorted({(len(u) + 2) % 4 for name, u, raw in built if raw and name.startswith("raw")}) == [0, 1, 2, 3]
    assert M.MAXM == 22 and PIECE * 4 == 64
    assert len(M.parse(np.frombuffer(built[2][1], np.uint8))) % 8 == 0 and len(M.parse(np.frombuffer(built[3][1], np.uint8))) % 8 == 1


def test_the_oracle_parses_the_units_as_the_model_does(oracle):
    for name, u, raw in _built():
        streams = M.chunk_streams(R.expected(oracle, u))
        assert len(streams) == 1, name
        assert bool(streams[0][1] & 0x80) == (not raw), name
        if raw:
            assert streams[0][2:] == u, name
        else:
            assert M.token_lengths(streams[0]) == M.parse(np.frombuffer(u, np.uint8)), name


@pytest.mark.gpu
@pytest.mark.parametrize("path", R.PATHS)
@pytest.mark.parametrize("mode", [1, 2])
def test_lznt1_emission(oracle, gpu_ctx, mode, path):
    built = _built()
    R.check_plan(oracle, gpu_ctx, [u for _, u, _ in built], mode, path, "emission", names=[name for name, _, _ in built])
