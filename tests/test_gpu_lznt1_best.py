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

import lznt1_model as M
import lznt1_run as R
from lznt1_model import NKEYS, P18, P34, best_key as _key, filler as _filler, finish as _finish, place as _place


def _kind(step):
    return ("none", "one", "several")[min(len(step["winners"]), 2)]


def _build(p, spec, seed, cut=None):
    """A chunk whose position p has len(spec) older entries in its bucket, oldest first: 0 = a position of another key of the bucket (it agrees
    with p on fewer than 3 bytes), L >= 3 = a position that agrees with p on exactly L bytes (on max_len and more where L is max_len).
    Between the candidates and p's window a 24-byte block repeats, so that the chunk is not stored raw; p's window holds filler in front of p.
    cut: the chunk ends cut bytes behind p, and the candidates' bytes from `cut` on are zeros (what a compare past the end would look at)."""
    n = p + 64
    nc = len(spec)
    ks = M.keys_of_bucket(M.BUCKET, NKEYS)                                       # ks[j]: the colliding key of candidate j, ks[-1]: the position's own
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
        if p not in M.greedy_token_starts(c):
            continue
        return c, f
    raise AssertionError("no unit for position %d, candidates %s" % (p, spec))


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


def _chunk_is_compressed(stream, k):
    """whether chunk k of an LZNT1 stream is a compressed chunk (header bit 15), not a raw copy"""
    return not list(M.walk_stream(stream))[k][2]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
def test_lznt1_finishing_steps_best(oracle, gpu_ctx, mode):
    built = _built()
    for name, u, k, _ in built:
        assert _chunk_is_compressed(R.expected(oracle, u), k), "%s: the target's chunk is stored raw and tests nothing" % name
    R.check_batch(oracle, gpu_ctx, [u for _, u, _, _ in built], mode, 0, "finishing steps", names=[name for name, _, _, _ in built])
