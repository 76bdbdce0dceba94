"""The finishing event of LZNT1's window parse (csrc/lznt1.hip lz_window): the greedy walk stops on a position whose best match is not settled,
the whole wave settles it (the finishing steps, 64 candidates each), and the event's epilogue clears the position's bit, writes its key back
into its lane, takes the match or steps over the position as a literal and finds the next stop. The event's scalar code is hand-shaped: the
walk leaves without a flag, the step loop keeps its threshold across steps and ends on one compare, the epilogue is one block that relies on
shift counts wrapping. The units here put one event (or two, or three) on every edge of that code: where in the window it happens, where its
match ends, what follows it, how the bucket's entries fall into steps, how the threshold moves, and the long-pending stops.
Every unit is one chunk. Each builder places its positions on the CPU model of the bucket array that tests/lznt1_model.py keeps, proves
there that the unit is what it claims (a unit that is not fails the CPU test), and the GPU tests compare all units with the oracle byte for byte
in both chunk-kernel modes, through a plan with host tables, a plan with device tables and the serial-atomics instance."""
import functools

import numpy as np
import pytest

import lznt1_model as M
import lznt1_run as R
from lznt1_model import BUCKET, NKEYS, P18, P34, SELF, parse as _parse

LAST = (1 << M.BITS) - 1                             # the last bucket: its youngest entry is the last slot of the bucket array
SEAM = 64 * M.SEG_FIRST_WINDOW[1]                    # first position of segment 1


def _copies(b, after, k=6):
    """a `pre` step of _unit: k copies of the bytes b behind the candidates, each followed by a byte that differs from `after`"""
    def put(c, at):
        for _ in range(k):
            M.place(c, at, b)
            c[at + len(b)] = after ^ 0x55
            at += len(b) + 4
        return at
    return put


def _unit(p, spec, seed, cut=None, fill_to=None, bucket=BUCKET, xpatch=None, pre=None, check=None):
    """_build of tests/test_gpu_lznt1_best.py with three more handles. A chunk of p + 64 bytes whose position p has len(spec) older entries in its bucket, oldest first: 0 = a
    position of another key of the bucket, L >= 3 = a position that agrees with p on exactly L bytes; a 24-byte block repeats between the
    candidates and fill_to (default: the start of p's window, which then holds filler in front of p).
    xpatch(x, c): changes the bytes x that will stand at p, before the candidates copy them; pre(x) -> put(c, at): places more bytes behind
    the candidates; check(f, c, parse): what the unit claims, on the model -- a filler that misses it is replaced by the next."""
    n = p + 64
    nc = len(spec)
    ks = M.keys_of_bucket(bucket, NKEYS)
    assert nc < NKEYS
    for s in range(80):
        sd = seed + 7919 * s
        c = M.filler(n, sd).copy()
        x = np.concatenate([np.frombuffer(ks[-1], dtype=np.uint8), M.filler(60, sd + 13)]).copy()
        if xpatch is not None:
            xpatch(x, c)
        at, where = 8, []
        for j, L in enumerate(spec):
            where.append(at)
            if L == 0:
                M.place(c, at, ks[j])
                at += 6
            else:
                M.place(c, at, x[:L])
                c[at + L] = x[L] ^ 0x55
                if cut is not None:
                    c[at + cut:at + L + 1] = 0
                at += L + 4
        if pre is not None:
            at = pre(x)(c, at)
        hi = p & ~63 if fill_to is None else fill_to
        assert hi - (at + 8) >= 48, "no room for the repeats in front of position %d" % p
        c[at + 8:hi] = np.resize(M.filler(24, sd + 5), hi - (at + 8))
        M.place(c, p, x[:min(len(x), n - p)])
        if cut is not None:
            c = c[:p + cut].copy()
        f = M.finish(c, p)
        want = [min(L, cut) if cut is not None and L else L for L in spec]
        if f["rank"] != nc or f["cands"] != where:
            continue
        if not all(l == w if w else l < 3 for l, w in zip(f["lens"], want)):
            continue
        parse = _parse(c)
        if p not in parse or parse[p] != ((f["best"] >> 12) if (f["best"] >> 12) >= 3 else 0):
            continue
        if check is not None and not check(f, c, parse):
            continue
        return c
    raise AssertionError("no unit for position %d, candidates %s" % (p, spec))


def _event(f):
    """the walk stops on the position and the wave runs finishing steps for it"""
    return bool(f["finish"]) and len(f["steps"]) >= 1


def _cases():
    Z = [0]
    ONE = Z * 4 + [0, 6, 0]                          # an event whose one step has one winner: a match of 6 bytes
    cs = []

    def add(name, p, spec, check, **kw):
        cs.append((name, p, spec, check, kw))

    def lens(f):
        return (f["best"] >> 12)

    # -- position of the event in the window
    add("event at lane 0 of a window", 1536, ONE, lambda f, c, t: _event(f) and lens(f) == 6)
    add("event at lane 63 of a window", 1535, ONE, lambda f, c, t: _event(f) and lens(f) == 6)
    add("event at the last active lane of a short last window (max_len 3)", 1497, Z * 4 + [0, 30, 0],
        lambda f, c, t: _event(f) and len(c) == 1500 and len(c) % 64 and f["maxl"] == 3 and lens(f) == 3, cut=3)
    add("event at the entry lane of a repaired seam window", SEAM + 7, ONE,
        lambda f, c, t: _event(f) and SEAM not in t and (SEAM + 6) not in t and lens(f) == 6, fill_to=SEAM + 7)
    # -- where the event's match ends
    add("match ends inside the window on a further stop", P34, ONE,
        lambda f, c, t: _event(f) and t.get(P34 + 6, 0) >= 3 and (P34 + 6) % 64 > 6, xpatch=lambda x, c: x.__setitem__(slice(6, 11), c[2:7]))
    add("match ends inside the window with no stop left", P34, ONE,
        lambda f, c, t: _event(f) and all(t.get(q) == 0 for q in range(P34 + 6, (P34 | 63) + 1)))
    add("match ends exactly at the window's end", 1530, ONE, lambda f, c, t: _event(f) and (1530 + lens(f)) % 64 == 0)
    add("match ends beyond the window", 1532, ONE, lambda f, c, t: _event(f) and 1532 % 64 + lens(f) > 64)
    add("a long match ends far beyond the window", 1530, Z * 4 + [0, 34, 0],
        lambda f, c, t: _event(f) and lens(f) == 34 and f["steps"][0]["tail"])
    # -- what follows the event
    add("the event leaves a literal, the next stop is the next position", P34, Z * 7,
        lambda f, c, t: _event(f) and lens(f) < 3 and t[P34] == 0 and t.get(P34 + 1, 0) >= 3, pre=lambda x: _copies(x[1:5], int(x[5]), k=1))
    add("two events at adjacent positions", P34, Z * 7,
        lambda f, c, t: _event(f) and t[P34] == 0 and _event(M.finish(c, P34 + 1)) and t.get(P34 + 1, 0) == 3,
        pre=lambda x: _copies(x[1:4], int(x[4])))
    add("three events in one window with taken matches between them", P34, ONE,
        lambda f, c, t: _event(f) and _event(M.finish(c, P34 + 6)) and _event(M.finish(c, P34 + 11))
        and (t.get(P34), t.get(P34 + 6), t.get(P34 + 11)) == (6, 5, 4) and (P34 + 15) // 64 == P34 // 64,
        pre=lambda x: (lambda c, at: _copies(x[11:15], int(x[15]))(c, _copies(x[6:11], int(x[11]))(c, at))))
    # -- bucket geometry of the step loop
    add("exactly 5 older entries: one candidate in the one step", P34, Z * 4 + [6],
        lambda f, c, t: _event(f) and [s["valid"] for s in f["steps"]] == [1] and f["steps"][0]["winners"] == [0])
    add("4 + 63 older entries", P34, Z * 4 + Z * 62 + [6],
        lambda f, c, t: _event(f) and [s["valid"] for s in f["steps"]] == [63] and f["steps"][0]["winners"] == [62])
    add("4 + 64 older entries: the own entry is lane 0 of a second step", P34, Z * 4 + Z * 63 + [6],
        lambda f, c, t: _event(f) and [s["valid"] for s in f["steps"]] == [64, 0] and f["steps"][0]["winners"] == [63])
    add("4 + 65 older entries", P34, Z * 4 + Z * 64 + [6],
        lambda f, c, t: _event(f) and [s["valid"] for s in f["steps"]] == [64, 1] and f["steps"][1]["winners"] == [0])
    add("the own entry is the last slot of the bucket array", P34, ONE,
        lambda f, c, t: _event(f) and M.bucket_model(c)[1][P34] == len(c) - 3 and lens(f) == 6, bucket=LAST)
    # -- the threshold and the early exit
    add("a winner in step 1 that step 2 beats by one byte", P34, [3, 0, 0, 0, 5] + Z * 63 + [6],
        lambda f, c, t: _event(f) and [s["need"] for s in f["steps"]] == [4, 6] and [len(s["winners"]) for s in f["steps"]] == [1, 1] and lens(f) == 6)
    add("a winner in step 1 that step 2 only ties", P34, [3, 0, 0, 0, 5] + Z * 63 + [5],
        lambda f, c, t: _event(f) and [s["need"] for s in f["steps"]] == [4, 6] and [len(s["winners"]) for s in f["steps"]] == [1, 0]
        and f["best"] == M.best_key(5, f["cands"][4]))
    add("a winner reaches max_len with candidates left behind", P18, Z * 4 + [0, 18, 0] + Z * 70,
        lambda f, c, t: _event(f) and lens(f) == f["maxl"] == 18 and f["left"] > 0 and len(f["steps"]) == 1)
    for m in (3, 8, 9, 16, 17):
        add("max_len %d at the event" % m, 1500 - m, Z * 4 + [0, 30, 0], lambda f, c, t, m=m: _event(f) and lens(f) == f["maxl"] == m, cut=m)
    add("max_len 8 with a candidate that stops inside the first stage", 1492, Z * 4 + [0, 5, 0],
        lambda f, c, t: _event(f) and f["maxl"] == 8 and lens(f) == 5, cut=8)
    # -- long-pending stops
    add("long-pending and unresolved: the steps run behind the extension", P34, [20, 0, 0, 0, 18, 25, 0],
        lambda f, c, t: f["pending"] and _event(f) and f["steps"][0]["need"] == 21 and lens(f) == 25)
    add("long-pending with a fifth candidate, resolved by the extension", P34, [34, 0, 0, 0, 0, 20, 0],
        lambda f, c, t: f["pending"] and f["rank"] > SELF and (f["provisional"] >> 12) == 16 and not f["finish"] and lens(f) == f["maxl"] == 34)
    add("long-pending alone: no fifth candidate", P34, [20, 0],
        lambda f, c, t: f["pending"] and f["rank"] <= SELF and not f["finish"] and lens(f) == 20)
    return cs


@functools.lru_cache(maxsize=None)
def _built():
    """[(name, unit)]"""
    return [(name, _unit(p, spec, 500 + 10 * i, check=check, **kw).tobytes()) for i, (name, p, spec, check, kw) in enumerate(_cases())]


def test_units_are_what_they_claim():
    built = _built()                                 # (every builder checks its unit on the model and raises if no filler makes it)
    assert len(built) == len(_cases()) and all(0 < len(u) <= 8192 for _, u in built)
    assert len({u for _, u in built}) == len(built)


def _expected(oracle):
    """{name: the oracle's bytes of the unit}"""
    out = {name: R.expected(oracle, u) for name, u in _built()}
    for name, exp in out.items():
        assert exp[1] & 0x80, "%s: the chunk is stored raw and tests nothing" % name
    return out


def test_the_oracle_parses_the_units_as_the_model_does(oracle):
    """what the builders proved on the model holds for the oracle's stream: the same token starts and match lengths"""
    expected = _expected(oracle)
    for name, u in _built():
        assert M.token_lengths(expected[name]) == _parse(np.frombuffer(u, np.uint8)), name


@pytest.mark.gpu
@pytest.mark.parametrize("path", R.PATHS)
@pytest.mark.parametrize("mode", [1, 2])
def test_lznt1_finishing_event(oracle, gpu_ctx, mode, path):
    built = _built()
    _expected(oracle)
    R.check_plan(oracle, gpu_ctx, [u for _, u in built], mode, path, "finishing event", names=[name for name, _ in built])
