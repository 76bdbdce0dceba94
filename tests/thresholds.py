"""Inputs that land on the encoders' raw / fallback decisions, stored as recipes (tests/golden/thresholds.json).

Two codecs switch the whole encoding of a chunk on one size comparison:

* Xpress+Huffman: ``comp > limit`` (limit = 65538 for a chunk that is not the last, chunk length + 36 for the last one) throws the LZ parse
  away and writes the chunk as literals with the package-merge code. delta = comp - limit; the switch happens at delta >= +1.
* LZNT1: a chunk is stored compressed only if its body S is strictly shorter than the chunk (n). delta = S - n; raw at delta >= 0.

A recipe is ``random.Random(seed).randbytes(length)`` (base "shuffle": seeded permutations of the 256 byte values one after the other, the
flattest histogram there is -- short chunks of independent random bytes never come up to the Xpress+Huffman limit) with copies planted in order: a plant (pos, off, len) sets
``b[pos + i] = b[pos + i - off]`` for i in 0..len-1. ``build`` rebuilds the bytes, ``probe`` asks the oracle's decision probes
(oracle/mscomp_oracle.h) for the record of the boundary chunk, ``search`` is the seeded hill-climber that tools/make_golden_thresholds.py
runs to find the plants; the tests only rebuild and probe. Xpress (plain) has no such switch.
"""
import json
import os
import random

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "thresholds.json")
XH_CHUNK, LZ_CHUNK = 65536, 4096
CODECS = {"xh": 4, "lznt1": 2, "lznt1_sa": 2}              # recipe codec -> format number


def chunk_size(codec):
    return XH_CHUNK if codec == "xh" else LZ_CHUNK


def build(recipe):
    """the input bytes of a recipe"""
    rnd = random.Random(recipe["seed"])
    if recipe.get("base") == "shuffle":                       # seeded permutations of the 256 byte values, one after the other: a flat histogram
        b = bytearray()
        while len(b) < recipe["length"]:
            b += bytes(rnd.sample(range(256), 256))
        del b[recipe["length"]:]
    else:
        b = bytearray(rnd.randbytes(recipe["length"]))
    for pos, off, ln in recipe["plants"]:
        assert 0 < off <= pos and pos + ln <= len(b), (pos, off, ln)
        for i in range(pos, pos + ln):
            b[i] = b[i - off]
    return bytes(b)


def probe(loader, recipe, data=None):
    """(delta, record of the boundary chunk, records of every chunk) from the oracle's decision probe"""
    data = build(recipe) if data is None else data
    if recipe["codec"] == "xh":
        recs = loader.xpress_huff_decisions(data)
        r = recs[recipe["chunk"]]
        return r["comp"] - r["limit"], r, recs
    recs = loader.lznt1_decisions(data, sa=recipe["codec"] == "lznt1_sa")
    r = recs[recipe["chunk"]]
    return r["S"] - r["n"], r, recs


def switched(recipe, delta):
    """True when the boundary chunk takes the other encoding (XH fallback / LZNT1 raw)"""
    return delta >= (1 if recipe["codec"] == "xh" else 0)


def oracle_compress(loader, recipe, data, cap=None):
    fmt = CODECS[recipe["codec"]]
    if recipe["codec"] == "lznt1_sa":
        return loader.oracle_compress_sa(data, cap)
    return loader.oracle_compress(fmt, data, cap)


def ref_compress(loader, recipe, data, cap=None):
    if recipe["codec"] == "lznt1_sa":
        return loader.ref_compress_sa(data, cap)
    return loader.ref_compress(CODECS[recipe["codec"]], data, cap)


def load():
    with open(PATH) as f:
        return json.load(f)


# ---------------------------------------------------------------------------------------------------------------------
# labels: extra conditions a recipe may ask for beside its delta (all read from the probe's record)
# ---------------------------------------------------------------------------------------------------------------------
LABELS = {
    "len1": lambda r: r["len1"] >= 1,                                   # a match with one raw length byte (len-3 in 15..269)
    "len1_odd": lambda r: r["len1"] >= 1 and r["extra"] % 2 == 1,       # ... and an odd number of raw length bytes in all
    "len3": lambda r: r["len3"] >= 1,                                   # a match with three raw length bytes (len-3 >= 270)
    "cross_early": lambda r: r["raw"] == 1 and r["cross_group"] + 8 <= r["groups"],   # LZNT1: a group well before the end reaches n
}


def label_ok(recipe, rec):
    return all(LABELS[k](rec) for k in recipe.get("labels", []))


# ---------------------------------------------------------------------------------------------------------------------
# the search (tools/make_golden_thresholds.py only)
# ---------------------------------------------------------------------------------------------------------------------
def _chunk_range(recipe):
    cs = recipe["chunk"] * chunk_size(recipe["codec"])
    return cs, min(recipe["length"], cs + chunk_size(recipe["codec"]))


def search(loader, recipe, want, evals=4000, pinned=0, want_ok=None):
    """Hill-climb the plants of `recipe` (a dict with codec, seed, length, chunk, plants, labels) until the boundary chunk's delta is `want`
    (or want_ok(delta) holds) and the labels hold. The first `pinned` plants stay in place; a pinned plant may only change its length by one.
    Every plant lies inside the boundary chunk, so the other chunks keep their bytes; offsets may reach back into earlier chunks (Xpress+Huffman
    matches cross chunks; an LZNT1 chunk sees only itself, so its offsets stay inside). Returns (recipe, delta, evaluations) or None."""
    rnd = random.Random((recipe["seed"] << 8) ^ (want & 0xFF) ^ 0x5EED)
    cs, ce = _chunk_range(recipe)
    xh = recipe["codec"] == "xh"
    done = want_ok or (lambda d: d == want)

    def score(r):
        d, rec, _ = probe(loader, r)
        return (0 if done(d) else max(1, abs(d - want))) + (0 if label_ok(r, rec) else 1000), d

    def new_plant(d):
        if d is not None and d - want > 12:                   # far above: one plant takes most of the way (a match saves about its length)
            ln = rnd.randint(3, min(d - want, 250))
        elif d is None or d > want or not xh:
            ln = rnd.choice((1, 1, 2, 3, 3, 3, 4, 5, 6, 8))
        else:                                                 # below: byte copies that flatten the histogram, far 3-byte matches
            ln = rnd.choice((1, 1, 1, 2, 3, 3))
        ln = min(ln, ce - cs - 1)
        pos = rnd.randrange(cs + 1, ce - ln + 1)
        lo = 0 if xh else cs
        far = xh and rnd.random() < 0.5
        max_off = min(pos - lo, 65535 if xh else 4095)
        off = rnd.randint(max(1, max_off // 2), max_off) if far else rnd.randint(1, max_off)
        return [pos, off, ln]

    cur = dict(recipe, plants=[list(p) for p in recipe["plants"]])
    best, d = score(cur)
    n = 1
    while best and n < evals:
        cand = dict(cur, plants=[list(p) for p in cur["plants"]])
        pl = cand["plants"]
        move = rnd.random()
        free = list(range(pinned, len(pl)))
        if move < 0.5 or not pl:
            pl.append(new_plant(d))
        elif move < 0.65 and free:
            del pl[rnd.choice(free)]
        elif move < 0.9:
            p = pl[rnd.randrange(len(pl))]
            p[2] += rnd.choice((-1, 1))
            if p[2] < 1 or p[0] + p[2] > ce:
                continue
        elif free:
            pl[rnd.choice(free)] = new_plant(d)
        else:
            continue
        s, dd = score(cand)
        n += 1
        if s <= best:
            cur, best, d = cand, s, dd
    if best:
        return None
    for i in range(len(cur["plants"]) - 1, pinned - 1, -1):   # drop every plant the result does not need (plateau moves pile them up)
        cand = dict(cur, plants=cur["plants"][:i] + cur["plants"][i + 1:])
        s, dd = score(cand)
        n += 1
        if s == 0:
            cur, d = cand, dd
    return cur, d, n


# ---------------------------------------------------------------------------------------------------------------------
# histograms for the stage test of the package-merge builder (CreateCodesSlow): symbols 0..0x100 only, as the fallback has them
# ---------------------------------------------------------------------------------------------------------------------
def seeded_histograms(seed=23):
    """512-bin histograms with counts on symbols 0..0x100 only: flat with ties (255..257, with and without EOS), counts of 1..3 over 100..257
    symbols, geometric and Fibonacci-like counts whose unrestricted tree is deeper than 15, one symbol, two symbols, 257 equal counts, one
    count of 65536."""
    rnd = random.Random(seed)
    out = []

    def hist(counts, eos):
        return list(counts) + [0] * (256 - len(counts)) + [eos] + [0] * 255

    for eos in (0, 1):
        for _ in range(6):
            out.append(hist([rnd.randint(255, 257) for _ in range(256)], eos))
        out.append(hist([256] * 256, eos))
    for _ in range(12):
        k = rnd.randint(100, 257)
        c = [rnd.randint(1, 3) for _ in range(k)] + [0] * (257 - k)
        rnd.shuffle(c)
        out.append(hist(c[:256], c[256]))
    for base in (1.3, 1.5, 1.62, 2.0):
        for k in (20, 24, 40):
            c = [min(int(base ** i) + 1, 1 << 24) for i in range(k)] + [0] * (256 - k)
            rnd.shuffle(c)
            out.append(hist(c, 1))
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    out.append(hist(fib, 1))
    out.append(hist(fib[::-1] + [1] * 200, 0))
    out.append(hist([0] * 65 + [300], 0))                      # one symbol
    out.append(hist([], 1))                                    # EOS alone
    out.append(hist([0] * 7 + [5, 0, 5], 0))                   # two symbols, tied
    out.append(hist([9], 1))                                   # a literal and EOS
    out.append(hist([77] * 256, 77))                           # 257 equal counts
    out.append(hist([1] * 256, 1))
    out.append(hist([0] * 200 + [65536], 0))                   # one count of 65536
    out.append(hist([0] * 200 + [65536], 1))
    for _ in range(8):                                         # random chunk-like: literals of a skewed source
        c = [int(60000 / (1 + i) ** rnd.uniform(0.5, 1.5)) for i in range(256)]
        rnd.shuffle(c)
        out.append(hist(c, rnd.randint(0, 1)))
    return out
