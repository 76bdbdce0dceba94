"""tests/golden/blocks.json: the recipes of the block-container tests (tests/blocks_model.py) and, per recipe, format and block size, the
SHA-256 of the expected packed bytes and tables -- computed here from the model over the oracle, every block checked against the
compiled reference where oracle/_ref is built.                    python tools/make_golden_blocks.py

The general recipes have lengths mult * B + add, so that 0, 1, B - 1, B, B + 1 and 3 B + 7 are met at every block size, and kinds that give
every format raw blocks (random bytes) and compressed ones (zeros, text). The threshold recipes are "k random bytes, then zeros" around the
k at which a block stops shrinking: a sweep of k over a window around the bisected switch point, from which the k with
delta = len(compressed) - len(block) = -1, 0, +1 are taken, or the nearest delta on a side that skips its value. Block lengths: 4096, 32768
(whole blocks at those block sizes) and 300 (a short lone block, at every block size). For Xpress+Huffman the delta moves in steps of two
and the sweep meets odd deltas only; lengths 299, 301, 1001, 4095 are swept for a delta of 0 as well, and what was not reached goes
to the fixture's "unreachable" list.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import loader as L
import blocks_model as M

L.build()
FMT = {"lznt1": 2, "xpress": 3, "xpress_huff": 4}
SEED = 7
RECIPES = [dict(id="g%02d" % i, kind=k, seed=100 + i, mult=m, add=a) for i, (k, m, a) in enumerate([
    ("zeros", 0, 0), ("random", 0, 1), ("random", 1, -1), ("text", 1, -1), ("random", 1, 0), ("text", 1, 0), ("text", 1, 1), ("random", 1, 1),
    ("mixed", 3, 7), ("random", 3, 7), ("text", 2, 100), ("text", 0, 300), ("random", 0, 2000), ("zeros", 1, 5), ("mixed", 2, 0)])]


def delta(fmt, blen, k):
    data = M.build(dict(kind="prefix", seed=SEED, blen=blen, k=k), 0)
    st, c = L.oracle_compress(fmt, data)
    assert st == 0
    return len(c) - blen


def sweep(fmt, blen):
    lo, hi = 0, blen                                            # delta(lo) < 0 <= delta(hi): all zeros shrink, all random bytes do not
    if delta(fmt, blen, lo) >= 0 or delta(fmt, blen, hi) < 0:
        return {}
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if delta(fmt, blen, mid) < 0 else (lo, mid)
    return {k: delta(fmt, blen, k) for k in range(max(0, hi - 24), min(blen, hi + 24) + 1)}


thresholds, unreachable = [], []
for name, fmt in FMT.items():
    for blen in (4096, 32768, 300):
        seen = sweep(fmt, blen)
        wants = (-1, 1) if fmt == 4 else (-1, 0, 1)
        for want in wants:
            side = [d for d in seen.values() if (d < 0) == (want < 0) and (d == 0) == (want == 0)]
            if not side:
                unreachable.append(dict(fmt=fmt, blen=blen, want=want, note="no delta on this side in the sweep"))
                continue
            d = want if want in side else min(side, key=lambda x: abs(x - want))
            k = min(k for k, v in seen.items() if v == d)
            thresholds.append(dict(id="t-%s-%d-d%+d" % (name, blen, d), kind="prefix", seed=SEED, fmt=fmt, blen=blen, k=k, delta=d, want=want))
    if fmt == 4:                                                # a delta of 0: other parities of the block length
        found = False
        reached = set()
        for blen in (299, 301, 1001, 4095):
            seen = sweep(fmt, blen)
            reached |= set(seen.values())
            ks = [k for k, v in seen.items() if v == 0]
            if ks:
                thresholds.append(dict(id="t-%s-%d-d+0" % (name, blen), kind="prefix", seed=SEED, fmt=fmt, blen=blen, k=min(ks), delta=0, want=0))
                found = True
        if not found:
            unreachable.append(dict(fmt=fmt, blen=[300, 4096, 32768, 299, 301, 1001, 4095], want=0, closest=sorted(reached, key=abs)[:4],
                                    note="the compressed length moves in steps of two and stayed odd against every length swept"))

fixture = dict(recipes=RECIPES, thresholds=thresholds)
ref = L.load_ref()
digests = {}
for name, fmt in FMT.items():
    digests[name] = {}
    for B in M.BLOCK_SIZES:
        per = {}
        for r in M.recipes_for(fixture, fmt, B):
            data = M.build(r, B)
            if ref is not None:
                for at in range(0, len(data), B):
                    assert L.ref_compress(fmt, data[at: at + B]) == L.oracle_compress(fmt, data[at: at + B]), (r["id"], B, at)
            packed, first, off, st = M.model_compress(L, fmt, [data], B, len(data), len(data))
            assert list(st) == [0] and len(packed) == int(off[-1]) <= len(data)
            if "delta" in r:
                assert (len(packed) == len(data)) == (r["delta"] >= 0), r
            per[r["id"]] = M.digest(packed, first, off)
        digests[name][str(B)] = per

with open(M.PATH, "w") as f:
    f.write('{"about": "block-container recipes and expected digests (tests/blocks_model.py; tools/make_golden_blocks.py)",\n')
    f.write('"unreachable": %s,\n' % json.dumps(unreachable))
    f.write('"recipes": [\n' + ",\n".join(json.dumps(r, separators=(",", ":")) for r in RECIPES) + "\n],\n")
    f.write('"thresholds": [\n' + ",\n".join(json.dumps(r, separators=(",", ":")) for r in thresholds) + "\n],\n")
    f.write('"digests": %s}\n' % json.dumps(digests, separators=(",", ":")))
print(len(RECIPES), "recipes,", len(thresholds), "thresholds,", len(unreachable), "unreachable,", os.path.getsize(M.PATH), "bytes; reference",
      "checked" if ref is not None else "NOT present")
for t in thresholds:
    print(t)
print(unreachable)
