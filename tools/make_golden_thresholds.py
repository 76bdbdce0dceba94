"""tests/golden/thresholds.json: inputs that land on the encoders' raw / fallback decisions (tests/thresholds.py), found here by a
seeded search against the oracle's decision probes and checked one by one against the compiled reference (oracle/_ref).
Dev container only (needs oracle/_ref).        python tools/make_golden_thresholds.py

Per case: the recipe (codec, seed, length, boundary chunk, plants, labels, wanted delta), the probe's record of the boundary chunk, the
reference's output length and SHA-256, and the reference's status at cap = size and cap = size - 1. Plus digests of the reference's
CreateCodesSlow for the seeded histograms of tests/thresholds.py (the package-merge stage test).

Short chunks of independent random bytes never come up to the Xpress+Huffman limit (300 B: at most -2 over 2000 seeds, and plants only copy, so the
number of distinct byte values cannot grow; 4096 B with the 18-byte match an odd delta needs: at most -3), and a match with three raw length bytes costs a
64 KiB chunk of random bytes about 267 B where about 150 are on offer. These cases start from the recipe base "shuffle" (seeded permutations of the 256
byte values, the flattest histogram): a 300-byte chunk then starts at +6, a 64 KiB chunk at about +266.

What the search could NOT reach is written to the "unreachable" list of the fixture with the closest delta found, and stated here:

* Xpress+Huffman, odd deltas on chunks of 300 bytes (one chunk of 300 B; a last chunk of 300 B after a full one). comp - extra is a whole number of
  16-bit words and the limit n + 36 is even, so an odd delta needs an odd number of raw length bytes, i.e. a match of at least 18 bytes; in 300 bytes
  such a match takes comp far below the limit (closest odd delta found: -8 in both geometries). The boundary cases of these two geometries are therefore
  the even neighbours of the switch: delta 0 (kept) and +2 (falls back), three seeds each, and -2, -4 below.
* Xpress+Huffman, an odd `extra` at delta 0: not searched for, it cannot exist (the same parity: every limit of the 64 KiB geometries is even). The
  odd-extra cases are at delta -1 and +1; the cases at delta 0 with a 1-byte raw length carry two such matches.
Everything else the coverage list asks for was found, the match with three raw length bytes at +1..+3 included.
"""
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import loader as L
import thresholds as T

C = 65536
CROSS_MID = [[C + 100, 300, 5], [C + 5000, 40000, 4], [C + 30000, 65535, 6]]      # sources in the previous chunk
CROSS_LAST = [[C + 20, 1000, 4], [C + 150, 50000, 5]]
XH_GEOMS = [  # name, length, boundary chunk, pinned plants, even deltas only, base (short chunks of independent random bytes stay below the limit)
    ("one300", 300, 0, [], True, "shuffle"), ("one4096", 4096, 0, [], False, "shuffle"), ("one40000", 40000, 0, [], False, "random"),
    ("one65536", C, 0, [], False, "random"), ("tail1", C + 1, 0, [], False, "random"), ("tail100", C + 100, 0, [], False, "random"),
    ("tail65536", 2 * C, 0, [], False, "random"), ("mid3", 2 * C + 5000, 1, CROSS_MID, False, "random"), ("last300", C + 300, 1, CROSS_LAST, True, "shuffle"),
]
XH_WANTS = [0, 0, 0, 1, 1, 1, -2, -1, 2, 3]
XH_WANTS_EVEN = [0, 0, 0, 2, 2, 2, -2, -4]
LZ_LENGTHS = [71, 100, 257, 1000, 4095, 4096]
LZ_WANTS = [-1, 0, -1, 0, -1, 0, -2, 1]          # placements alternate along this list

t_start = time.time()


def best_seeds(base, want, first_seed, scan):
    """seeds of the scan ordered by how little is left to do: a base delta at or above `want` first (going down is what a plant does)"""
    ds = []
    for s in range(first_seed, first_seed + scan):
        d = T.probe(L, dict(base, seed=s))[0]
        ds.append(((0, d - want) if d >= want else (1, want - d), s))
    return [s for _, s in sorted(ds)]


def find(base, want, first_seed, pinned, taken, evals=4000, scan=40, tries=6, want_ok=None):
    closest = None
    for s in best_seeds(base, want, first_seed, scan):
        if s in taken:
            continue
        if tries == 0:
            break
        tries -= 1
        res = T.search(L, dict(base, seed=s), want, evals, pinned, want_ok)
        if res:
            taken.add(s)
            return res[0], res[1]
    return None, closest


def finish(case_id, geom, recipe, delta):
    data = T.build(recipe)
    d, rec, recs = T.probe(L, recipe, data)
    assert d == delta and T.label_ok(recipe, rec)
    st, out = T.oracle_compress(L, recipe, data)
    rst, rout = T.ref_compress(L, recipe, data)
    assert (st, out) == (rst, rout) and st == 0, case_id
    caps = {}
    for name, cap in (("size", len(out)), ("size-1", len(out) - 1)):
        cs, cout = T.ref_compress(L, recipe, data, cap)
        os_, oout = T.oracle_compress(L, recipe, data, cap)
        assert cs == os_ and (cs != 0 or cout == oout == out), (case_id, name)
        caps[name] = cs
    return dict(id=case_id, geom=geom, codec=recipe["codec"], base=recipe["base"], seed=recipe["seed"], length=recipe["length"], chunk=recipe["chunk"],
                plants=recipe["plants"], labels=recipe.get("labels", []), want=delta, record=rec,
                ref_len=len(rout), ref_sha256=hashlib.sha256(rout).hexdigest(), ref_cap_status=caps)


def job_xh_geom(gi):
    geom, length, chunk, pins, even, kind = XH_GEOMS[gi]
    cases, unreachable, taken = [], [], set()
    cs = chunk * C
    for want in (XH_WANTS_EVEN if even else XH_WANTS):
        base = dict(codec="xh", base=kind, length=length, chunk=chunk, plants=[list(p) for p in pins], labels=[])
        pinned = len(pins)
        if want % 2:                                           # every limit here is even: an odd delta needs an odd number of raw length bytes
            cn = min(length - cs, C)
            base["plants"].append([cs + cn // 2, cn // 4, 18]); base["labels"] = ["len1_odd"]; pinned += 1
        r, d = find(base, want, 1000 * gi, pinned, taken, scan=100 if length - cs <= 4096 else 40, tries=12)
        if r is None:
            unreachable.append(dict(geom=geom, want=want, note="not found"))
            continue
        cases.append(finish("xh-%s-d%+d-s%d" % (geom, d, r["seed"]), geom, r, d))
    if even:                                                   # odd deltas of the 300-byte geometries: how close an 18-byte match gets
        base = dict(codec="xh", base=kind, length=length, chunk=chunk, plants=[list(p) for p in pins] + [[cs + 150, 75, 18]], labels=["len1_odd"])
        hit = []
        for s in best_seeds(base, 1, 0, 100)[:3]:
            T.search(L, dict(base, seed=s), 1, 3000, len(pins) + 1, lambda d, hit=hit: hit.append(d) and False)
        unreachable.append(dict(geom=geom, want="any odd delta", closest=max(hit), note="an odd delta needs a match of >= 18 bytes"))
    return cases, unreachable


LEN_CASES = [  # raw length bytes on the 64 KiB geometries: geom, length, chunk, base, wanted delta (or range), pinned plants, labels
    ("tail100", C + 100, 0, "random", 0, [[20000, 5000, 40], [40000, 9, 19]], ["len1"]),
    ("one65536", C, 0, "random", 0, [[30000, 7, 100], [50000, 20000, 18]], ["len1"]),
    ("mid3", 2 * C + 5000, 1, "random", 0, CROSS_MID + [[C + 9000, 20000, 30], [C + 50000, 3, 269]], ["len1"]),
    ("tail100", C + 100, 0, "random", 1, [[20000, 5000, 40]], ["len1_odd"]),
    ("one65536", C, 0, "random", 1, [[30000, 7, 100]], ["len1_odd"]),
    ("mid3", 2 * C + 5000, 1, "random", 1, CROSS_MID + [[C + 9000, 20000, 30], [C + 50000, 3, 269], [C + 60000, 100, 18]], ["len1_odd"]),
    ("tail65536", 2 * C, 0, "random", -1, [[1000, 500, 272]], ["len1_odd"]),
    ("tail100", C + 100, 0, "shuffle", (-2, 0), [[20000, 5000, 300]], ["len3"]),
    ("tail1", C + 1, 0, "shuffle", (1, 3), [[20000, 5000, 273]], ["len3"]),
]


def job_len(k):
    geom, length, chunk, kind, want, plants, labels = LEN_CASES[k]
    base = dict(codec="xh", base=kind, length=length, chunk=chunk, plants=[list(p) for p in plants], labels=labels)
    seen = []
    if isinstance(want, tuple):
        lo, hi = want
        r, d = find(base, (lo + hi) // 2, 20000 + 100 * k, len(plants), set(), evals=6000, tries=4,
                    want_ok=lambda d: seen.append(d) or lo <= d <= hi)
    else:
        r, d = find(base, want, 20000 + 100 * k, len(plants), set())
    if r is None:
        closest = min(seen, key=lambda d: abs(d - (want[0] + want[1]) // 2)) if seen else None
        return [], [dict(geom=geom, want=list(want) if isinstance(want, tuple) else want, labels=labels, closest=closest, note="not found")]
    return [finish("xh-%s-%s-d%+d-s%d" % (geom, labels[0], d, r["seed"]), geom, r, d)], []


LZ_JOBS = [("lznt1", n) for n in LZ_LENGTHS] + [("lznt1_sa", n) for n in (1000, 4096)]


def job_lz(j):
    codec, n = LZ_JOBS[j]
    cases, unreachable, taken = [], [], set()
    for k, want in enumerate(LZ_WANTS):
        place = ("only", "first3" if n == 4096 else "last3")[(k // 2 + k) % 2]
        length, chunk = {"only": (n, 0), "first3": (2 * 4096 + 1500, 0), "last3": (2 * 4096 + n, 2)}[place]
        base = dict(codec=codec, base="random", length=length, chunk=chunk, plants=[], labels=[])
        r, d = find(base, want, 40000 + 1000 * j, 0, taken, scan=8)
        if r is None:
            unreachable.append(dict(geom="%s-%d-%s" % (codec, n, place), want=want, note="not found"))
            continue
        cases.append(finish("%s-%d-%s-d%+d-s%d" % (codec, n, place, d, r["seed"]), "%d-%s" % (n, place), r, d))
    return cases, unreachable


def job_early(_):
    # a group well before the end already reaches n (the reference leaves the parse there; the kernels compare the total)
    cases = []
    for length, chunk, plants, seed in ((4096, 0, [[1000, 500, 40], [3000, 1, 200]], 50001), (8192 + 4095, 2, [[8192 + 300, 100, 30], [8192 + 700, 2, 60]], 50002)):
        r = dict(codec="lznt1", base="random", seed=seed, length=length, chunk=chunk, plants=plants, labels=["cross_early"])
        d, rec, _ = T.probe(L, r)
        assert d >= 8 and T.label_ok(r, rec), (d, rec)
        cases.append(finish("lznt1-%d-early-d%+d-s%d" % (rec["n"], d, seed), "early", r, d))
    return cases, []


def run(job):
    fn, arg = job
    t = time.time()
    out = globals()[fn](arg)
    print("%s(%s): %d cases, %d unreached, %.0f s" % (fn, arg, len(out[0]), len(out[1]), time.time() - t), flush=True)
    return out


import multiprocessing
jobs = [("job_xh_geom", i) for i in range(len(XH_GEOMS))] + [("job_len", k) for k in range(len(LEN_CASES))] \
    + [("job_lz", j) for j in range(len(LZ_JOBS))] + [("job_early", 0)]
with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
    results = pool.map(run, jobs, chunksize=1)
cases = [c for r in results for c in r[0]]
unreachable = [u for r in results for u in r[1]]

# ---- the package-merge builder: the reference's CreateCodesSlow on the seeded histograms
HUFF = os.path.join(ROOT, "oracle", "_ref", "huff_ref")
per = []
for c in T.seeded_histograms():
    out = subprocess.run([HUFF, "slow"], input=" ".join(map(str, c)), capture_output=True, text=True, check=True).stdout.split()
    lens = bytes(int(x) for x in out)
    assert len(lens) == 512
    per.append(hashlib.sha256(lens).hexdigest()[:16])

with open(T.PATH, "w") as f:
    f.write('{"about": "inputs on the raw / fallback decisions of the encoders, as recipes (tests/thresholds.py; tools/make_golden_thresholds.py)",\n')
    f.write('"unreachable": %s,\n' % json.dumps(unreachable))
    f.write('"huff_slow_sha256_16": %s,\n' % json.dumps(per))
    f.write('"cases": [\n' + ",\n".join(json.dumps(c, separators=(",", ":")) for c in cases) + "\n]}\n")
print(len(cases), "cases,", len(unreachable), "unreachable, %d bytes, %.0f s" % (os.path.getsize(T.PATH), time.time() - t_start))
