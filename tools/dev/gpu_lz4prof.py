"""dev (GPU box): phase cycles of lznt1_chunk4_kernel per WAVE from a -DLZ4_PROFILE build (lane 0 of every wave, summed over blocks), each corpus
member as one unit; with --json PATH the figures go to a file as well.
    hipcc ... -DLZ4_PROFILE -c csrc/lznt1.hip, linked like the Makefile does;  MSCOMP_AMD_LIB=<that library> python tools/dev/gpu_lz4prof.py [--json PATH] [member ...]"""
import ctypes, hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import ms_compress_amd as m
from ms_compress_amd import corpus
NSLOT, NEV = 20, 4                              # (lznt1.hip LZ4_NSLOT; the event counters behind the slots)
PHASES = ["load", "B1 rank", "B2 re-read + sums", "B3 pack", "B4 scatter", "parse + seam", "cascade", "clear + scans", "stage + emit", "flags + header"]
argv = sys.argv[1:]
jpath = None
if argv[:1] == ["--json"]:
    jpath, argv = argv[1], argv[2:]
names = argv or list(corpus.NAMES)
ctx = m.Context()
z = (ctypes.c_ulonglong * (4 * NSLOT + NEV))()
res, tot, nch_all, sha = {}, [0] * (4 * NSLOT), 0, hashlib.sha256()


def table(v, nch):
    """per phase: work cycles per chunk of the four waves, the longest of them, and the mean idle time in front of the barrier that ends it"""
    out = {}
    for i, ph in enumerate(PHASES):
        work = [v[NSLOT * w + 2 * i] / nch for w in range(4)]
        idle = [v[NSLOT * w + 2 * i + 1] / nch for w in range(4)]
        out[ph] = {"work": [round(x, 1) for x in work], "longest": round(max(work), 1), "idle_mean": round(sum(idle) / 4, 1)}
    out["sum_wave0"] = round(sum(v[:NSLOT]) / nch, 1)
    return out


for name in names:
    buf = corpus.by_name(name).tobytes()
    out, st = m.compress_units(2, [buf], ctx=ctx)          # warm-up (tables, first-touch)
    ctx.lib.mscomp_amd_debug_lz4_prof(z)
    out, st = m.compress_units(2, [buf], ctx=ctx)
    ctx.lib.mscomp_amd_debug_lz4_prof(z)
    sha.update(out[0])
    v = list(z)[:4 * NSLOT]; nch = (len(buf) + 4095) // 4096
    tot = [a + b for a, b in zip(tot, v)]; nch_all += nch
    res[name] = {"chunks": nch, **table(v, nch)}
    print(name, json.dumps(res[name]))
if len(names) > 1:
    res["all"] = {"chunks": nch_all, **table(tot, nch_all), "sha": sha.hexdigest()[:16]}
    print("all", json.dumps(res["all"]))
if jpath:
    with open(jpath, "w") as f:
        json.dump(res, f, indent=1)
