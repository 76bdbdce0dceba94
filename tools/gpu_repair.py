"""Salvage and repair (mscomp_amd_blocks_salvage, mscomp_amd_deduper_repair) on the bench corpus as block containers: one resource per file
(12 files), B = 65536 and 4096, with checksums. The primary has the first stored byte of 1 % of its blocks flipped, the mirror that of
another 1 %, and two of the blocks are damaged in both. Reported per format and block size, HIP events after two warm-ups, mean of `reps`
executions, the calls' own graphs:
  base_ms / base2_ms  BlockContainer.decompress + .check of the primary -- what salvage replaces --, taken before and after salvage_ms: their
                      difference is the baseline's own spread in this run
  both_ms             decompress + check of both containers: what a caller does today before deciding anything on the host
  salvage_ms          salvage of the primary
  masked_ms           salvage of the mirror with d_only = the primary's verdicts
  repair_ms           the repair alone
  splice_ms           the splice by extents of the repair's lists alone
  graph_ms            the four calls captured once in one graph of the stream, replayed
and from `reps` profiled executions (plain launches, an event pair around each stage) the mean time per stage of each call, the time per
timed stage of salvage and per launch of repair (six), and new_ms: the four passes salvage adds behind the raw copy (units, verdicts,
zero-fill, fold). Checked before any number is
printed: the verdicts name exactly the damaged rows, the salvaged bytes are the data with zeros in those rows, and the rebuilt container is
the undamaged one byte for byte -- packed bytes, tables, checksums -- but for the two rows no copy has, which stay the primary's.
Prints one line per case and writes the list to profiles/repair_blocks.json (or to `out`).
Usage: python tools/gpu_repair.py [reps] [out]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ms_compress_amd as m  # noqa: E402
from ms_compress_amd import corpus  # noqa: E402
from gpu_read import event_ms  # noqa: E402
from gpu_splice import Container, z32, z64  # noqa: E402

NEW_PASSES = ("bk_sunits_kernel", "bk_sverdict_kernel", "bk_szero_kernel", "bk_sfold_kernel")


def damage(whole, B, seed):
    """(rows of the primary, rows of the mirror, the two in common): 1 % of the blocks each"""
    rs = np.random.RandomState(seed)
    k = max(3, whole.nb // 100)
    pick = rs.choice(whole.nb, 2 * k - 2, replace=False)
    common = pick[:2]
    return np.sort(pick[:k]), np.sort(np.concatenate([common, pick[k:]])), np.sort(common)


def flipped(whole, off, rows):
    """the stored bytes with the first byte of every row of ``rows`` flipped"""
    d = whole.d_packed.clone()
    idx = torch.from_numpy(off[rows].astype(np.int64)).cuda()
    d[idx] = d[idx] ^ 0xFF
    return d


def profiled(ctx, fn, reps):
    """{stage: mean ms}, timed stages per execution"""
    fn()
    ctx.profile_enable(True)
    for _ in range(reps):
        fn()
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    return {k: round(ms / reps, 4) for k, (ms, cnt) in prof.items()}, sum(cnt for _, cnt in prof.values()) // reps


def run(ctx, stream, fmt, B, files, reps):
    n = len(files)
    whole = Container(ctx, fmt, B, files)
    nb, nbt = whole.nb, whole.nbt
    off = whole.d_boff.cpu().numpy().view(np.uint64)
    first = whole.d_first.cpu().numpy().view(np.uint64)
    rows_p, rows_m, common = damage(whole, B, 11)
    d_pp, d_pm = flipped(whole, off, rows_p), flipped(whole, off, rows_m)
    view = lambda d: (d, whole.d_first, whole.d_boff, whole.t_len, whole.d_crc, whole.packed_bytes, n, nbt)
    bk2 = m.BlockContainer(ctx, fmt, B, n, whole.total)             # (the mirror's calls keep graphs of their own)
    out = [dict(d_out=torch.zeros_like(whole.d_in), olen=z64(n), bad=z32(n), ver=z32(nbt), cnt=z64(4), st=z32(n)) for _ in range(2)]

    def salvage(bk, d_packed, o, only=None):
        bk.salvage(d_packed, whole.d_first, whole.d_boff, whole.t_len, o["d_out"], whole.t_off, whole.t_len, o["olen"], o["bad"], o["ver"], o["cnt"], o["st"],
                   d_block_crc=whole.d_crc, d_only=only, packed_len=whole.packed_bytes)
    salvage_p = lambda: salvage(whole.bk, d_pp, out[0])
    salvage_m = lambda: salvage(bk2, d_pm, out[1], out[0]["ver"])
    base_out = [(torch.zeros_like(whole.d_in), z64(n), z32(n)) for _ in range(2)]

    def decode(bk, d_packed, o):
        bk.decompress(d_packed, whole.d_first, whole.d_boff, whole.t_len, o[0], whole.t_off, whole.t_len, o[1], o[2], packed_len=whole.packed_bytes)
        bk.check(o[0], whole.t_off, whole.t_len, whole.d_first, whole.d_crc, o[1], o[2])
    base = lambda: decode(whole.bk, d_pp, base_out[0])

    def both():
        base()
        decode(bk2, d_pm, base_out[1])
    base_ms = event_ms(base, reps)
    salvage_ms = event_ms(salvage_p, reps)
    base2_ms = event_ms(base, reps)
    masked_ms = event_ms(salvage_m, reps)
    both_ms = event_ms(both, reps)
    # the repair and the splice
    dd, sp = m.BlockDeduper.for_repair(ctx, B, 2, n, nb), m.BlockSplicer.for_extents(ctx, B, 2, n, nb, nbt)
    d_ef, d_ext, d_fix, d_lost, d_cnt, d_st = z64(n + 1), z64(4 * nb), z64(n), z64(n), z64(4), z32(n)
    N = (torch.zeros_like(whole.d_packed), z64(n + 1), z64(nbt + 1), z64(n), z32(nbt), z32(n))
    repair = lambda: dd.repair([view(d_pp), view(d_pm)], [out[0]["ver"], out[1]["ver"]], d_ef, d_ext, d_fix, d_lost, d_cnt, d_st)
    splice = lambda: sp.splice_extents([view(d_pp), view(d_pm)], d_ef, d_ext, N[0], N[1], N[2], N[3], N[5], d_new_block_crc=N[4], new_cap=whole.total)
    repair_ms = event_ms(repair, reps)
    splice_ms = event_ms(splice, reps)
    stream.synchronize()
    # the checks: verdicts, salvaged bytes, counts, the rebuilt container
    ver = [o["ver"].cpu().numpy().view(np.uint32) for o in out]
    assert sorted(np.nonzero((ver[0] != 0) & (ver[0] != 4))[0]) == list(rows_p) and (ver[0][:nb] != 4).all() and (ver[0][nb:] == 4).all(), "the primary's verdicts"
    assert sorted(np.nonzero(ver[1] != 4)[0]) == list(rows_p) and sorted(np.nonzero((ver[1] != 0) & (ver[1] != 4))[0]) == list(common), "the mirror's verdicts"
    row_res = np.searchsorted(first, rows_p, side="right") - 1
    want = whole.d_in.clone()
    zeroed = 0
    for j, r in zip(rows_p, row_res):
        at = int(whole.off[r]) + int(j - first[r]) * B
        e = min(B, whole.lens[r] - int(j - first[r]) * B)
        want[at: at + e] = 0
        zeroed += e
    assert torch.equal(out[0]["d_out"], want), "salvaged bytes: the data, zeros in the bad rows"
    assert [int(x) for x in out[0]["cnt"].cpu()] == [nb, len(rows_p), zeroed, len(set(row_res.tolist()))] and [int(x) for x in out[1]["cnt"].cpu()][:2] == [len(rows_p), 2]
    assert [int(x) for x in out[0]["olen"].cpu()] == whole.lens
    count = [int(x) for x in d_cnt.cpu()]
    assert count[:2] == [len(rows_p) - 2, 2] and count[3] == int((d_lost != 0).sum()) and int(d_st.ne(0).sum()) == count[3]
    expect = flipped(whole, off, common)                           # the two lost rows stay the primary's
    assert not bool(N[5].any()) and bool((N[1] == whole.d_first).all()) and bool((N[2] == whole.d_boff).all()) and bool((N[4] == whole.d_crc).all())
    assert bool((N[3] == whole.t_len).all()) and torch.equal(N[0][: whole.packed_bytes], expect[: whole.packed_bytes]), "the rebuilt container"
    # one captured graph of the four calls
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        salvage_p(); salvage_m(); repair(); splice()
    graph_ms = event_ms(g.replay, reps)
    stream.synchronize()
    assert torch.equal(N[0][: whole.packed_bytes], expect[: whole.packed_bytes]) and [int(x) for x in d_cnt.cpu()] == count
    del g
    stages = {}
    for name, fn in (("base", base), ("salvage", salvage_p), ("masked", salvage_m), ("repair", repair), ("splice", splice)):
        stages[name], stages[name + "_stages"] = profiled(ctx, fn, reps)
    new_ms = sum(stages["salvage"][k] for k in NEW_PASSES)
    for h in (dd, sp, bk2, whole.bk):
        h.close()
    return dict(format=fmt, block=B, resources=n, rows=nb, mb=round(whole.total / 1e6, 1), packed_mb=round(whole.packed_bytes / 1e6, 1), bad_rows=len(rows_p),
                count=count, base_ms=round(base_ms, 4), base2_ms=round(base2_ms, 4), base_spread_ms=round(abs(base_ms - base2_ms), 4), both_ms=round(both_ms, 4),
                salvage_ms=round(salvage_ms, 4), new_ms=round(new_ms, 4), salvage_over_base=round(salvage_ms / min(base_ms, base2_ms), 4),
                excess_ms=round(salvage_ms - max(base_ms, base2_ms), 4), masked_ms=round(masked_ms, 4), masked_over_salvage=round(masked_ms / salvage_ms, 4),
                repair_ms=round(repair_ms, 4), splice_ms=round(splice_ms, 4), graph_ms=round(graph_ms, 4), pipeline_over_both=round(graph_ms / both_ms, 4),
                salvage_ms_per_stage=round(salvage_ms / stages["salvage_stages"], 5), repair_ms_per_launch=round(repair_ms / 6, 5),
                stages=stages)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "repair_blocks.json")
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    out = []
    with torch.cuda.stream(stream):
        ctx = m.Context(stream=stream)
        files = [corpus.file_bytes(i) for i in range(12)]
        for B in (65536, 4096):
            for name, fmt in m.FORMATS.items():
                r = run(ctx, stream, fmt, B, files, reps)
                r["name"] = name
                print(json.dumps({k: v for k, v in r.items() if k != "stages"}), flush=True)
                out.append(r)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
