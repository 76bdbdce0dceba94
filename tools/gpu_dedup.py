"""The block deduper (mscomp_amd_deduper_dedup) on the bench corpus as block containers: one resource per file (12 files), B = 65536, with
checksums. Reported per format, HIP events after two warm-ups, mean of `reps` executions, the call's own graph:
  a_ms               two containers that hold the same 12 files in two orders: everything in the second is a duplicate
  b_ms               the same with no duplicates (the second container holds the files with their first byte changed): the floor, tables
                     and 32 bytes per row only
  c_ms / c_host_ms   (a) followed by the splice of its picks (a splicer made for 24 picks takes d_pick as it is), against what a caller
                     does today: BlockContainer.decompress of both containers, then torch.equal per pair of resources of equal length
                     (a host clock around it: every torch.equal answers on the host)
and from `reps` profiled executions of (a) (plain launches, an event pair around each stage) the mean time per stage -- judge, keys,
confirm, settle -- and the confirm pass beside a plain device copy of the bytes of the duplicates (copy_ms, a mean of `reps` too): the
confirm pass reads that many bytes twice and writes none. Both run largely out of the Infinity Cache at these sizes: not HBM rates. The results
are checked: the representatives, the counts, and the spliced container against the first one.
Prints one line per format and writes the list to profiles/dedup_blocks.json (or to `out`).
Usage: python tools/gpu_dedup.py [reps] [out]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ms_compress_amd as m  # noqa: E402
from ms_compress_amd import corpus  # noqa: E402
from gpu_read import event_ms  # noqa: E402
from gpu_splice import Container, z32, z64  # noqa: E402

ORDER2 = [7, 0, 9, 3, 5, 11, 1, 6, 10, 2, 8, 4]                  # the second container holds the files in this order


def run(ctx, fmt, B, files, reps):
    n = len(files)
    one, two = Container(ctx, fmt, B, files), Container(ctx, fmt, B, [files[k] for k in ORDER2])
    changed = []
    for k in ORDER2:
        f = files[k].copy()
        f[0] ^= 0x55
        changed.append(f)
    other = Container(ctx, fmt, B, changed)
    N, rows = 2 * n, one.nbt + two.nbt
    dd = m.BlockDeduper(ctx, B, 2, N, rows)
    d_rep, d_idx, d_pick, d_cnt, d_st = z64(N), z64(N), z64(2 * N), z64(4), z32(N)
    # (a) everything in the second container is a duplicate
    dedup = lambda second: dd.dedup([one.view, second.view], d_rep, d_idx, d_pick, d_cnt, d_st)
    a_ms = event_ms(lambda: dedup(two), reps)
    torch.cuda.synchronize()
    want = list(range(n)) + ORDER2
    assert d_rep.cpu().tolist() == want and d_cnt.cpu().tolist() == [n, N, two.packed_bytes, 0] and not bool(d_st.any())
    dedup(two)                                                     # (a plain execution first: the profiled ones start warm)
    ctx.profile_enable(True)
    for _ in range(reps):
        dedup(two)
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    assert all(prof[k][1] == reps for k in ("dd_judge", "dd_keys", "dd_confirm_kernel", "dd_settle_kernel"))
    stage = {k: prof[k][0] / reps for k in ("dd_judge", "dd_keys", "dd_confirm_kernel", "dd_settle_kernel")}
    d_copy = torch.zeros_like(two.d_packed)
    copy_ms = event_ms(lambda: d_copy[: two.packed_bytes].copy_(two.d_packed[: two.packed_bytes]), reps)
    # (c) dedup, then the splice of the picks: the merged container is the first one
    sp = m.BlockSplicer(ctx, B, 2, N, one.nbt + n)
    d_new, d_nfirst, d_noff, d_ncrc, d_nlen, d_sst = torch.zeros_like(one.d_packed), z64(N + 1), z64(one.nbt + n + 1), z32(one.nbt + n), z64(N), z32(N)

    def both():
        dedup(two)
        sp.splice([one.view, two.view], d_pick, d_new, d_nfirst, d_noff, d_nlen, d_sst, d_new_block_crc=d_ncrc, new_cap=one.total)
    c_ms = event_ms(both, reps)
    torch.cuda.synchronize()
    assert d_sst.cpu().tolist() == [0] * n + [m.MSCOMP_ARG_ERROR] * n and bool((d_nfirst[: n + 1] == one.d_first).all())
    assert bool((d_noff[: one.nb + 1] == one.d_boff[: one.nb + 1]).all()) and bool((d_ncrc[: one.nb] == one.d_crc[: one.nb]).all())
    assert bool((d_new[: one.packed_bytes] == one.d_packed[: one.packed_bytes]).all())
    # what a caller does today: decode both containers, compare every pair of equal length
    outs = [(torch.zeros_like(c.d_in), z64(n), z32(n)) for c in (one, two)]

    def host_side():
        for c, (d_out, d_olen, d_dst) in zip((one, two), outs):
            c.bk.decompress(c.d_packed, c.d_first, c.d_boff, c.t_len, d_out, c.t_off, c.t_len, d_olen, d_dst, packed_len=c.packed_bytes)
        rep = list(range(N))
        data = [(outs[s][0], int(c.off[r]), c.lens[r]) for s, c in enumerate((one, two)) for r in range(n)]
        for g, (t, o, ln) in enumerate(data):
            for h, (t2, o2, ln2) in enumerate(data[:g]):
                if ln2 == ln and rep[h] == h and torch.equal(t[o: o + ln], t2[o2: o2 + ln2]):
                    rep[g] = h
                    break
        return rep
    for _ in range(2):
        assert host_side() == want
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        host_side()
    torch.cuda.synchronize()
    c_host_ms = (time.perf_counter() - t0) * 1e3 / reps
    # (b) no duplicates: the floor
    b_ms = event_ms(lambda: dedup(other), reps)
    torch.cuda.synchronize()
    assert d_rep.cpu().tolist() == list(range(N)) and d_cnt.cpu().tolist() == [N, N, 0, 0]
    sp.close(); dd.close()
    res = dict(format=fmt, block=B, resources=N, rows=one.nb + two.nb, mb=round(2 * one.total / 1e6, 1), packed_mb=round((one.packed_bytes + two.packed_bytes) / 1e6, 1),
               dup_packed_mb=round(two.packed_bytes / 1e6, 1), a_ms=round(a_ms, 4), b_ms=round(b_ms, 4), c_ms=round(c_ms, 4), c_host_ms=round(c_host_ms, 3),
               c_ratio=round(c_ms / c_host_ms, 4), judge_ms=round(stage["dd_judge"], 4), keys_ms=round(stage["dd_keys"], 4),
               confirm_ms=round(stage["dd_confirm_kernel"], 4), settle_ms=round(stage["dd_settle_kernel"], 4),
               confirm_read_gbs=round(2 * two.packed_bytes / stage["dd_confirm_kernel"] / 1e6, 1), copy_ms=round(copy_ms, 4),
               copy_gbs=round(two.packed_bytes / copy_ms / 1e6, 1), confirm_over_copy=round(stage["dd_confirm_kernel"] / copy_ms, 3))
    for c in (one, two, other):
        c.bk.close()
    return res


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "dedup_blocks.json")
    torch.cuda.set_device(0)
    ctx = m.Context()
    files = [corpus.file_bytes(i) for i in range(12)]
    out = []
    for name, fmt in m.FORMATS.items():
        r = run(ctx, fmt, 65536, files, reps)
        r["name"] = name
        print(json.dumps(r), flush=True)
        out.append(r)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
