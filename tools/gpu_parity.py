"""Parity rows (mscomp_amd_parity_build, mscomp_amd_parity_rebuild) on the bench corpus as block containers: one resource per file (12
files), B = 65536 and 4096, with checksums, (k, m) = (16, 2). The build reads every stored byte once and writes m / k as many, so its
yardstick is a device copy of packed_len bytes IN THE SAME RUN; the CRC pass over the same stored rows stands beside it. Reported per
format and block size, HIP events after two warm-ups, mean of `reps` executions, the calls' own graphs, in `rounds` rounds that take
build, copy and CRC by turns:
  build_ms / copy_ms / crc_ms     the median over the rounds, with build_over_copy = the median of the rounds' ratios and its lowest and
                                  highest round (the spread), and build_gbs = (stored + parity bytes) / build_ms
  rebuild_ms                      rebuild with the first stored byte flipped in 1 % of the rows (no three of a group)
  chain_ms / graph_ms             salvage -> rebuild -> salvage of the fix view (d_only) -> repair -> splice by extents, as plain calls and
                                  captured once in one graph of the stream, replayed
  base_ms                         BlockContainer.decompress + .check of the container: what finding the damage costs today
and from `reps` profiled executions the mean time per stage of build and rebuild. Checked before any number is printed: the rebuilt rows
are the healthy container's bytes, and the chain's container is the healthy one byte for byte -- packed bytes, tables, checksums.
Prints one line per case and writes the list to profiles/parity_blocks.json (or to `out`).
Usage: python tools/gpu_parity.py [reps] [out] [rounds]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ms_compress_amd as m  # noqa: E402
from ms_compress_amd import corpus  # noqa: E402
from gpu_read import event_ms, tab  # noqa: E402
from gpu_repair import profiled  # noqa: E402
from gpu_splice import Container, z32, z64  # noqa: E402

K, M = 16, 2


def run(ctx, stream, fmt, B, files, reps, rounds):
    n = len(files)
    whole = Container(ctx, fmt, B, files)
    nb, nbt, plen = whole.nb, whole.nbt, whole.packed_bytes
    off = whole.d_boff.cpu().numpy().view(np.uint64)
    G = (nb + K - 1) // K
    pr = m.BlockParity(ctx, B, nbt, K, M)
    rows, room = pr.bound()
    d_par = torch.zeros(room + 16, dtype=torch.uint8, device="cuda")
    d_poff, d_pcrc, d_rl, d_head, d_pst = z64(rows + 1), z32(rows), z32(nbt), z64(4), z32(1)
    view = lambda d: (d, whole.d_first, whole.d_boff, whole.t_len, whole.d_crc, plen, n, nbt)
    build = lambda: pr.build(view(whole.d_packed), d_par, d_poff, d_pcrc, d_rl, d_head, d_pst, par_cap=room)
    d_copy = torch.zeros_like(whole.d_packed)
    copy = lambda: d_copy[:plen].copy_(whole.d_packed[:plen])
    crcp = m.CrcDevPlan(ctx, nb, plen)
    t_roff, t_rlen, d_rcrc, d_rst = tab(off[:nb]), tab(np.diff(off[: nb + 1])), z32(nb), z32(nb)
    crc = lambda: crcp.execute(whole.d_packed, t_roff, t_rlen, d_rcrc, d_rst)
    per = {"build": [], "copy": [], "crc": []}
    for _ in range(rounds):
        for name, fn in (("build", build), ("copy", copy), ("crc", crc)):
            per[name].append(event_ms(fn, reps))
    stream.synchronize()
    assert int(d_pst.cpu()[0]) == 0 and [int(x) for x in d_head.cpu()] == [nb, G, K, M]
    par_len = int(d_poff.cpu().numpy()[rows])
    ratios = sorted(b / c for b, c in zip(per["build"], per["copy"]))
    med = lambda v: float(np.median(v))
    # damage: the first stored byte of 1 % of the rows, no three of a group
    rs = np.random.RandomState(11)
    hit, seen = [], {}
    for j in rs.permutation(nb):
        if len(hit) >= max(3, nb // 100):
            break
        if seen.get(int(j) % G, 0) < M:
            seen[int(j) % G] = seen.get(int(j) % G, 0) + 1
            hit.append(int(j))
    hit = np.sort(np.array(hit))
    d_bad = whole.d_packed.clone()
    idx = torch.from_numpy(off[hit].astype(np.int64)).cuda()
    d_bad[idx] = d_bad[idx] ^ 0xFF
    bk2 = m.BlockContainer(ctx, fmt, B, n, whole.total)             # (the fix view's salvage keeps a graph of its own)
    out = [dict(d_out=torch.zeros_like(whole.d_in), olen=z64(n), bad=z32(n), ver=z32(nbt), cnt=z64(4), st=z32(n)) for _ in range(2)]
    fix_room = plen
    d_fix, d_foff, d_fver, d_fcnt, d_fst = torch.zeros(fix_room + 16, dtype=torch.uint8, device="cuda"), z64(nbt + 1), z32(nbt), z64(6), z32(1)
    fix_view = m.BlockParity.fix_view(view(d_bad), d_fix, d_foff, fix_len=fix_room)

    def salvage(bk, v, o, only=None):
        bk.salvage(v[0], v[1], v[2], v[3], o["d_out"], whole.t_off, whole.t_len, o["olen"], o["bad"], o["ver"], o["cnt"], o["st"], d_block_crc=whole.d_crc, d_only=only,
                   packed_len=v[5])
    salvage_p = lambda: salvage(whole.bk, view(d_bad), out[0])
    rebuild = lambda: pr.rebuild(view(d_bad), out[0]["ver"], d_par, d_poff, d_pcrc, d_rl, d_head, d_fix, d_foff, d_fver, d_fcnt, d_fst, par_len=par_len, fix_cap=fix_room)
    salvage_f = lambda: salvage(bk2, fix_view, out[1], out[0]["ver"])
    dd, sp = m.BlockDeduper.for_repair(ctx, B, 2, n, nb), m.BlockSplicer.for_extents(ctx, B, 2, n, nb, nbt)
    d_ef, d_ext, d_fixed, d_lost, d_cnt, d_st = z64(n + 1), z64(4 * nb), z64(n), z64(n), z64(4), z32(n)
    N = (torch.zeros_like(whole.d_packed), z64(n + 1), z64(nbt + 1), z64(n), z32(nbt), z32(n))
    repair = lambda: dd.repair([view(d_bad), fix_view], [out[0]["ver"], out[1]["ver"]], d_ef, d_ext, d_fixed, d_lost, d_cnt, d_st)
    splice = lambda: sp.splice_extents([view(d_bad), fix_view], d_ef, d_ext, N[0], N[1], N[2], N[3], N[5], d_new_block_crc=N[4], new_cap=whole.total)

    def chain():
        salvage_p(); rebuild(); salvage_f(); repair(); splice()
    base_out = (torch.zeros_like(whole.d_in), z64(n), z32(n))

    def base():
        whole.bk.decompress(d_bad, whole.d_first, whole.d_boff, whole.t_len, base_out[0], whole.t_off, whole.t_len, base_out[1], base_out[2], packed_len=plen)
        whole.bk.check(base_out[0], whole.t_off, whole.t_len, whole.d_first, whole.d_crc, base_out[1], base_out[2])
    salvage_p()
    rebuild_ms = event_ms(rebuild, reps)
    chain_ms = event_ms(chain, reps)
    base_ms = event_ms(base, reps)
    stream.synchronize()
    counts = [int(x) for x in d_fcnt.cpu()]
    foff = d_foff.cpu().numpy().view(np.uint64)
    assert int(d_fst.cpu()[0]) == 0 and counts[:4] == [len(hit), len(hit), len(seen), 0] and counts[5] == int(foff[nbt]), "the rebuild's counts"
    ver = d_fver.cpu().numpy().view(np.uint32)
    assert sorted(np.nonzero(ver == 0)[0]) == list(hit), "the fix view's verdicts"
    for j in hit[:: max(1, len(hit) // 50)]:
        a, b = int(foff[j]), int(foff[j + 1])
        assert torch.equal(d_fix[a:b], whole.d_packed[int(off[j]): int(off[j + 1])]), "a rebuilt row"
    assert not bool(d_st.any()) and not bool(N[5].any()) and whole.same(N[0], N[1], N[2], N[4]) and bool((N[3] == whole.t_len).all()), "the chain's container"
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        chain()
    N[0].zero_()
    graph_ms = event_ms(g.replay, reps)
    stream.synchronize()
    assert whole.same(N[0], N[1], N[2], N[4])
    del g
    stages = {}
    for name, fn in (("build", build), ("rebuild", rebuild)):
        stages[name], stages[name + "_stages"] = profiled(ctx, fn, reps)
    for h in (dd, sp, bk2, crcp, pr, whole.bk):
        h.close()
    return dict(format=fmt, block=B, k=K, m=M, resources=n, rows=nb, groups=G, mb=round(whole.total / 1e6, 1), packed_mb=round(plen / 1e6, 1), parity_mb=round(par_len / 1e6, 1),
                build_ms=round(med(per["build"]), 4), copy_ms=round(med(per["copy"]), 4), crc_ms=round(med(per["crc"]), 4),
                build_over_copy=round(float(np.median(ratios)), 4), build_over_copy_low=round(ratios[0], 4), build_over_copy_high=round(ratios[-1], 4),
                build_over_crc=round(med(per["build"]) / med(per["crc"]), 4), build_gbs=round((plen + par_len) / med(per["build"]) / 1e6, 1),
                copy_gbs=round(2 * plen / med(per["copy"]) / 1e6, 1), rounds={k: [round(x, 4) for x in v] for k, v in per.items()},
                bad_rows=len(hit), rebuild_counts=counts, rebuild_ms=round(rebuild_ms, 4), chain_ms=round(chain_ms, 4), graph_ms=round(graph_ms, 4),
                base_ms=round(base_ms, 4), graph_over_base=round(graph_ms / base_ms, 4), stages=stages)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "parity_blocks.json")
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    out = []
    with torch.cuda.stream(stream):
        ctx = m.Context(stream=stream)
        files = [corpus.file_bytes(i) for i in range(12)]
        for B in (65536, 4096):
            for name, fmt in m.FORMATS.items():
                r = run(ctx, stream, fmt, B, files, reps, rounds)
                r["name"] = name
                print(json.dumps({k: v for k, v in r.items() if k not in ("stages", "rounds")}), flush=True)
                out.append(r)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
