"""The device layer (ms_compress_amd/device.py: DeviceBlocks, BlockOps) on the bench corpus as one block container: one resource per file
(12 files), B = 65536, with checksums. One chain -- compress + crc, write (one request of 1000 bytes across the middle of every resource),
resize (the first resource cut by 12345 bytes, the second extended by two blocks and 7 bytes), delta against the first container, patch --
is run four ways on one context and stream:
  host      through the blocks_* conveniences: every call uploads its container, makes its object, synchronises and fetches
  ops       through BlockOps as plain calls: the objects made once, the containers stay in device memory, every result a fresh tensor
  graph     the BlockOps chain captured once in one graph of the stream (BlockOps.graph), replayed
  handles   the same objects called directly with the tensors of a finished chain: what ops costs without its allocations
The patched container of each way is compared with the host way's byte for byte -- packed bytes, tables, checksums -- before anything is
timed. Reported per format: wall time per chain (a chain is complete when the stream is idle: the host way by construction, the others
synchronise once after `reps` chains) for host, ops and graph, and HIP-event time per chain on the stream for handles, ops and graph; each
the median over `rounds` rounds that take the ways by turns, with every round's value and the handles' lowest-to-highest spread. The
layer launches nothing of its own in this chain, so ops_event_ms may exceed handles_event_ms by no more than that spread:
"ops_within_spread" says whether it did. Prints one line per format and writes the list to profiles/device_blocks.json (or to `out`).
Usage: python tools/gpu_device_blocks.py [reps] [out] [rounds]"""
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
from gpu_read import tab  # noqa: E402

B, PAYLOAD, BUDGET = 65536, 1000, 64


def plan(files):
    """the chain's edits: (writes as (resource, offset, bytes), the lengths the resize asks for)"""
    rs = np.random.RandomState(23)
    writes = [(r, len(f) // 2 - PAYLOAD // 2, rs.bytes(PAYLOAD)) for r, f in enumerate(files)]
    want = [len(f) for f in files]
    want[0] -= 12345
    want[1] += 2 * B + 7
    return writes, want


def host_chain(ctx, fmt, bufs, writes, want):
    """the chain through the conveniences over the files as byte strings; returns the patched container (packed, block_first, block_off,
    lengths, block_crc) and the diff's counts"""
    packed, first, off, st = m.blocks_compress(fmt, bufs, B, ctx=ctx)
    crc, _ = m.blocks_crc(fmt, bufs, B, ctx=ctx)
    a = (packed, first, off, [len(b) for b in bufs], crc)
    packed, off, crc, _, wst, rst = m.blocks_write(fmt, *a[:4], B, writes, ctx=ctx, block_crc=a[4])
    assert not st.any() and not any(wst) and not any(rst)
    packed, off, crc, first, lens, rst = m.blocks_resize(fmt, packed, a[1], off, a[3], B, want, ctx=ctx, block_crc=crc)
    c = (packed, first, off, lens, crc)
    delta, recipe, _, counts, dst = m.blocks_delta(a, c, B, ctx=ctx)
    packed, first, off, lens, crc, pst = m.blocks_patch(a, delta, recipe, B, ctx=ctx)
    assert not any(rst) and not any(dst) and not any(pst)
    return (packed, first, off, lens, crc), counts


class Inputs:
    """what the device ways read: the files back to back, their tables, the requests and their payload, the wanted lengths"""

    def __init__(self, files, writes, want):
        lens = [len(f) for f in files]
        off, total = m.pack_offsets(lens)
        blob = np.zeros(total + 16, dtype=np.uint8)
        for o, f in zip(off, files):
            blob[int(o): int(o) + len(f)] = f
        self.d_data, self.d_off, self.d_len = torch.from_numpy(blob).cuda(), tab(off), tab(lens)
        self.d_req = tab(np.array([(r, o, len(b)) for r, o, b in writes], dtype=np.uint64).reshape(-1))
        self.d_src = torch.from_numpy(np.frombuffer(b"".join(b for _, _, b in writes), dtype=np.uint8).copy()).cuda()
        self.d_src_off, self.d_want = tab(np.arange(len(writes)) * PAYLOAD), tab(want)


def ops_chain(ops, x):
    a = ops.compress(x.d_data, x.d_off, x.d_len)
    b, d_wr, d_st = ops.write(a, x.d_req, x.d_src, x.d_src_off)
    c = ops.resize(b, x.d_want)
    d, df = ops.delta(a, c)
    return a, b, c, d, ops.patch(a, d, df), df, d_wr, d_st


def handles_chain(ops, x, made):
    """the calls ops_chain makes, on the objects of ``ops`` and into the tensors of the finished chain ``made``"""
    a, b, c, d, p, df, d_wr, d_st = made
    cap, nq, nbm = ops.in_total_max, x.d_req.numel() // 3, ops.n_blocks_max
    bk, wr, rs, dd = ops._made[("container",)], ops._made[("write", nq)], ops._made[("resize",)], ops._made[("diff",)]
    sp1, sp2 = ops._made[("splice_extents", 1, nbm)], ops._made[("splice_extents", 2, nbm)]

    def run():
        bk.crc(x.d_data, x.d_off, x.d_len, a.block_crc, a.status)
        bk.compress(x.d_data, x.d_off, x.d_len, a.packed, a.block_first, a.block_off, a.status, packed_cap=cap)
        wr.write(a.packed, a.block_first, a.block_off, a.res_len, x.d_req, x.d_src, x.d_src_off, b.packed, b.block_off, d_wr, d_st, b.status,
                 d_block_crc=a.block_crc, d_new_block_crc=b.block_crc, packed_len=cap, new_cap=cap)
        rs.resize(b.packed, b.block_first, b.block_off, b.res_len, x.d_want, c.packed, c.block_first, c.block_off, c.res_len, c.status,
                  d_block_crc=b.block_crc, d_new_block_crc=c.block_crc, packed_len=cap, new_cap=cap)
        dd.diff(a.view(), c.view(), ops._pairs, *df)
        sp1.splice_extents([c.view()], df.delta_ext_first, df.delta_ext, d.packed, d.block_first, d.block_off, d.res_len, d.status,
                           d_new_block_crc=d.block_crc, new_cap=cap)
        sp2.splice_extents([a.view(), d.view()], df.patch_ext_first, df.patch_ext, p.packed, p.block_first, p.block_off, p.res_len, p.status,
                           d_new_block_crc=p.block_crc, new_cap=cap)
    return run


def same(got, want, what):
    for k, name in enumerate(("packed", "block_first", "block_off", "lengths", "block_crc")):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and (a == b).all(), (what, name)


def timed(stream, fn, reps):
    """(wall ms, HIP-event ms) per call of ``fn``, over ``reps`` calls after one warm-up, the stream idle before and after"""
    fn()
    stream.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, a.elapsed_time(b) / reps


def run(ctx, stream, fmt, files, bufs, reps, rounds):
    writes, want = plan(files)
    total = sum(len(f) for f in files)
    t0 = time.perf_counter()
    expect, counts = host_chain(ctx, fmt, bufs, writes, want)
    first_host_ms = (time.perf_counter() - t0) * 1e3
    with torch.cuda.stream(stream):
        x = Inputs(files, writes, want)
        ops = m.BlockOps(ctx, fmt, B, len(files), total + 4 * B)
        ops.prepare("write", n_req=len(writes), blocks_max=BUDGET)
        ops.prepare("resize", blocks_max=BUDGET)
        made = ops_chain(ops, x)
        same(made[4].host(), expect, "the BlockOps chain")
        direct = handles_chain(ops, x, made)
        made[4].packed.zero_()
        direct()
        same(made[4].host(), expect, "the handles' chain")
    stream.synchronize()
    with ops.graph("container", "write", "resize", "diff", "splice_extents") as g:
        captured = ops_chain(ops, x)
    with torch.cuda.stream(stream):
        g.replay()
        same(captured[4].host(), expect, "the captured chain")
        per = {"host": [], "ops": [], "graph": [], "handles": []}
        for _ in range(rounds):
            t0 = time.perf_counter()
            host_chain(ctx, fmt, bufs, writes, want)
            per["host"].append(((time.perf_counter() - t0) * 1e3, None))
            per["handles"].append(timed(stream, direct, reps))
            per["ops"].append(timed(stream, lambda: ops_chain(ops, x), reps))
            per["graph"].append(timed(stream, g.replay, reps))
    med = lambda way, k: float(np.median([v[k] for v in per[way]]))
    ev = lambda way: [round(v[1], 3) for v in per[way]]
    spread = max(ev("handles")) - min(ev("handles"))
    res = {"block_size": B, "n_res": len(files), "in_bytes": total, "packed_bytes": len(expect[0]), "changed_blocks": counts[0], "reps": reps, "rounds": rounds,
           "first_host_ms": round(first_host_ms, 1),
           "host_wall_ms": round(med("host", 0), 1), "ops_wall_ms": round(med("ops", 0), 3), "graph_wall_ms": round(med("graph", 0), 3),
           "handles_wall_ms": round(med("handles", 0), 3),
           "handles_event_ms": round(med("handles", 1), 3), "ops_event_ms": round(med("ops", 1), 3), "graph_event_ms": round(med("graph", 1), 3),
           "handles_event_rounds": ev("handles"), "ops_event_rounds": ev("ops"), "graph_event_rounds": ev("graph"),
           "handles_spread_ms": round(spread, 3), "ops_within_spread": bool(med("ops", 1) - med("handles", 1) <= spread)}
    del g, captured, made
    ops.close()
    return res


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "device_blocks.json")
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    ctx = m.Context(stream=stream)
    files = [corpus.file_bytes(i) for i in range(12)]
    bufs = [f.tobytes() for f in files]
    out = []
    for name, fmt in m.FORMATS.items():
        r = run(ctx, stream, fmt, files, bufs, reps, rounds)
        r["name"] = name
        print(json.dumps(r), flush=True)
        out.append(r)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
