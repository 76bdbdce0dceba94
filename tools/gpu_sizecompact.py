"""The two stages that take device tables since size dev plans and mscomp_amd_compact_dev, against their host-table forms on the same units.
Size leg: a size dev plan (mscomp_amd_plan_create_size_dev) against a host size plan on the rows of tools/gpu_devplan.py (the bench corpus
  cut into 3 239 units of 64 KiB per format; mozilla, 51 MB, as one unit per format): HIP events after a warm-up, the two plans alternated
  in blocks of 5 executions until each has `reps`; results compared entry for entry. large_ms: a size dev plan created with
  MSCOMP_AMD_DEV_LARGE_UNITS, alternated with the host plan in the same way.
Compact leg: mscomp_amd_compact_dev against mscomp_amd_compact_batch on the compressed outputs of the configs[4]-shaped batch (the 12 files,
  16 replicas: Xpress as 51 824 units of 64 KiB, LZNT1 as 192 whole files), outputs at their capacities:
  batch_wall_ms  compact_batch to the end of the stream, host clock (its table upload and synchronise included)
  dev_wall_ms    compact_dev to the end of the stream, host clock
  dev_ms         compact_dev, HIP events (the offset scan and the copy kernel)
  copy_ms        torch copy_ of the same number of bytes, device to device, HIP events: the bandwidth ceiling
  GB/s = bytes moved (read + written = 2 x packed bytes) / time. Kernel-only times of both copy kernels come from a kernel trace of
  `python tools/gpu_sizecompact.py 5 compact`.
Prints one line per case and a JSON list at the end. Usage: python tools/gpu_sizecompact.py [reps] [both|size|compact]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ms_compress_amd as m  # noqa: E402
from ms_compress_amd import corpus  # noqa: E402

REPLICAS = 16


def tab(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def compress(ctx, fmt, units):
    """(d_out, out_off, out_cap, d_out_len, lens on the host) of a host compress plan over the units"""
    lens = [len(u) for u in units]
    in_off, in_total = m.pack_offsets(lens)
    caps = [m.max_compressed_size(fmt, n) + 2 for n in lens]
    c_off, c_total = m.pack_offsets(caps)
    blob = np.zeros(in_total + 16, dtype=np.uint8)
    for o, u in zip(in_off, units):
        blob[int(o): int(o) + len(u)] = u
    n = len(units)
    d_in = torch.from_numpy(blob).cuda()
    d_c = torch.zeros(c_total + 16, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
    p = m.Plan(ctx, fmt, in_off, lens, c_off, caps)
    p.execute(d_in, d_c, d_len, d_st)
    torch.cuda.synchronize()
    p.close()
    assert bool((d_st == 0).all())
    return d_c, c_off, np.array(caps, np.uint64), d_len, d_len.cpu().numpy().view(np.uint64).copy(), c_total


def events_ms(fn, k):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(fa, fb, reps, block=5):
    """mean ms of fa and of fb, run in alternating blocks after a warm-up of each"""
    for _ in range(2):
        fa()
        fb()
    torch.cuda.synchronize()
    ta = tb = 0.0
    done = 0
    while done < reps:
        k = min(block, reps - done)
        ta += events_ms(fa, k)
        tb += events_ms(fb, k)
        done += k
    return ta / reps, tb / reps


def run_size(ctx, fmt, units, label, reps):
    d_c, c_off, _, d_clen, clens, _ = compress(ctx, fmt, units)
    n = len(units)
    res = [[torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda"),
            torch.zeros(n, dtype=torch.int32, device="cuda")] for _ in range(2)]
    t_off = tab(c_off)
    host = m.SizePlan(ctx, fmt, c_off, clens)
    dev = m.SizeDevPlan(ctx, fmt, n, int(clens.sum()))
    host_ms, dev_ms = alternate(lambda: host.execute(d_c, *res[0]), lambda: dev.execute(d_c, t_off, d_clen, *res[1]), reps)
    torch.cuda.synchronize()
    ok = all(torch.equal(a, b) for a, b in zip(*res)) and bool((res[0][2] == 0).all())
    dev.close()
    for t in res[1]:
        t.zero_()
    large = m.SizeDevPlan(ctx, fmt, n, int(clens.sum()), large_units=True)
    _, large_ms = alternate(lambda: host.execute(d_c, *res[0]), lambda: large.execute(d_c, t_off, d_clen, *res[1]), reps)
    torch.cuda.synchronize()
    ok = ok and all(torch.equal(a, b) for a, b in zip(*res)) and m.api.plan_paths(large) == m.api.plan_paths(host)
    host.close()
    large.close()
    r = {"leg": "size", "format": fmt, "units": label, "n_units": n, "in_bytes": int(clens.sum()), "ok": ok,
         "host_ms": round(host_ms, 4), "dev_ms": round(dev_ms, 4), "dev_over_host": round(dev_ms / host_ms, 3),
         "large_ms": round(large_ms, 4), "large_over_host": round(large_ms / host_ms, 3)}
    print("size fmt %d %-26s %s  host %9.4f ms  dev %9.4f ms (x%.3f)  dev, large units %9.4f ms (x%.3f)"
          % (fmt, label, "ok" if ok else "MISMATCH", host_ms, dev_ms, r["dev_over_host"], large_ms, r["large_over_host"]), flush=True)
    return r


def run_compact(ctx, fmt, units, label, reps):
    d_one, off_one, cap_one, d_len_one, clens_one, stride = compress(ctx, fmt, units)
    # the replicas: the same compressed bytes REPLICAS times in memory of their own, offsets shifted
    stride = (stride + 16 + 15) // 16 * 16
    d_src = torch.zeros(stride * REPLICAS, dtype=torch.uint8, device="cuda")
    for r in range(REPLICAS):
        d_src[r * stride: r * stride + d_one.numel()].copy_(d_one)
    out_off = np.concatenate([off_one + np.uint64(r * stride) for r in range(REPLICAS)])
    out_cap = np.tile(cap_one, REPLICAS)
    clens = np.tile(clens_one, REPLICAS)
    d_len, t_off = tab(clens), tab(out_off)
    n, packed = len(clens), int(clens.sum())
    del d_one
    d_pd = torch.zeros(packed + 16, dtype=torch.uint8, device="cuda")
    d_pd_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_pb = torch.zeros(packed + 16, dtype=torch.uint8, device="cuda")
    d_pb_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    lib, P = ctx.lib, lambda t: t.data_ptr()  # noqa: E731

    def batch():
        assert lib.mscomp_amd_compact_batch(ctx._h, n, P(d_src), out_off.ctypes.data, out_cap.ctypes.data, P(d_len), P(d_pb), P(d_pb_off)) == 0

    def dev():
        m.compact_dev(ctx, d_src, t_off, d_len, 1, d_pd, d_pd_off, packed_cap=packed)

    def plain():
        d_pb[:packed].copy_(d_src[:packed])

    def wall(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
            torch.cuda.current_stream().synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps

    batch_wall, dev_wall = wall(batch), wall(dev)
    dev_ms, copy_ms = alternate(dev, plain, reps)
    batch()
    dev()
    torch.cuda.synchronize()
    ok = torch.equal(d_pb_off, d_pd_off) and torch.equal(d_pb[:packed], d_pd[:packed])
    gbs = lambda ms: round(2 * packed / ms / 1e6, 1)  # noqa: E731
    r = {"leg": "compact", "format": fmt, "units": label, "n_units": n, "packed_bytes": packed, "ok": ok,
         "batch_wall_ms": round(batch_wall, 4), "dev_wall_ms": round(dev_wall, 4), "dev_ms": round(dev_ms, 4), "copy_ms": round(copy_ms, 4),
         "batch_wall_GBs": gbs(batch_wall), "dev_wall_GBs": gbs(dev_wall), "dev_GBs": gbs(dev_ms), "copy_GBs": gbs(copy_ms)}
    print("compact fmt %d %-28s %s  %d B  compact_batch wall %8.4f ms (%7.1f GB/s)  compact_dev wall %8.4f ms, events %8.4f ms (%7.1f GB/s)  "
          "copy_ %8.4f ms (%7.1f GB/s)" % (fmt, label, "ok" if ok else "MISMATCH", packed, batch_wall, r["batch_wall_GBs"], dev_wall, dev_ms,
                                          r["dev_GBs"], copy_ms, r["copy_GBs"]), flush=True)
    return r


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    legs = sys.argv[2] if len(sys.argv) > 2 else "both"
    torch.cuda.set_device(0)
    ctx = m.Context()
    files = [corpus.file_bytes(i) for i in range(12)]
    u64k = [f[k:k + 65536] for f in files for k in range(0, len(f), 65536)]
    res = []
    fmts = (m.MSCOMP_LZNT1, m.MSCOMP_XPRESS, m.MSCOMP_XPRESS_HUFF)
    if legs in ("both", "size"):
        moz = files[corpus.NAMES.index("mozilla")]
        for fmt in fmts:
            res.append(run_size(ctx, fmt, u64k, "%d x 64 KiB" % len(u64k), reps))
        for fmt in fmts:
            res.append(run_size(ctx, fmt, [moz], "mozilla, one unit", max(5, reps // 4)))
    if legs in ("both", "compact"):
        res.append(run_compact(ctx, m.MSCOMP_XPRESS, u64k, "%d x 64 KiB" % (len(u64k) * REPLICAS), reps))
        res.append(run_compact(ctx, m.MSCOMP_LZNT1, files, "%d whole files" % (12 * REPLICAS), reps))
    ctx.close()
    print(json.dumps(res))
    return 0 if all(r["ok"] for r in res) else 1


if __name__ == "__main__":
    sys.exit(main())
