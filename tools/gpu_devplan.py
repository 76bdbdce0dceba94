"""Plans with device tables against host-table plans, on the same units: the bench corpus cut into 64 KiB units (3239 units, each of the
three formats) and one large unit per format (mozilla, 51 MB).
Decompress leg: decompress dev plans against host decompress plans (every input is compressed on the GPU first).
Compress leg: compress dev plans (mscomp_amd_plan_create_compress_dev) against host compress plans on the plain units.
Reported per case (HIP events after a warm-up, mean of `reps` executions):
  host_ms       mscomp_amd_plan_execute of one host plan (its own graph replayed)
  dev_ms        mscomp_amd_plan_execute_dev of one dev plan, tables in device memory (its own graph replayed)
  large_ms      the same of a dev plan created with MSCOMP_AMD_DEV_LARGE_UNITS (decompress leg; compress plans have no such paths)
  host_batch_ms create + execute + destroy of a host plan per batch, to the end of the batch (host clock)
  dev_batch_ms  one dev plan executed per batch, tables written on the device, to the end of the batch (host clock)
The outputs of both plans are compared byte for byte. Prints one line per case and a JSON list at the end.
Usage: python tools/gpu_devplan.py [reps] [both|decompress|compress]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ms_compress_amd as m  # noqa: E402
from ms_compress_amd import corpus  # noqa: E402


def event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def wall_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) * 1e3 / reps


def tab(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def run(ctx, fmt, units, label, reps):
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
    clens = np.array([int(x) for x in d_len.cpu()], dtype=np.uint64)
    del d_in
    lens = np.array(lens, dtype=np.uint64)
    d_ho = torch.zeros(in_total + 16, dtype=torch.uint8, device="cuda")
    d_do = torch.zeros(in_total + 16, dtype=torch.uint8, device="cuda")
    d_hl, d_dl = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
    d_hs, d_ds = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    t_coff, t_clen, t_ooff, t_ocap = tab(c_off), tab(clens), tab(in_off), tab(lens)
    q = m.Plan(ctx, fmt, c_off, clens, in_off, lens, decompress=True)
    d = m.DevPlan(ctx, fmt, n, int(clens.sum()), int(lens.sum()))
    host_ms = event_ms(lambda: q.execute(d_c, d_ho, d_hl, d_hs), reps)
    dev_ms = event_ms(lambda: d.execute(d_c, t_coff, t_clen, d_do, t_ooff, t_ocap, d_dl, d_ds), reps)
    torch.cuda.synchronize()
    ok = bool((d_hs == 0).all()) and torch.equal(d_hs, d_ds) and torch.equal(d_hl, d_dl) and torch.equal(d_ho, d_do)
    host_paths = m.api.plan_paths(q)
    q.close()
    for t in (d_do, d_dl, d_ds):
        t.zero_()
    g = m.DevPlan(ctx, fmt, n, int(clens.sum()), int(lens.sum()), large_units=True)
    large_ms = event_ms(lambda: g.execute(d_c, t_coff, t_clen, d_do, t_ooff, t_ocap, d_dl, d_ds), reps)
    torch.cuda.synchronize()
    ok = ok and torch.equal(d_hs, d_ds) and torch.equal(d_hl, d_dl) and torch.equal(d_ho, d_do) and m.api.plan_paths(g) == host_paths

    def host_batch():
        h = m.Plan(ctx, fmt, c_off, clens, in_off, lens, decompress=True)
        h.execute(d_c, d_ho, d_hl, d_hs)
        h.close()                                                    # (synchronizes the stream)

    def dev_batch():
        t_clen.copy_(d_len)                                          # the batch's tables come from earlier GPU work
        d.execute(d_c, t_coff, t_clen, d_do, t_ooff, t_ocap, d_dl, d_ds)
        torch.cuda.current_stream().synchronize()

    host_batch_ms = wall_ms(host_batch, reps)
    dev_batch_ms = wall_ms(dev_batch, reps)
    d.close()

    def large_batch():
        t_clen.copy_(d_len)
        g.execute(d_c, t_coff, t_clen, d_do, t_ooff, t_ocap, d_dl, d_ds)
        torch.cuda.current_stream().synchronize()

    large_batch_ms = wall_ms(large_batch, reps)
    g.close()
    out = int(lens.sum())
    r = {"format": fmt, "units": label, "n_units": n, "in_bytes": int(clens.sum()), "out_bytes": out, "ok": ok,
         "host_ms": round(host_ms, 3), "dev_ms": round(dev_ms, 3), "dev_over_host": round(dev_ms / host_ms, 3),
         "large_ms": round(large_ms, 3), "large_over_host": round(large_ms / host_ms, 3), "large_over_dev": round(large_ms / dev_ms, 3),
         "paths": list(host_paths),
         "host_batch_ms": round(host_batch_ms, 3), "dev_batch_ms": round(dev_batch_ms, 3), "batch_ratio": round(dev_batch_ms / host_batch_ms, 3),
         "large_batch_ms": round(large_batch_ms, 3)}
    print("fmt %d %-26s %s  host %8.3f ms  dev %8.3f ms (x%.3f)  dev, large units %8.3f ms (x%.3f of host)  per batch: create+execute %8.3f ms, dev plan %8.3f ms (x%.3f), large units %8.3f ms"
          % (fmt, label, "ok" if ok else "MISMATCH", host_ms, dev_ms, r["dev_over_host"], large_ms, r["large_over_host"], host_batch_ms, dev_batch_ms,
             r["batch_ratio"], large_batch_ms), flush=True)
    return r


def run_compress(ctx, fmt, units, label, reps):
    lens = [len(u) for u in units]
    in_off, in_total = m.pack_offsets(lens)
    caps = [m.max_compressed_size(fmt, n) + 2 for n in lens]
    c_off, c_total = m.pack_offsets(caps)
    blob = np.zeros(in_total + 16, dtype=np.uint8)
    for o, u in zip(in_off, units):
        blob[int(o): int(o) + len(u)] = u
    n = len(units)
    lens, caps = np.array(lens, dtype=np.uint64), np.array(caps, dtype=np.uint64)
    d_in = torch.from_numpy(blob).cuda()
    d_ho = torch.zeros(c_total + 16, dtype=torch.uint8, device="cuda")
    d_do = torch.zeros(c_total + 16, dtype=torch.uint8, device="cuda")
    d_hl, d_dl = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
    d_hs, d_ds = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    t_ioff, t_ilen, t_coff, t_ccap = tab(in_off), tab(lens), tab(c_off), tab(caps)
    q = m.Plan(ctx, fmt, in_off, lens, c_off, caps)
    d = m.CompressDevPlan(ctx, fmt, n, int(lens.sum()), int(lens.max()))
    host_ms = event_ms(lambda: q.execute(d_in, d_ho, d_hl, d_hs), reps)
    dev_ms = event_ms(lambda: d.execute(d_in, t_ioff, t_ilen, d_do, t_coff, t_ccap, d_dl, d_ds), reps)
    torch.cuda.synchronize()
    ok = bool((d_hs == 0).all()) and torch.equal(d_hs, d_ds) and torch.equal(d_hl, d_dl)
    if ok:
        ho, do, hl = d_ho.cpu().numpy(), d_do.cpu().numpy(), d_hl.cpu().numpy()
        ok = all(np.array_equal(ho[int(o): int(o) + int(k)], do[int(o): int(o) + int(k)]) for o, k in zip(c_off, hl))
    q.close()
    src_len = tab(lens)

    def host_batch():
        h = m.Plan(ctx, fmt, in_off, lens, c_off, caps)
        h.execute(d_in, d_ho, d_hl, d_hs)
        h.close()                                                    # (synchronizes the stream)

    def dev_batch():
        t_ilen.copy_(src_len)                                        # the batch's tables come from earlier GPU work
        d.execute(d_in, t_ioff, t_ilen, d_do, t_coff, t_ccap, d_dl, d_ds)
        torch.cuda.current_stream().synchronize()

    host_batch_ms = wall_ms(host_batch, reps)
    dev_batch_ms = wall_ms(dev_batch, reps)
    d.close()
    r = {"leg": "compress", "format": fmt, "units": label, "n_units": n, "in_bytes": int(lens.sum()), "out_bytes": int(d_hl.sum()), "ok": ok,
         "host_ms": round(host_ms, 3), "dev_ms": round(dev_ms, 3), "dev_over_host": round(dev_ms / host_ms, 3),
         "host_batch_ms": round(host_batch_ms, 3), "dev_batch_ms": round(dev_batch_ms, 3), "batch_ratio": round(dev_batch_ms / host_batch_ms, 3)}
    print("compress fmt %d %-26s %s  host %8.3f ms  dev %8.3f ms (x%.3f)  per batch: create+execute %8.3f ms, dev plan %8.3f ms (x%.3f)"
          % (fmt, label, "ok" if ok else "MISMATCH", host_ms, dev_ms, r["dev_over_host"], host_batch_ms, dev_batch_ms, r["batch_ratio"]), flush=True)
    return r


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    legs = sys.argv[2] if len(sys.argv) > 2 else "both"
    torch.cuda.set_device(0)
    ctx = m.Context()
    files = [corpus.file_bytes(i) for i in range(12)]
    u64k = [f[k:k + 65536] for f in files for k in range(0, len(f), 65536)]
    moz = corpus.file_bytes(corpus.NAMES.index("mozilla"), 51_220_480)
    res = []
    fmts = (m.MSCOMP_LZNT1, m.MSCOMP_XPRESS, m.MSCOMP_XPRESS_HUFF)
    if legs in ("both", "decompress"):
        for fmt in fmts:
            res.append(run(ctx, fmt, u64k, "%d x 64 KiB" % len(u64k), reps))
        for fmt in fmts:
            res.append(run(ctx, fmt, [moz], "mozilla, one stream", max(3, reps // 4)))
    if legs in ("both", "compress"):
        for fmt in fmts:
            res.append(run_compress(ctx, fmt, u64k, "%d x 64 KiB" % len(u64k), reps))
        for fmt in fmts:
            res.append(run_compress(ctx, fmt, [moz], "mozilla, one unit", max(3, reps // 4)))
    ctx.close()
    print(json.dumps(res))
    return 0 if all(r["ok"] for r in res) else 1


if __name__ == "__main__":
    sys.exit(main())
