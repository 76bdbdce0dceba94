"""Decompressed-size query against decoding, on the same units: the bench corpus (BASELINE configs[2..4]: the 12 files cut into 64 KiB
units, for each of the three formats; Xpress+Huffman also as 12 files, one buffer each), the 51 MB mozilla-like LZNT1 unit, and one
large Xpress stream (mozilla as one stream). Every input is compressed on the GPU first; the size pass is checked against the lengths,
then both passes are timed (mean of `reps` executions of one plan, after a warm-up). Prints one line per case and a JSON list at the end.
Usage: python tools/gpu_sizes.py [reps]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ms_compress_amd as m  # noqa: E402
from ms_compress_amd import corpus  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def run(ctx, fmt, units, label, reps):
    dev = torch.device("cuda", ctx.device)
    lens = [len(u) for u in units]
    in_off, in_total = m.pack_offsets(lens)
    caps = [m.max_compressed_size(fmt, n) + 2 for n in lens]
    c_off, c_total = m.pack_offsets(caps)
    blob = np.zeros(in_total + 16, dtype=np.uint8)
    for o, u in zip(in_off, units):
        blob[int(o): int(o) + len(u)] = u
    d_in = torch.from_numpy(blob).to(dev)
    d_c = torch.zeros(c_total + 16, dtype=torch.uint8, device=dev)
    n = len(units)
    d_len = torch.zeros(n, dtype=torch.int64, device=dev)
    d_st = torch.zeros(n, dtype=torch.int32, device=dev)
    p = m.Plan(ctx, fmt, in_off, lens, c_off, caps)
    p.execute(d_in, d_c, d_len, d_st)
    torch.cuda.synchronize()
    p.close()
    assert bool((d_st == 0).all())
    clens = [int(x) for x in d_len.cpu()]
    del d_in
    # the size pass (no limits) and the decoder with exact capacities, on the same compressed units
    d_ol = torch.zeros(n, dtype=torch.int64, device=dev)
    d_need = torch.zeros(n, dtype=torch.int64, device=dev)
    d_s2 = torch.zeros(n, dtype=torch.int32, device=dev)
    sp = m.SizePlan(ctx, fmt, c_off, clens)
    sp.execute(d_c, d_ol, d_need, d_s2)
    torch.cuda.synchronize()
    ok = bool((d_s2 == 0).all()) and [int(x) for x in d_ol.cpu()] == lens and [int(x) for x in d_need.cpu()] == lens
    t_size = timed(lambda: sp.execute(d_c, d_ol, d_need, d_s2), reps)
    d_out = torch.zeros(in_total + 16, dtype=torch.uint8, device=dev)
    q = m.Plan(ctx, fmt, c_off, clens, in_off, lens, decompress=True)
    t_dec = timed(lambda: q.execute(d_c, d_out, d_len, d_st), reps)
    ok = ok and bool((d_st == 0).all())
    sp.close()
    q.close()
    cin, out = sum(clens), sum(lens)
    r = {"format": fmt, "units": label, "n_units": n, "in_bytes": cin, "out_bytes": out, "ok": ok,
         "size_ms": round(t_size * 1e3, 3), "size_in_GBps": round(cin / t_size / 1e9, 2), "size_out_GBps": round(out / t_size / 1e9, 2),
         "decode_ms": round(t_dec * 1e3, 3), "decode_out_GBps": round(out / t_dec / 1e9, 2), "decode_over_size": round(t_dec / t_size, 2)}
    print("fmt %d %-28s %s  size %8.3f ms (%7.2f GB/s in)  decode %8.3f ms (%7.2f GB/s out)  decode/size %.2f"
          % (fmt, label, "ok" if ok else "MISMATCH", r["size_ms"], r["size_in_GBps"], r["decode_ms"], r["decode_out_GBps"], r["decode_over_size"]), flush=True)
    return r


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    torch.cuda.set_device(0)
    ctx = m.Context()
    files = [corpus.file_bytes(i) for i in range(12)]
    u64k = [f[k:k + 65536] for f in files for k in range(0, len(f), 65536)]
    moz = corpus.file_bytes(corpus.NAMES.index("mozilla"), 51_220_480)
    res = []
    for fmt in (2, 3, 4):
        res.append(run(ctx, fmt, u64k, "%d units of 64 KiB" % len(u64k), reps))
    res.append(run(ctx, 4, files, "12 files", reps))
    res.append(run(ctx, 2, [moz], "mozilla, one unit", reps))
    res.append(run(ctx, 3, [moz], "mozilla, one stream", reps))
    ctx.close()
    print(json.dumps(res))
    return 0 if all(r["ok"] for r in res) else 1


if __name__ == "__main__":
    sys.exit(main())
