"""CRC-32 in HBM (CrcDevPlan, BlockContainer.crc / .check) on the bench corpus, one resource per file (12 files), at the block sizes given.
Reported, HIP events after two warm-ups, mean of `reps` executions, the calls' own graphs:
  plan_blocks   CrcDevPlan over the blocks as units, input GB/s      plan_files   over the 12 files as 12 units
  plan_small    over 100 000 units of 40 bytes each (the table and seed passes against the fixed grid)
and per (format, block size):
  crc_ms     BlockContainer.crc (block and resource CRCs)
  d_ms       BlockContainer.decompress of every block
  check_ms   BlockContainer.check behind it                                  ratio = check_ms / d_ms
Every CRC is compared with zlib's. Prints one line per case and a JSON list at the end.
Usage: python tools/gpu_crc.py [reps] [block sizes, comma separated; default 32768,65536]"""
import json
import os
import sys
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ms_compress_amd as m  # noqa: E402
from ms_compress_amd import corpus  # noqa: E402


def event_ms(fn, reps):
    fn()
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def tab(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def u32(t, n):
    return t.cpu().numpy().view(np.uint32)[:n]


def plan_gbs(ctx, d_in, offs, lens, want, reps):
    n, total = len(offs), int(np.sum(lens))
    plan = m.CrcDevPlan(ctx, n, total)
    t_off, t_len = tab(offs), tab(lens)
    d_crc, d_st = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    ms = event_ms(lambda: plan.execute(d_in, t_off, t_len, d_crc, d_st), reps)
    assert not bool(d_st.any()) and (u32(d_crc, n) == want).all()
    plan.close()
    return ms, total / ms / 1e6


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    sizes = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [32768, 65536]
    torch.cuda.set_device(0)
    ctx = m.Context()
    files = [corpus.file_bytes(i) for i in range(12)]
    n = len(files)
    lens = [len(f) for f in files]
    off, total = m.pack_offsets(lens)
    blob = np.zeros(total + 16, dtype=np.uint8)
    for o, f in zip(off, files):
        blob[int(o): int(o) + len(f)] = f
    d_in = torch.from_numpy(blob).cuda()
    res_want = np.array([zlib.crc32(bytes(f)) for f in files], dtype=np.uint32)
    out = []
    ms, gbs = plan_gbs(ctx, d_in, off, lens, res_want, reps)
    out.append(dict(case="plan_files", units=n, mb=round(total / 1e6, 1), ms=round(ms, 4), gbs=round(gbs, 1)))
    print(json.dumps(out[-1]), flush=True)
    s_off = np.arange(100000, dtype=np.uint64) * 41
    s_len = np.full(100000, 40, dtype=np.uint64)
    ms, gbs = plan_gbs(ctx, d_in, s_off, s_len, np.array([zlib.crc32(blob[int(o): int(o) + 40].tobytes()) for o in s_off], dtype=np.uint32), reps)
    out.append(dict(case="plan_small", units=100000, mb=4.0, ms=round(ms, 4), gbs=round(gbs, 1)))
    print(json.dumps(out[-1]), flush=True)
    z64 = lambda k: torch.zeros(max(1, k), dtype=torch.int64, device="cuda")
    z32 = lambda k: torch.zeros(max(1, k), dtype=torch.int32, device="cuda")
    t_off, t_len = tab(off), tab(lens)
    for B in sizes:
        b_off = np.concatenate([int(o) + np.arange(0, ln, B, dtype=np.uint64) for o, ln in zip(off, lens)])
        b_len = np.concatenate([np.minimum(B, ln - np.arange(0, ln, B)).astype(np.uint64) for ln in lens])
        blk_want = np.array([zlib.crc32(blob[int(o): int(o) + int(ln)].tobytes()) for o, ln in zip(b_off, b_len)], dtype=np.uint32)
        ms, gbs = plan_gbs(ctx, d_in, b_off, b_len, blk_want, reps)
        out.append(dict(case="plan_blocks", block=B, units=len(b_off), mb=round(total / 1e6, 1), ms=round(ms, 4), gbs=round(gbs, 1)))
        print(json.dumps(out[-1]), flush=True)
        for name, fmt in m.FORMATS.items():
            bk = m.BlockContainer(ctx, fmt, B, n, total)
            M = bk.n_blocks_max
            d_bcrc, d_rcrc, d_kst = z32(M), z32(n), z32(n)
            crc_ms = event_ms(lambda: bk.crc(d_in, t_off, t_len, d_bcrc, d_kst, d_res_crc=d_rcrc), reps)
            nb = len(b_off)
            assert not bool(d_kst.any()) and (u32(d_bcrc, nb) == blk_want).all() and (u32(d_rcrc, n) == res_want).all()
            d_packed, d_first, d_boff, d_st = torch.zeros(total + 16, dtype=torch.uint8, device="cuda"), z64(n + 1), z64(M + 1), z32(n)
            bk.compress(d_in, t_off, t_len, d_packed, d_first, d_boff, d_st, packed_cap=total)
            assert not bool(d_st.any())
            d_out, d_olen, d_dst = torch.zeros(total + 16, dtype=torch.uint8, device="cuda"), z64(n), z32(n)
            d_ms = event_ms(lambda: bk.decompress(d_packed, d_first, d_boff, t_len, d_out, t_off, t_len, d_olen, d_dst, packed_len=total), reps)
            check_ms = event_ms(lambda: bk.check(d_out, t_off, t_len, d_first, d_bcrc, d_olen, d_dst), reps)
            assert not bool(d_dst.any()) and bool((d_out == d_in).all())
            d_out[int(off[5]) + 12345] ^= 1                                   # ... and the check sees one flipped bit
            bk.check(d_out, t_off, t_len, d_first, d_bcrc, d_olen, d_dst)
            assert d_dst.cpu().tolist() == [m.MSCOMP_DATA_ERROR if r == 5 else 0 for r in range(n)]
            bk.close()
            out.append(dict(case="container", name=name, block=B, blocks=nb, mb=round(total / 1e6, 1), crc_ms=round(crc_ms, 4), d_ms=round(d_ms, 4),
                            check_ms=round(check_ms, 4), ratio=round(check_ms / d_ms, 3), crc_gbs=round(total / crc_ms / 1e6, 1),
                            check_gbs=round(total / check_ms / 1e6, 1)))
            print(json.dumps(out[-1]), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
