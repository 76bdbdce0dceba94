"""Block readers (mscomp_amd_reader_*) on the bench corpus as a block container: one resource per file (12 files), at the block sizes given.
Reported per (format, block size), HIP events after two warm-ups, mean of `reps` executions, the calls' own graphs:
  a_read_ms / a_bk_ms   1 % of each resource's blocks (at least one) as whole-block requests, the reader created for that count, against
                        BlockContainer.decompress ranged over the same blocks
  b_ms / b_crc_ms       10 000 requests of 4 KiB at seeded random offsets, without and with d_block_crc
  c_ms                  100 000 requests of 64 bytes: requests/s, output GB/s, and from one profiled execution the gather kernel's own time
                        beside the time of everything the inner decode plan launched
Every read is compared with the slice of the source. Prints one line per case and a JSON list at the end.
Usage: python tools/gpu_read.py [reps] [block sizes, comma separated; default 32768,65536]"""
import json
import os
import sys

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


class Reads:
    """one batch of requests against the container: a reader sized for it, its output laid out back to back"""

    def __init__(self, ctx, fmt, B, n, nbt, lens, reqs):
        reqs = np.asarray(reqs, dtype=np.uint64).reshape(-1, 3)
        self.reqs, self.nq = reqs, len(reqs)
        L = np.asarray(lens, dtype=np.uint64)[reqs[:, 0].astype(np.int64)]
        o = np.minimum(reqs[:, 1], L)
        self.want = w = np.minimum(reqs[:, 2], L - o)
        self.blocks = int(np.where(w > 0, (o + w - 1) // B - o // B + 1, 0).sum())
        self.ooff = np.concatenate([[0], np.cumsum(w)]).astype(np.uint64)
        self.rd = m.BlockReader(ctx, fmt, B, n, nbt, self.nq, self.blocks)
        self.d_req, self.d_ooff, self.d_ocap = tab(reqs.reshape(-1)), tab(self.ooff[:-1]), tab(w)
        self.d_out = torch.zeros(int(self.ooff[-1]) + 16, dtype=torch.uint8, device="cuda")
        self.d_olen = torch.zeros(self.nq, dtype=torch.int64, device="cuda")
        self.d_st = torch.zeros(self.nq, dtype=torch.int32, device="cuda")

    def run(self, c, crc=None):
        self.rd.read(c["packed"], c["first"], c["boff"], c["len"], self.d_req, self.d_out, self.d_ooff, self.d_ocap, self.d_olen, self.d_st,
                     d_block_crc=crc, packed_len=c["total"])

    def verify(self, c):
        """every request MSCOMP_OK and its bytes the slice of the source (gathered on the device by index)"""
        torch.cuda.synchronize()
        assert not bool(self.d_st.any()) and bool((self.d_olen.cpu().numpy().view(np.uint64) == self.want).all())
        src0 = np.asarray(c["off"], dtype=np.int64)[self.reqs[:, 0].astype(np.int64)] + self.reqs[:, 1].astype(np.int64)
        idx = np.repeat(src0 - self.ooff[:-1].astype(np.int64), self.want.astype(np.int64)) + np.arange(int(self.ooff[-1]), dtype=np.int64)
        assert bool((self.d_out[: int(self.ooff[-1])] == c["in"][torch.from_numpy(idx).cuda()]).all())

    def close(self):
        self.rd.close()


def run(ctx, fmt, files, B, reps):
    n = len(files)
    lens = [len(f) for f in files]
    off, total = m.pack_offsets(lens)
    blob = np.zeros(total + 16, dtype=np.uint8)
    for o, f in zip(off, files):
        blob[int(o): int(o) + len(f)] = f
    d_in = torch.from_numpy(blob).cuda()
    z64 = lambda k: torch.zeros(max(1, k), dtype=torch.int64, device="cuda")
    z32 = lambda k: torch.zeros(max(1, k), dtype=torch.int32, device="cuda")
    bk = m.BlockContainer(ctx, fmt, B, n, total)
    nbt = bk.n_blocks_max
    t_off, t_len = tab(off), tab(lens)
    d_packed, d_first, d_boff, d_st, d_crc = torch.zeros(total + 16, dtype=torch.uint8, device="cuda"), z64(n + 1), z64(nbt + 1), z32(n), z32(nbt)
    bk.compress(d_in, t_off, t_len, d_packed, d_first, d_boff, d_st, packed_cap=total)
    bk.crc(d_in, t_off, t_len, d_crc, d_st)
    torch.cuda.synchronize()
    assert not bool(d_st.any())
    first = d_first.cpu().numpy()
    c = dict(packed=d_packed, first=d_first, boff=d_boff, len=t_len, total=total, off=off, **{"in": d_in})
    # (a) 1 % of every resource's blocks, whole
    cnt = np.diff(first)
    rng = np.stack([cnt // 2, np.maximum(1, cnt // 100)], axis=1).astype(np.uint64)
    reqs = [(r, int(jb) * B, B) for r in range(n) for jb in range(int(rng[r][0]), int(rng[r][0] + rng[r][1]))]
    a = Reads(ctx, fmt, B, n, nbt, lens, reqs)
    a_read = event_ms(lambda: a.run(c), reps)
    a.verify(c)
    a_counts = a.rd.counts()
    d_out, d_olen, d_dst, t_rng = torch.zeros(total + 16, dtype=torch.uint8, device="cuda"), z64(n), z32(n), tab(rng.reshape(-1))
    a_bk = event_ms(lambda: bk.decompress(d_packed, d_first, d_boff, t_len, d_out, t_off, t_len, d_olen, d_dst, d_range=t_rng, packed_len=total), reps)
    assert not bool(d_dst.any())
    a.close()
    # (b) 10 000 x 4 KiB, (c) 100 000 x 64 bytes: resources by their share of the bytes, offsets uniform
    rs = np.random.RandomState(2024)
    res = {}
    for key, count, size in (("b", 10000, 4096), ("c", 100000, 64)):
        r = rs.choice(n, size=count, p=np.asarray(lens, dtype=np.float64) / total)
        o = (rs.random_sample(count) * (np.asarray(lens)[r] - size)).astype(np.uint64)
        q = Reads(ctx, fmt, B, n, nbt, lens, np.stack([r.astype(np.uint64), o, np.full(count, size, dtype=np.uint64)], axis=1))
        ms = event_ms(lambda: q.run(c), reps)
        q.verify(c)
        res[key] = dict(ms=ms, counts=q.rd.counts(), out_bytes=int(q.ooff[-1]))
        if key == "b":
            res[key]["crc_ms"] = event_ms(lambda: q.run(c, d_crc), reps)
            q.verify(c)
        else:                                                  # one profiled execution (plain launches): the gather beside the decode
            ctx.profile_enable(True)
            q.run(c)
            prof = ctx.profile_read()
            ctx.profile_enable(False)
            own = ("rd_req_kernel", "rd_units", "rd_fold_kernel", "rd_gather_kernel")
            res[key]["gather_ms"] = prof.get("rd_gather_kernel", (0.0, 0))[0]
            res[key]["decode_ms"] = sum(v[0] for k, v in prof.items() if k not in own)
            res[key]["tables_ms"] = sum(prof.get(k, (0.0, 0))[0] for k in own[:3])
        q.close()
    bk.close()
    rb, rc = res["b"], res["c"]
    return dict(format=fmt, block=B, resources=n, blocks=int(first[n]), mb=round(total / 1e6, 1),
                a_requests=len(reqs), a_counts=a_counts, a_read_ms=round(a_read, 3), a_bk_ms=round(a_bk, 3), a_ratio=round(a_read / a_bk, 3),
                b_counts=rb["counts"], b_ms=round(rb["ms"], 3), b_crc_ms=round(rb["crc_ms"], 3), b_mreq_s=round(10000 / rb["ms"] / 1e3, 2),
                b_out_gbs=round(rb["out_bytes"] / rb["ms"] / 1e6, 2),
                c_counts=rc["counts"], c_ms=round(rc["ms"], 3), c_mreq_s=round(100000 / rc["ms"] / 1e3, 2), c_out_gbs=round(rc["out_bytes"] / rc["ms"] / 1e6, 3),
                c_gather_ms=round(rc["gather_ms"], 4), c_decode_ms=round(rc["decode_ms"], 3), c_tables_ms=round(rc["tables_ms"], 4))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    sizes = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [32768, 65536]
    torch.cuda.set_device(0)
    ctx = m.Context()
    files = [corpus.file_bytes(i) for i in range(12)]
    out = []
    for B in sizes:
        for name, fmt in m.FORMATS.items():
            r = run(ctx, fmt, files, B, reps)
            r["name"] = name
            print(json.dumps(r), flush=True)
            out.append(r)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
