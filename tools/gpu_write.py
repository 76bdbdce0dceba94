"""Block writers (mscomp_amd_writer_*) on the bench corpus as a block container: one resource per file (12 files), at the block sizes given.
Reported per (format, block size), HIP events after two warm-ups, mean of `reps` executions, the calls' own graphs:
  a_ms / a_full_ms      one 4 KiB write into 1 % of each resource's blocks (at least one), with checksums, against BlockContainer.compress +
                        .crc of the whole patched data in the same run
  b_ms                  10 000 writes of 64 bytes at seeded random offsets, with checksums
  c_ms                  the writes of (a) without checksum arrays
and for each case, from one profiled execution (plain launches), the time per stage -- tables (admission, owners, lists, fold), patch, layout,
move, crc (both CRC passes), codec (everything the two inner plans launched) -- and the move pass's bytes per second beside a plain device
copy of the packed buffer (copy_ms, copy_gbs). Every result is checked: the new container is decoded and compared with the patched source.
Prints one line per case and a JSON list at the end.
Usage: python tools/gpu_write.py [reps] [block sizes, comma separated; default 32768,65536]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ms_compress_amd as m  # noqa: E402
from ms_compress_amd import corpus  # noqa: E402
from gpu_read import event_ms, tab  # noqa: E402

TABLES = ("rd_req_kernel", "rd_units", "wr_link", "rd_fold_kernel")
CRC = ("crc_tables_kernel", "crc_seed_kernel", "crc_kernel")
OWN = {"tables": TABLES, "patch": ("wr_patch",), "layout": ("wr_layout_kernel",), "move": ("bk_move_kernel",), "crc": CRC}


class Writes:
    """one batch of writes against the container: a writer sized for it, its sources laid out back to back, a new container of its own"""

    def __init__(self, ctx, fmt, B, n, nbt, lens, total, reqs, seed):
        reqs = np.asarray(reqs, dtype=np.uint64).reshape(-1, 3)
        self.reqs, self.nq = reqs, len(reqs)
        o, w = reqs[:, 1], reqs[:, 2]                           # (every request lies inside its resource)
        self.blocks = int(((o + w - 1) // B - o // B + 1).sum())
        self.soff = np.concatenate([[0], np.cumsum(w)]).astype(np.uint64)
        self.src = np.random.RandomState(seed).randint(0, 256, int(self.soff[-1]) + 16).astype(np.uint8)
        self.wr = m.BlockWriter(ctx, fmt, B, n, nbt, self.nq, self.blocks)
        self.d_req, self.d_soff, self.d_src = tab(reqs.reshape(-1)), tab(self.soff[:-1]), torch.from_numpy(self.src).cuda()
        self.d_new = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
        self.d_noff = torch.zeros(nbt + 1, dtype=torch.int64, device="cuda")
        self.d_ncrc = torch.zeros(max(1, nbt), dtype=torch.int32, device="cuda")
        self.d_wr = torch.zeros(self.nq, dtype=torch.int64, device="cuda")
        self.d_st = torch.zeros(self.nq, dtype=torch.int32, device="cuda")
        self.d_rst = torch.zeros(n, dtype=torch.int32, device="cuda")

    def run(self, c, crc=True):
        self.wr.write(c["packed"], c["first"], c["boff"], c["len"], self.d_req, self.d_src, self.d_soff, self.d_new, self.d_noff, self.d_wr, self.d_st,
                      self.d_rst, d_block_crc=c["crc"] if crc else None, d_new_block_crc=self.d_ncrc if crc else None, packed_len=c["total"],
                      new_cap=c["total"])

    def patched(self, c):
        """the source blob with the writes applied in request order (host)"""
        blob = c["blob"].copy()
        for (r, o, w), s in zip(self.reqs, self.soff[:-1]):
            at = int(c["off"][int(r)]) + int(o)
            blob[at: at + int(w)] = self.src[int(s): int(s) + int(w)]
        return blob

    def verify(self, c, bk, crc):
        """every request MSCOMP_OK, the new container decodes to the patched source, and its checksums are the patched blocks'"""
        torch.cuda.synchronize()
        assert not bool(self.d_st.any()) and not bool(self.d_rst.any()) and bool((self.d_wr.cpu().numpy().view(np.uint64) == self.reqs[:, 2]).all())
        want = torch.from_numpy(self.patched(c)).cuda()
        n = len(c["lens"])
        d_out = torch.zeros_like(want)
        d_olen, d_dst = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
        bk.decompress(self.d_new, c["first"], self.d_noff, c["len"], d_out, c["t_off"], c["len"], d_olen, d_dst, packed_len=c["total"])
        if crc:
            bk.check(d_out, c["t_off"], c["len"], c["first"], self.d_ncrc, d_olen, d_dst)
        torch.cuda.synchronize()
        assert not bool(d_dst.any())
        for o, ln in zip(c["off"], c["lens"]):
            assert bool((d_out[int(o): int(o) + ln] == want[int(o): int(o) + ln]).all())
        return want

    def stages(self, ctx, c, crc):
        ctx.profile_enable(True)
        self.run(c, crc)
        prof = ctx.profile_read()
        ctx.profile_enable(False)
        out = {k: sum(prof.get(x, (0.0, 0))[0] for x in names) for k, names in OWN.items()}
        named = {x for names in OWN.values() for x in names}
        out["codec"] = sum(v[0] for k, v in prof.items() if k not in named)
        return {k: round(v, 4) for k, v in out.items()}

    def close(self):
        self.wr.close()


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
    packed_bytes = int(d_boff.cpu().numpy()[int(first[n])])
    c = dict(packed=d_packed, first=d_first, boff=d_boff, len=t_len, total=total, off=off, lens=lens, blob=blob, crc=d_crc, t_off=t_off)
    # a plain device copy of the packed bytes: the move pass's yardstick
    d_copy = torch.zeros_like(d_packed)
    copy_ms = event_ms(lambda: d_copy[:packed_bytes].copy_(d_packed[:packed_bytes]), reps)
    # (a) / (c): a 4 KiB write in the middle of 1 % of every resource's blocks (the block's last bytes when it is shorter)
    cnt = np.diff(first)
    reqs = []
    for r in range(n):
        k = max(1, int(cnt[r]) // 100)
        for jb in np.linspace(0, int(cnt[r]) - 1, k).astype(np.int64):
            at = min(int(jb) * B + B // 2, max(0, lens[r] - 4096))
            reqs.append((r, at, min(4096, lens[r] - at)))
    a = Writes(ctx, fmt, B, n, nbt, lens, total, reqs, 7)
    res = {}
    for key, crc in (("a", True), ("c", False)):
        ms = event_ms(lambda: a.run(c, crc), reps)
        want = a.verify(c, bk, crc)
        res[key] = dict(ms=ms, counts=a.wr.counts(), stages=a.stages(ctx, c, crc))
    # the full re-compress of the patched data
    d_p2, d_f2, d_b2, d_c2 = torch.zeros_like(d_packed), z64(n + 1), z64(nbt + 1), z32(nbt)

    def full():
        bk.compress(want, t_off, t_len, d_p2, d_f2, d_b2, d_st, packed_cap=total)
        bk.crc(want, t_off, t_len, d_c2, d_st)
    a_full = event_ms(full, reps)
    torch.cuda.synchronize()
    new_bytes = int(a.d_noff.cpu().numpy()[-1])
    a.run(c, True)
    torch.cuda.synchronize()
    assert bool((a.d_noff == d_b2).all()) and bool((a.d_new[:new_bytes] == d_p2[:new_bytes]).all()) and bool((a.d_ncrc == d_c2).all())   # rule 10
    a.close()
    # (b) 10 000 x 64 bytes: resources by their share of the bytes, offsets uniform
    rs = np.random.RandomState(2024)
    r = rs.choice(n, size=10000, p=np.asarray(lens, dtype=np.float64) / sum(lens))
    o = (rs.random_sample(10000) * (np.asarray(lens)[r] - 64)).astype(np.uint64)
    b = Writes(ctx, fmt, B, n, nbt, lens, total, np.stack([r.astype(np.uint64), o, np.full(10000, 64, dtype=np.uint64)], axis=1), 8)
    b_ms = event_ms(lambda: b.run(c, True), reps)
    b.verify(c, bk, True)
    res["b"] = dict(ms=b_ms, counts=b.wr.counts(), stages=b.stages(ctx, c, True))
    b.close()
    bk.close()
    out = dict(format=fmt, block=B, resources=n, blocks=int(first[n]), mb=round(total / 1e6, 1), packed_mb=round(packed_bytes / 1e6, 1),
               copy_ms=round(copy_ms, 4), copy_gbs=round(packed_bytes / copy_ms / 1e6, 1), a_requests=len(reqs), a_full_ms=round(a_full, 3),
               a_ratio=round(res["a"]["ms"] / a_full, 3))
    for key in ("a", "b", "c"):
        s = res[key]["stages"]
        out.update({key + "_ms": round(res[key]["ms"], 3), key + "_counts": res[key]["counts"], key + "_stages": s,
                    key + "_move_gbs": round(packed_bytes / s["move"] / 1e6, 1) if s["move"] else None})
    return out


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
