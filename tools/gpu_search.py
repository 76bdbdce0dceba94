"""The block searcher (mscomp_amd_searcher_search) on the bench corpus: the corpus as a block container, one resource per file (12 files),
B = 65536 and 4096, with checksums; one request per resource, whole; 1, 8 and 64 patterns of 4 to 16 bytes cut from the corpus at seeded
places, and one pattern that never occurs, alone. Reported per format, block size and pattern set, HIP events after
two warm-ups, mean of `reps` executions, the legs alternated in rounds of one execution each:
  search_ms          the whole call, its own graph, beside
  read_ms            BlockReader.read of the same ranges in the same rounds: admission, owners, decode, CRC, fold and the gather -- the
                     decode is the floor the searcher cannot go below
  crc_ms, copy_ms    a CrcDevPlan pass over the same (raw) bytes and a device copy of them, in the same rounds
  scan_ms            the count and emit passes alone (sr_count_kernel + sr_emit_kernel, from profiled executions), front_ms the passes in
                     front of them: what the searcher shares with the reader
  filter_share       positions whose four bytes pass the prefix filter of some pattern, confirm_share those that are hits, over all
                     positions (computed with torch on the raw bytes)
and the mean time of every stage of a profiled execution. The results are checked first, on the device, against the raw bytes: every
record is an occurrence of its pattern, the records ascend in (q, x, p), and the exact counts per request are those of a comparison at
every position. Prints one line per case and writes the list to profiles/search.json (or to `out`).
Usage: python tools/gpu_search.py [reps] [out]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ms_compress_amd as m  # noqa: E402
from ms_compress_amd import corpus  # noqa: E402
from gpu_read import tab  # noqa: E402
from gpu_splice import Container, z32, z64  # noqa: E402

HITS_MAX = 1 << 22
NEVER = bytes([0xFE, 0x01, 0xFD, 0x02, 0xFC, 0x03, 0xFB, 0x04, 0xFA, 0x05, 0xF9, 0x06])


def patterns(files, n_pat):
    """n_pat byte strings of 4 to 16 bytes from seeded places of the files; 0: the one that occurs nowhere"""
    rs = np.random.RandomState(11)
    out = []
    for _ in range(n_pat):
        f = files[int(rs.randint(0, len(files)))]
        ln = int(rs.randint(4, 17))
        at = int(rs.randint(0, len(f) - ln))
        out.append(bytes(f[at: at + ln]))
    return out or [NEVER]


def alternate(legs, reps):
    """mean ms per execution of every leg: two warm-ups each, then `reps` rounds of one execution of each leg by turns"""
    for fn in legs.values():
        fn(); fn()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for k in legs}
    for i in range(reps):
        for k, fn in legs.items():
            ev[k][i][0].record(); fn(); ev[k][i][1].record()
    torch.cuda.synchronize()
    return {k: sum(a.elapsed_time(b) for a, b in v) / reps for k, v in ev.items()}


def expected(d_in, off, lens, pats):
    """on the device, from the raw bytes: hits per resource (the comparison at every position), positions passing the four-byte filter"""
    per_res, passing = [], 0
    keys = torch.tensor(sorted({int.from_bytes(p[:4], "little") for p in pats}), dtype=torch.int64, device="cuda")
    for o, L in zip(off, lens):
        d = d_in[int(o): int(o) + L]
        hits = 0
        for p in pats:
            if len(p) <= L:
                ok = torch.ones(L - len(p) + 1, dtype=torch.bool, device="cuda")
                for k, b in enumerate(p):
                    ok &= d[k: L - len(p) + 1 + k] == b
                hits += int(ok.sum())
        per_res.append(hits)
        if L >= 4:
            key = d[: L - 3].to(torch.int64) | (d[1: L - 2].to(torch.int64) << 8) | (d[2: L - 1].to(torch.int64) << 16) | (d[3:].to(torch.int64) << 24)
            passing += int(torch.isin(key, keys).sum())
    return per_res, passing


def check(con, d_hits, d_rh, d_cnt, d_pst, d_st, pats, want):
    torch.cuda.synchronize()
    total, written = (int(x) for x in d_cnt.cpu().tolist())
    assert not bool(d_st.any()) and not bool(d_pst.any())
    assert [int(x) for x in d_rh.cpu().tolist()] == want and total == sum(want) and written == min(total, HITS_MAX), (total, written, want)
    x, w = d_hits[0: 2 * written: 2], d_hits[1: 2 * written: 2]
    q, p = w >> 32, w & 0xFFFFFFFF
    rise = (q[1:] > q[:-1]) | ((q[1:] == q[:-1]) & ((x[1:] > x[:-1]) | ((x[1:] == x[:-1]) & (p[1:] > p[:-1]))))
    assert bool(rise.all()), "the records do not ascend"
    table = torch.zeros((len(pats), 16), dtype=torch.uint8, device="cuda")
    for i, pt in enumerate(pats):
        table[i, : len(pt)] = torch.tensor(list(pt), dtype=torch.uint8)
    plen = torch.tensor([len(pt) for pt in pats], dtype=torch.int64, device="cuda")
    for lo in range(0, written, 1 << 20):
        g = con.t_off[q[lo: lo + (1 << 20)]] + x[lo: lo + (1 << 20)]
        pp = p[lo: lo + (1 << 20)]
        col = torch.arange(16, device="cuda")
        same = (con.d_in[g[:, None] + col] == table[pp]) | (col[None, :] >= plen[pp][:, None])
        assert bool(same.all()), "a record is not an occurrence"
    return total, written


def run(ctx, fmt, B, files, reps, sets):
    n = len(files)
    con = Container(ctx, fmt, B, files)
    total = con.total
    reqs = tab(np.array([(r, 0, (1 << 64) - 1) for r in range(n)], dtype=np.uint64).reshape(-1))
    blocks = con.nb + n                                            # every block, and a look-ahead block per request at the most
    rd = m.BlockReader(ctx, fmt, B, n, con.nbt, n, blocks)
    d_out, d_olen, d_ost = torch.zeros_like(con.d_in), z64(n), z32(n)
    read = lambda: rd.read(con.d_packed, con.d_first, con.d_boff, con.t_len, reqs, d_out, con.t_off, con.t_len, d_olen, d_ost, d_block_crc=con.d_crc,
                           packed_len=con.packed_bytes)
    cp = m.CrcDevPlan(ctx, n, total)
    d_crc, d_cst = z32(n), z32(n)
    crc = lambda: cp.execute(con.d_in, con.t_off, con.t_len, d_crc, d_cst)
    d_copy = torch.empty_like(con.d_in)
    copy = lambda: d_copy.copy_(con.d_in)
    d_hits, d_rh, d_cnt, d_st = z64(2 * HITS_MAX), z64(n), z64(2), z32(n)
    out = []
    for pats, (want, passing) in sets:
        sr = m.BlockSearcher(ctx, fmt, B, n, con.nbt, n, blocks, len(pats), 16, HITS_MAX)
        d_pat = torch.from_numpy(np.frombuffer(b"".join(pats) + bytes(16), dtype=np.uint8).copy()).cuda()
        d_poff, d_pst = tab(np.cumsum([0] + [len(p) for p in pats])), z32(len(pats))
        search = lambda: sr.search(con.d_packed, con.packed_bytes, con.d_first, con.d_boff, con.t_len, con.d_crc, reqs, d_pat, d_poff, d_hits, d_rh, d_cnt, d_pst, d_st)
        search()
        hits, written = check(con, d_hits, d_rh, d_cnt, d_pst, d_st, pats, want)
        ms = alternate({"search": search, "read": read, "crc": crc, "copy": copy}, reps)
        torch.cuda.synchronize()
        assert not bool(d_ost.any()) and not bool(d_cst.any())
        ctx.profile_enable(True)
        for _ in range(reps):
            search()
        prof = ctx.profile_read()
        ctx.profile_enable(False)
        stage = {k: round(v[0] / reps, 4) for k, v in prof.items()}
        scan_ms = stage.get("sr_count_kernel", 0.0) + stage.get("sr_emit_kernel", 0.0)
        front_ms = sum(v for k, v in stage.items() if not k.startswith("sr_") or k == "sr_req_kernel")
        counts = sr.counts()
        sr.close()
        out.append(dict(format=fmt, block=B, resources=n, mb=round(total / 1e6, 1), patterns=len(pats), never=pats[0] == NEVER, hits=hits, records=written, counts=counts,
                        search_ms=round(ms["search"], 4), read_ms=round(ms["read"], 4), crc_ms=round(ms["crc"], 4), copy_ms=round(ms["copy"], 4),
                        search_over_read=round(ms["search"] / ms["read"], 3), scan_ms=round(scan_ms, 4), front_ms=round(front_ms, 4),
                        scan_gbs=round(total / scan_ms / 1e6, 1) if scan_ms else None, scan_over_front=round(scan_ms / front_ms, 3) if front_ms else None,
                        scan_over_crc=round(scan_ms / ms["crc"], 2), scan_over_copy=round(scan_ms / ms["copy"], 2),
                        filter_share=round(passing / total, 6), confirm_share=round(hits / total, 6), stages=stage))
    for h in (rd, cp, con.bk):
        h.close()
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "search.json")
    torch.cuda.set_device(0)
    ctx = m.Context()
    files = [corpus.file_bytes(i) for i in range(12)]
    lens = [len(f) for f in files]
    off, _ = m.pack_offsets(lens)
    blob = np.zeros(sum(lens) + 16 * len(files) + 16, dtype=np.uint8)
    for o, f in zip(off, files):
        blob[int(o): int(o) + len(f)] = f
    d_in = torch.from_numpy(blob).cuda()
    sets = []
    for n_pat in (1, 8, 64, 0):
        pats = patterns(files, n_pat)
        sets.append((pats, expected(d_in, off, lens, pats)))
    del d_in
    out = []
    for B in (65536, 4096):
        for name, fmt in m.FORMATS.items():
            for r in run(ctx, fmt, B, files, reps, sets):
                r["name"] = name
                print(json.dumps(r), flush=True)
                out.append(r)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
