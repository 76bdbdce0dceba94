"""The block sync (mscomp_amd_syncer_sync) on the bench corpus: the store is the corpus as a block container, one resource per file (12
files), B = 65536 and 4096, with checksums. The new version is RAW data: every file with one byte inserted at its front and 4 KiB
written into 1 % of its blocks -- the case diff and match answer with a delta of the whole container. Reported per format and block
size, HIP events after two warm-ups, mean of `reps` executions, the call's own graph:
  sync_ms            the whole call
  scan_ms            its boundary and scan stages (sy_bounds + sy_scan, from profiled executions), beside
  crc_ms             a CrcDevPlan pass over the same new data in the same run: it reads those bytes once, the scan's floor
  decode_ms          BlockContainer.decompress of the whole store: what the call must beat to be worth making
  literal_share      literal bytes over the new data, beside
  match_delta_share  the delta share mscomp_amd_deduper_match gives for the same pair once the new data is compressed into a container
and the mean time of every stage of a profiled execution. The results are checked first: the hits against the blocks that were not
written into, and the header's consequence on the device -- literal runs copied, BlockReader.read with the call's d_req / d_req_off, the
batch compared byte for byte. Prints one line per case and writes the list to profiles/sync.json (or to `out`).
Usage: python tools/gpu_sync.py [reps] [out]"""
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
from gpu_splice import Container, z32, z64  # noqa: E402


def next_version(files, B):
    """(the new files, the store blocks that survive whole in them)"""
    rs = np.random.RandomState(7)
    new, whole = [], 0
    for f in files:
        g = np.array(f, dtype=np.uint8, copy=True)
        nb = len(g) // B
        hit = set(int(k) for k in rs.choice(nb, max(1, nb // 100), replace=False)) if nb else set()
        at = min(100, B - 4096)
        for k in hit:
            g[k * B + at: k * B + at + 4096] = np.frombuffer(rs.bytes(4096), dtype=np.uint8)
        whole += nb - len(hit)
        new.append(np.concatenate([np.frombuffer(rs.bytes(1), dtype=np.uint8), g]))
    return new, whole


def run(ctx, fmt, B, files, reps):
    n = len(files)
    new_files, whole = next_version(files, B)
    store = Container(ctx, fmt, B, files)
    lens = [len(f) for f in new_files]
    total = sum(lens)
    off, _ = m.pack_offsets(lens)
    blob = np.zeros(total + 16 * n + 16, dtype=np.uint8)
    for o, f in zip(off, new_files):
        blob[int(o): int(o) + len(f)] = f
    d_in, d_off, d_len = torch.from_numpy(blob).cuda(), tab(off), tab(lens)
    nc = 2 * (total // B) + 8 * n
    sy = m.BlockSyncer(ctx, fmt, B, n, store.nbt, n, total, nc)
    d_hf, d_req, d_roff, d_lf, d_lit, d_cnt, d_rst, d_st = z64(n + 1), z64(3 * nc), z64(nc), z64(n + 1), z64(2 * (nc + n)), z64(8), z32(n), z32(n)
    sync = lambda: sy.sync(store.view, d_in, d_off, d_len, d_hf, d_req, d_roff, d_lf, d_lit, d_cnt, d_rst, d_st)
    sync_ms = event_ms(sync, reps)
    torch.cuda.synchronize()
    count = [int(x) for x in d_cnt.cpu().tolist()]
    assert not bool(d_rst.any()) and not bool(d_st.any())
    assert count[6] == total - B * count[4] and count[3] <= count[2] <= count[1] <= count[0], count      # (hits beside `whole`: the corpus repeats blocks, and a hit may cover a neighbour's start)
    # the consequence, on the device
    out = torch.full_like(d_in, 0xA5)
    lit = d_lit.cpu().numpy().view(np.uint64)
    for i in range(count[5]):
        o, ln = int(lit[2 * i]), int(lit[2 * i + 1])
        out[o: o + ln] = d_in[o: o + ln]
    rd = m.BlockReader(ctx, fmt, B, n, store.nbt, nc, nc)
    d_cap, d_olen, d_ost = tab([B] * nc), z64(nc), z32(nc)
    read = lambda: rd.read(store.d_packed, store.d_first, store.d_boff, store.t_len, d_req, out, d_roff, d_cap, d_olen, d_ost, d_block_crc=store.d_crc,
                           packed_len=store.packed_bytes)
    read_ms = event_ms(read, reps)
    torch.cuda.synchronize()
    assert not bool(d_ost[: count[4]].any())
    for o, ln in zip(off, lens):
        assert bool((out[int(o): int(o) + ln] == d_in[int(o): int(o) + ln]).all())
    # the stages
    sync()
    ctx.profile_enable(True)
    for _ in range(reps):
        sync()
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    stage = {k: round(v[0] / reps, 4) for k, v in prof.items()}
    scan_ms = stage["sy_bounds"] + stage["sy_scan"]
    # the scan's floor: a CRC pass over the same bytes
    cp = m.CrcDevPlan(ctx, n, total)
    d_crc, d_cst = z32(n), z32(n)
    crc_ms = event_ms(lambda: cp.execute(d_in, d_off, d_len, d_crc, d_cst), reps)
    # decode-all of the store
    d_dec, d_dlen, d_dst = torch.zeros_like(store.d_in), z64(n), z32(n)
    decode_ms = event_ms(lambda: store.bk.decompress(store.d_packed, store.d_first, store.d_boff, store.t_len, d_dec, store.t_off, store.t_len, d_dlen, d_dst,
                                                     packed_len=store.packed_bytes), reps)
    torch.cuda.synchronize()
    assert not bool(d_dst.any()) and not bool(d_cst.any())
    # what match makes of the same pair once the new data is a container
    new = Container(ctx, fmt, B, new_files)
    rows = new.nbt
    dd = m.BlockDeduper.for_match(ctx, B, 1, 2 * n, store.nbt + rows, rows)
    m_cnt, m_st = z64(6), z32(2 * n)
    dd.match([store.view], new.view, z64(n + 1), z64(4 * rows), z64(n + 1), z64(4 * rows), z64(3 * n), m_cnt, m_st)
    torch.cuda.synchronize()
    mcount = [int(x) for x in m_cnt.cpu().tolist()]
    assert not bool(m_st.any())
    for h in (sy, rd, cp, dd, store.bk, new.bk):
        h.close()
    return dict(format=fmt, block=B, resources=n, mb=round(total / 1e6, 1), store_rows=store.nb, whole=whole, n_cand_max=nc, count=count,
                literal_share=round(count[6] / total, 5), match_delta_share=round(mcount[4] / new.packed_bytes, 5), match_fresh=mcount[2],
                sync_ms=round(sync_ms, 4), scan_ms=round(scan_ms, 4), scan_gbs=round(total / scan_ms / 1e6, 1), crc_ms=round(crc_ms, 4),
                crc_gbs=round(total / crc_ms / 1e6, 1), scan_over_crc=round(scan_ms / crc_ms, 2), read_ms=round(read_ms, 4), decode_ms=round(decode_ms, 3),
                sync_over_decode=round(sync_ms / decode_ms, 3), stages=stage)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "sync.json")
    torch.cuda.set_device(0)
    ctx = m.Context()
    files = [corpus.file_bytes(i) for i in range(12)]
    out = []
    for B in (65536, 4096):
        for name, fmt in m.FORMATS.items():
            r = run(ctx, fmt, B, files, reps)
            r["name"] = name
            print(json.dumps(r), flush=True)
            out.append(r)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
