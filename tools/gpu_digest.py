"""The block digests (mscomp_amd_digester_*, mscomp_amd_syncer_sync_digest) on the workload of tools/gpu_sync.py: the bench corpus as a
block container of 12 resources, B = 65536 and 4096; the new version is raw data, every file with one byte inserted at its front and
4 KiB written into 1 % of its blocks. The consequence is checked on the device before anything is timed -- the digest syncer's outputs
against the syncer's (all but d_count[7]), literal runs copied, BlockReader.read with the call's d_req / d_req_off, the batch compared
byte for byte. HIP events after two warm-ups, mean of `reps` executions. Reported:
  per block size    digest_ms / digest_gbs of BlockDigester.blocks over the store's data beside crc_ms / crc_gbs of BlockContainer.crc over
                    the same bytes; leaf_ms and root_ms from profiled executions; at B = 524288 the same (the 128-compression root)
  per codec         sync_ms of BlockSyncer.sync and sync_digest_ms of sync_digest in the same run, the stages of both from profiled
                    executions, and the device memory each syncer's creation took (free memory before and after)
Prints one line per case and writes the list to profiles/digest.json (or to `out`).
Usage: python tools/gpu_digest.py [reps] [out]"""
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
from gpu_sync import next_version  # noqa: E402


def stages(ctx, fn, reps):
    fn()
    ctx.profile_enable(True)
    for _ in range(reps):
        fn()
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    return {k: round(v[0] / reps, 4) for k, v in prof.items()}


def held(make):
    """(object, device bytes its creation took)"""
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    obj = make()
    torch.cuda.synchronize()
    return obj, free0 - torch.cuda.mem_get_info()[0]


def digest_pass(ctx, store, B, reps):
    """the digest column of the store's data, beside the CRC pass over the same bytes: (record, device column)"""
    n, total = store.n, store.total
    dg = m.BlockDigester(ctx, B, n, total)
    d_dig, d_st, d_crc = z32(4 * dg.n_blocks_max), z32(n), z32(dg.n_blocks_max)
    blocks = lambda: dg.blocks(store.d_in, store.t_off, store.t_len, d_dig, d_st)
    crc = lambda: store.bk.crc(store.d_in, store.t_off, store.t_len, d_crc, d_st)
    digest_ms = event_ms(blocks, reps)
    crc_ms = event_ms(crc, reps)
    torch.cuda.synchronize()
    assert not bool(d_st.any())
    st = stages(ctx, blocks, reps)
    # a sample of the column against hashlib: the first and last block of every resource
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import digest_model as G
    first = store.d_first.cpu().numpy().view(np.uint64)
    dig = d_dig.cpu().numpy().view(np.uint32).reshape(-1, 4)
    blob = store.d_in.cpu().numpy()
    for r in range(n):
        o, L = int(store.off[r]), store.lens[r]
        for k in {0, (L - 1) // B} if L else ():
            assert dig[int(first[r]) + k].tobytes() == G.block_digest(blob[o + k * B: o + min(L, (k + 1) * B)].tobytes()), (r, k)
    dg.close()
    rec = dict(block=B, mb=round(total / 1e6, 1), blocks=int(first[n]), digest_ms=round(digest_ms, 4), digest_gbs=round(total / digest_ms / 1e6, 1),
               crc_ms=round(crc_ms, 4), crc_gbs=round(total / crc_ms / 1e6, 1), leaf_ms=st["dg_leaf_kernel"], root_ms=st["dg_root_kernel"],
               leaf_gbs=round(total / st["dg_leaf_kernel"] / 1e6, 1), stages=st)
    return rec, d_dig


def run(ctx, fmt, B, files, store, d_dig, reps):
    n = len(files)
    new_files, whole = next_version(files, B)
    lens = [len(f) for f in new_files]
    total = sum(lens)
    off, _ = m.pack_offsets(lens)
    blob = np.zeros(total + 16 * n + 16, dtype=np.uint8)
    for o, f in zip(off, new_files):
        blob[int(o): int(o) + len(f)] = f
    d_in, d_off, d_len = torch.from_numpy(blob).cuda(), tab(off), tab(lens)
    nc = 2 * (total // B) + 8 * n
    sy, sy_bytes = held(lambda: m.BlockSyncer(ctx, fmt, B, n, store.nbt, n, total, nc))
    dy, dy_bytes = held(lambda: m.BlockSyncer.for_digest(ctx, B, n, store.nbt, n, total, nc))
    outs = lambda: (z64(n + 1), z64(3 * nc), z64(nc), z64(n + 1), z64(2 * (nc + n)), z64(8), z32(n), z32(n))
    a, b = outs(), outs()
    sync = lambda: sy.sync(store.view, d_in, d_off, d_len, *a)
    blind = (None,) + tuple(store.view[1:])                    # the digest syncer gets no stored byte
    sync_digest = lambda: dy.sync_digest(blind, d_dig, d_in, d_off, d_len, *b)
    # the consequence, before anything is timed
    sync(); sync_digest()
    torch.cuda.synchronize()
    count, dcount = [int(x) for x in a[5].cpu().tolist()], [int(x) for x in b[5].cpu().tolist()]
    assert not bool(b[6].any()) and not bool(b[7].any())
    assert dcount[:7] == count[:7] and dcount[7] == dcount[2] and all(bool((x == y).all()) for x, y in zip(a[:5] + a[6:], b[:5] + b[6:]))
    d_hf, d_req, d_roff, d_lf, d_lit = b[:5]
    out = torch.full_like(d_in, 0xA5)
    lit = d_lit.cpu().numpy().view(np.uint64)
    for i in range(dcount[5]):
        o, ln = int(lit[2 * i]), int(lit[2 * i + 1])
        out[o: o + ln] = d_in[o: o + ln]
    rd = m.BlockReader(ctx, fmt, B, n, store.nbt, nc, nc)
    d_cap, d_olen, d_ost = tab([B] * nc), z64(nc), z32(nc)
    rd.read(store.d_packed, store.d_first, store.d_boff, store.t_len, d_req, out, d_roff, d_cap, d_olen, d_ost, d_block_crc=store.d_crc, packed_len=store.packed_bytes)
    torch.cuda.synchronize()
    assert not bool(d_ost[: dcount[4]].any())
    for o, ln in zip(off, lens):
        assert bool((out[int(o): int(o) + ln] == d_in[int(o): int(o) + ln]).all())
    # the times, in the same run
    sync_ms = event_ms(sync, reps)
    sync_digest_ms = event_ms(sync_digest, reps)
    st_a, st_b = stages(ctx, sync, reps), stages(ctx, sync_digest, reps)
    confirm = lambda st: round(sum(v for k, v in st.items() if not k.startswith(("sy_clear", "sy_seed", "dd_rows", "sy_keys", "sy_units", "sy_bounds", "sy_scan",
                                                                                   "sy_select"))), 4)
    for h in (sy, dy, rd):
        h.close()
    return dict(format=fmt, block=B, resources=n, mb=round(total / 1e6, 1), whole=whole, n_cand_max=nc, count=count, digest_count=dcount,
                sync_ms=round(sync_ms, 4), sync_digest_ms=round(sync_digest_ms, 4), speedup=round(sync_ms / sync_digest_ms, 2),
                confirm_ms=confirm(st_a), confirm_digest_ms=confirm(st_b), syncer_bytes=int(sy_bytes), digest_syncer_bytes=int(dy_bytes),
                digest_extra_formula=nc * (16 * B // 1024 + 32) + 64, stages=st_a, digest_stages=st_b)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "digest.json")
    torch.cuda.set_device(0)
    ctx = m.Context()
    files = [corpus.file_bytes(i) for i in range(12)]
    out = []
    for B in (65536, 4096):
        d_dig = None
        for name, fmt in m.FORMATS.items():
            store = Container(ctx, fmt, B, files)
            if d_dig is None:                                  # the column is over the data: one per block size serves every codec
                rec, d_dig = digest_pass(ctx, store, B, reps)
                rec["name"] = "digest"
                print(json.dumps(rec), flush=True)
                out.append(rec)
            r = run(ctx, fmt, B, files, store, d_dig, reps)
            r["name"] = name
            print(json.dumps(r), flush=True)
            out.append(r)
            store.bk.close()
    store = Container(ctx, m.FORMATS["xpress"], 524288, files)     # the 128-compression root
    rec, _ = digest_pass(ctx, store, 524288, reps)
    rec["name"] = "digest"
    print(json.dumps(rec), flush=True)
    out.append(rec)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
