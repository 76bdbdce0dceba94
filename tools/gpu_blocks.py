"""Block containers (mscomp_amd_blocks_*) against what the library could do before them on the same block list: the bench corpus, one
resource per file (12 files, 3 239 x 64 KiB), at the block sizes given.
Reported per (format, block size), HIP events after a warm-up, mean of `reps` executions:
  bk_c_ms     BlockContainer.compress
  comp_c_ms   a compress dev plan over the same blocks with host-built block tables (capacities of plan_layout_dev) followed by
              mscomp_amd_compact_dev -- no raw fallback: a block that does not shrink stays longer than its data
  bk_d_ms     BlockContainer.decompress of every block
  plan_d_ms   a decompress dev plan over the blocks the container stored compressed (the raw ones left out)
  bk_d1_ms    BlockContainer.decompress of a range of 1 % of each resource's blocks (at least one)
  raw         blocks stored raw / blocks
The container's bytes are checked by a whole decode against the input. Prints one line per case and a JSON list at the end.
Usage: python tools/gpu_blocks.py [reps] [block sizes, comma separated; default 32768,65536]"""
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
    M = bk.n_blocks_max
    t_off, t_len = tab(off), tab(lens)
    d_packed, d_first, d_boff, d_st = torch.zeros(total + 16, dtype=torch.uint8, device="cuda"), z64(n + 1), z64(M + 1), z32(n)
    bk_c = event_ms(lambda: bk.compress(d_in, t_off, t_len, d_packed, d_first, d_boff, d_st, packed_cap=total), reps)
    assert not bool(d_st.any())
    first, boff = d_first.cpu().numpy(), d_boff.cpu().numpy()
    nb = int(first[n])
    # the same blocks as units of a compress dev plan + compaction (what the library offered before)
    b_off = np.concatenate([int(o) + np.arange(0, ln, B, dtype=np.uint64) for o, ln in zip(off, lens)])
    b_len = np.concatenate([np.minimum(B, ln - np.arange(0, ln, B)).astype(np.uint64) for ln in lens])
    assert len(b_off) == nb
    tb_off, tb_len = tab(b_off), tab(b_len)
    cp = m.CompressDevPlan(ctx, fmt, nb, total, B)
    s_off, s_cap = m.plan_layout_dev(ctx, fmt, tb_len, align=16)
    torch.cuda.synchronize()
    d_stage = torch.zeros(int(s_off[nb]) + 16, dtype=torch.uint8, device="cuda")
    d_clen, d_cst, d_pk2, d_po2 = z64(nb), z32(nb), torch.zeros(int(s_off[nb]) + 16, dtype=torch.uint8, device="cuda"), z64(nb + 1)

    def composition():
        cp.execute(d_in, tb_off, tb_len, d_stage, s_off, s_cap, d_clen, d_cst)
        m.compact_dev(ctx, d_stage, s_off, d_clen, 1, d_pk2, d_po2)
    comp_c = event_ms(composition, reps)
    assert not bool(d_cst.any())
    # decode: the whole container, 1 % of it, and a decompress dev plan over the compressed blocks alone
    d_out, d_olen, d_dst = torch.zeros(total + 16, dtype=torch.uint8, device="cuda"), z64(n), z32(n)
    bk_d = event_ms(lambda: bk.decompress(d_packed, d_first, d_boff, t_len, d_out, t_off, t_len, d_olen, d_dst, packed_len=total), reps)
    assert not bool(d_dst.any()) and bool((d_out == d_in).all())
    cnt = np.diff(first)
    rng = np.stack([cnt // 2, np.maximum(1, cnt // 100)], axis=1).astype(np.uint64)
    t_rng = tab(rng.reshape(-1))
    bk_d1 = event_ms(lambda: bk.decompress(d_packed, d_first, d_boff, t_len, d_out, t_off, t_len, d_olen, d_dst, d_range=t_rng, packed_len=total), reps)
    assert not bool(d_dst.any())
    slen = np.diff(boff[: nb + 1]).astype(np.uint64)
    is_c = slen < b_len
    k = int(is_c.sum())
    dp = m.DevPlan(ctx, fmt, max(1, k), total, total)
    u_in, u_len, u_out, u_cap = tab(boff[:nb][is_c]), tab(slen[is_c]), tab(b_off[is_c]), tab(b_len[is_c])
    d_o2, d_l2, d_s2 = torch.zeros(total + 16, dtype=torch.uint8, device="cuda"), z64(k), z32(k)
    plan_d = event_ms(lambda: dp.execute(d_packed, u_in, u_len, d_o2, u_out, u_cap, d_l2, d_s2), reps) if k else 0.0
    assert not bool(d_s2.any())
    for p in (bk, cp, dp):
        p.close()
    return dict(format=fmt, block=B, resources=n, blocks=nb, raw=int(nb - k), mb=round(total / 1e6, 1), packed_mb=round(int(boff[nb]) / 1e6, 2),
                composition_packed_mb=round(int(d_po2[nb]) / 1e6, 2), bk_c_ms=round(bk_c, 3), comp_c_ms=round(comp_c, 3),
                c_ratio=round(bk_c / comp_c, 3), bk_d_ms=round(bk_d, 3), plan_d_ms=round(plan_d, 3), d_ratio=round(bk_d / plan_d, 3) if k else None,
                bk_d1_ms=round(bk_d1, 3), d1_share=round(bk_d1 / bk_d, 3))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
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
