"""The writer's resize (mscomp_amd_writer_resize) and mscomp_amd_res_crc_dev on the bench corpus as a block container: one resource per file
(12 files), B = 65536. Reported per format, HIP events after two warm-ups, mean of `reps` executions, the calls' own graphs:
  a_ms / a_full_ms      1 % of the resources (at least one) cut at mid-block and another 1 % extended by three blocks, with checksums,
                        against what it replaces in the same run: decode everything, then BlockContainer.compress + .crc of the resized data
  rcrc_ms / rcrc_full_ms  mscomp_amd_res_crc_dev over the new tables against BlockContainer.crc over the decoded data
and from one profiled execution (plain launches) the time per stage -- tables (rules, units, fold), fill, layout, move, crc (both CRC
passes), codec (everything the two inner plans launched) -- and the move pass's bytes per second beside a plain device copy of the packed
buffer (copy_ms, copy_gbs). Every result is compared with the full re-compress: packed bytes, the three tables, the resource checksums.
Prints one line per format and a JSON list at the end.
Usage: python tools/gpu_resize.py [reps]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ms_compress_amd as m  # noqa: E402
from ms_compress_amd import corpus  # noqa: E402
from gpu_read import event_ms, tab  # noqa: E402

B, GROW = 65536, 3
CRC = ("crc_tables_kernel", "crc_seed_kernel", "crc_kernel")
OWN = {"tables": ("rs_units", "rs_fold_kernel"), "fill": ("rs_fill",), "layout": ("rs_layout_kernel",), "move": ("bk_move_kernel",), "crc": CRC}


def run(ctx, fmt, files, reps):
    n = len(files)
    lens = [len(f) for f in files]
    k = max(1, n // 100)
    want = list(lens)
    for r in range(k):                                         # the largest resources are cut, the next ones grow
        order = np.argsort(lens)[::-1]
        cut, ext = int(order[r]), int(order[k + r])
        want[cut] = lens[cut] // 2 // B * B + B // 2
        want[ext] = lens[ext] + GROW * B
    room = max(sum(lens), sum(want))
    z64 = lambda c: torch.zeros(max(1, c), dtype=torch.int64, device="cuda")
    z32 = lambda c: torch.zeros(max(1, c), dtype=torch.int32, device="cuda")
    zu8 = lambda: torch.zeros(room + 16, dtype=torch.uint8, device="cuda")
    bk = m.BlockContainer(ctx, fmt, B, n, room)
    nbt = bk.n_blocks_max
    off, span = m.pack_offsets([max(a, b) for a, b in zip(lens, want)])
    blob = np.zeros(span + 16, dtype=np.uint8)
    for o, f in zip(off, files):
        blob[int(o): int(o) + len(f)] = f
    d_in, t_off, t_len, t_want = torch.from_numpy(blob).cuda(), tab(off), tab(lens), tab(want)
    d_packed, d_first, d_boff, d_st, d_crc = zu8(), z64(n + 1), z64(nbt + 1), z32(n), z32(nbt)
    bk.compress(d_in, t_off, t_len, d_packed, d_first, d_boff, d_st, packed_cap=room)
    bk.crc(d_in, t_off, t_len, d_crc, d_st)
    torch.cuda.synchronize()
    assert not bool(d_st.any())
    nb = int(d_first.cpu().numpy()[n])
    packed_bytes = int(d_boff.cpu().numpy()[nb])
    d_copy = torch.zeros_like(d_packed)
    copy_ms = event_ms(lambda: d_copy[:packed_bytes].copy_(d_packed[:packed_bytes]), reps)
    # (a) the resize
    blocks = lambda x: (x + B - 1) // B
    budget = sum((1 if min(a, b) % B else 0) + max(0, blocks(b) - blocks(a)) for a, b in zip(lens, want) if a != b)
    wr = m.BlockWriter(ctx, fmt, B, n, nbt, 0, budget)
    d_new, d_nfirst, d_noff, d_ncrc, d_nlen, d_rst = zu8(), z64(n + 1), z64(nbt + 1), z32(nbt), z64(n), z32(n)

    def resize():
        wr.resize(d_packed, d_first, d_boff, t_len, t_want, d_new, d_nfirst, d_noff, d_nlen, d_rst, d_block_crc=d_crc, d_new_block_crc=d_ncrc,
                  packed_len=packed_bytes, new_cap=room)
    a_ms = event_ms(resize, reps)
    counts = wr.counts()
    assert not bool(d_rst.any()) and [int(x) for x in d_nlen.cpu().numpy()] == want
    ctx.profile_enable(True)
    resize()
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    stages = {key: sum(prof.get(x, (0.0, 0))[0] for x in names) for key, names in OWN.items()}
    named = {x for names in OWN.values() for x in names}
    stages["codec"] = sum(v[0] for key, v in prof.items() if key not in named)
    stages = {key: round(v, 4) for key, v in stages.items()}
    # what it replaces: decode all, resize on the caller's side (cut by the length table, zeros behind the old end), compress + crc
    d_out, d_olen, d_p2, d_f2, d_b2, d_c2, d_r2 = torch.zeros_like(d_in), z64(n), zu8(), z64(n + 1), z64(nbt + 1), z32(nbt), z32(n)

    def full():
        bk.decompress(d_packed, d_first, d_boff, t_len, d_out, t_off, t_len, d_olen, d_st, packed_len=packed_bytes)
        bk.compress(d_out, t_off, t_want, d_p2, d_f2, d_b2, d_st, packed_cap=room)
        bk.crc(d_out, t_off, t_want, d_c2, d_st, d_res_crc=d_r2)
    a_full = event_ms(full, reps)                              # (the layout leaves room behind every resource that grows: d_out is zero there)
    torch.cuda.synchronize()
    nb2 = int(d_f2.cpu().numpy()[n])
    new_bytes = int(d_b2.cpu().numpy()[nb2])
    assert not bool(d_st.any()) and bool((d_nfirst == d_f2).all()) and bool((d_noff == d_b2).all()) and bool((d_ncrc == d_c2).all())
    assert bool((d_new[:new_bytes] == d_p2[:new_bytes]).all())
    # (b) the resource checksums from the new block checksums
    d_rcrc, d_rst2 = z32(n), z32(n)
    rcrc_ms = event_ms(lambda: m.res_crc_dev(ctx, B, n, nbt, d_nfirst, d_nlen, d_ncrc, d_rcrc, d_rst2), reps)
    rcrc_full = event_ms(lambda: bk.crc(d_out, t_off, t_want, d_c2, d_st, d_res_crc=d_r2), reps)
    torch.cuda.synchronize()
    assert not bool(d_rst2.any()) and bool((d_rcrc == d_r2).all())
    wr.close()
    bk.close()
    return dict(format=fmt, block=B, resources=n, blocks=nb, new_blocks=nb2, mb=round(sum(lens) / 1e6, 1), packed_mb=round(packed_bytes / 1e6, 1),
                copy_ms=round(copy_ms, 4), copy_gbs=round(packed_bytes / copy_ms / 1e6, 1), a_ms=round(a_ms, 3), a_full_ms=round(a_full, 3),
                a_ratio=round(a_ms / a_full, 3), a_counts=counts, a_stages=stages,
                a_move_gbs=round(new_bytes / stages["move"] / 1e6, 1) if stages["move"] else None,
                rcrc_ms=round(rcrc_ms, 4), rcrc_full_ms=round(rcrc_full, 3))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    torch.cuda.set_device(0)
    ctx = m.Context()
    files = [corpus.file_bytes(i) for i in range(12)]
    out = []
    for name, fmt in m.FORMATS.items():
        r = run(ctx, fmt, files, reps)
        r["name"] = name
        print(json.dumps(r), flush=True)
        out.append(r)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
