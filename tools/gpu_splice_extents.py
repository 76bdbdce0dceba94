"""Splice by block extents (mscomp_amd_splicer_splice_extents) on the bench corpus as block containers: one resource per file (12 files),
B = 65536 and 4096. Reported per format and block size, HIP events after two warm-ups, mean of `reps` executions, the call's own graph:
  a_ms / a_full_ms   all 12 resources joined into one, every resource but the last cut down to whole blocks, with checksums, against what
                     it replaces in the same run: BlockContainer.decompress of those block ranges back to back, then .compress + .crc
  b_ext_ms / b_pick_ms   the identity extent list (one extent per resource, through its last block) against mscomp_amd_splicer_splice of
                     the identity pick list, by turns in the same run
and from one profiled execution of each call of (b) (plain launches) the time per launch: the extent pass, the three tiled row passes and
the move beside sp_layout_kernel and its move on the same table. Every result is compared with a full compress + crc of the data it
stands for: packed bytes, the three tables. Prints one line per case and writes the list to profiles/splice_extents.json (or to `out`).
Usage: python tools/gpu_splice_extents.py [reps] [out]"""
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

END = (1 << 64) - 1
EXT_LAUNCHES = ("sx_extent_kernel", "sx_tile_kernel", "sx_tilescan_kernel", "sx_rows_kernel", "bk_move_kernel")
PICK_LAUNCHES = ("sp_layout_kernel", "bk_move_kernel")


def profiled(ctx, call, names):
    ctx.profile_enable(True)
    call()
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    return {k: round(prof[k][0], 4) for k in names}


def run(ctx, fmt, B, files, reps):
    n = len(files)
    whole = Container(ctx, fmt, B, files)
    # (a) all resources joined into one, all but the last cut down to whole blocks
    cut = [len(f) // B * B for f in files[:-1]] + [len(files[-1])]
    joined = np.concatenate([f[:c] for f, c in zip(files, cut)])
    want = Container(ctx, fmt, B, [joined])                     # (what the result must be, and the container object of the full path)
    ext = [(0, r, 0, c // B) for r, c in enumerate(cut[:-1])] + [(0, n - 1, 0, END)]
    sp = m.BlockSplicer.for_extents(ctx, B, 1, 1, n, want.nbt)
    d_ef, d_ext = tab([0, n]), tab(np.array(ext, dtype=np.uint64).reshape(-1))
    d_new, d_nfirst, d_noff, d_ncrc, d_nlen, d_st = torch.zeros_like(want.d_packed), z64(2), z64(want.nbt + 1), z32(want.nbt), z64(1), z32(1)

    def join():
        sp.splice_extents([whole.view], d_ef, d_ext, d_new, d_nfirst, d_noff, d_nlen, d_st, d_new_block_crc=d_ncrc, new_cap=want.total)
    a_ms = event_ms(join, reps)
    torch.cuda.synchronize()
    assert not bool(d_st.any()) and int(d_nlen[0]) == want.total and want.same(d_new, d_nfirst, d_noff, d_ncrc)
    a_launch = profiled(ctx, join, EXT_LAUNCHES)
    # what it replaces: decode the kept block ranges back to back, compress + crc of the result as one resource
    ranges = np.array([(0, c // B) for c in cut[:-1]] + [(0, 1 << 40)], dtype=np.uint64).reshape(-1)
    d_range, d_out, d_olen, d_dst = tab(ranges), torch.zeros(want.total + 64, dtype=torch.uint8, device="cuda"), z64(n), z32(n)
    t_ooff, t_ocap, t_zero = tab(np.concatenate([[0], np.cumsum(cut[:-1])])), tab(cut), tab([0])
    d_p2, d_f2, d_b2, d_c2, d_s2 = torch.zeros_like(want.d_packed), z64(2), z64(want.nbt + 1), z32(want.nbt), z32(1)

    def full():
        whole.bk.decompress(whole.d_packed, whole.d_first, whole.d_boff, whole.t_len, d_out, t_ooff, t_ocap, d_olen, d_dst, d_range=d_range,
                            packed_len=whole.packed_bytes)
        want.bk.compress(d_out, t_zero, want.t_len, d_p2, d_f2, d_b2, d_s2, packed_cap=want.total)
        want.bk.crc(d_out, t_zero, want.t_len, d_c2, d_s2)
    a_full = event_ms(full, reps)
    torch.cuda.synchronize()
    assert not bool(d_dst.any()) and not bool(d_s2.any()) and want.same(d_p2, d_f2, d_b2, d_c2)
    sp.close()
    # (b) the identity: extents against picks, by turns
    sx = m.BlockSplicer.for_extents(ctx, B, 1, n, n, whole.nbt)
    sk = m.BlockSplicer(ctx, B, 1, n, whole.nbt)
    d_ef, d_ext = tab(np.arange(n + 1)), tab(np.array([(0, r, 0, END) for r in range(n)], dtype=np.uint64).reshape(-1))
    d_pick = tab(np.array([(0, r) for r in range(n)], dtype=np.uint64).reshape(-1))
    outs = [(torch.zeros_like(whole.d_packed), z64(n + 1), z64(whole.nbt + 1), z32(whole.nbt), z64(n), z32(n)) for _ in range(2)]

    def by_extents():
        d_new, d_nfirst, d_noff, d_ncrc, d_nlen, d_st = outs[0]
        sx.splice_extents([whole.view], d_ef, d_ext, d_new, d_nfirst, d_noff, d_nlen, d_st, d_new_block_crc=d_ncrc, new_cap=whole.total)

    def by_picks():
        d_new, d_nfirst, d_noff, d_ncrc, d_nlen, d_st = outs[1]
        sk.splice([whole.view], d_pick, d_new, d_nfirst, d_noff, d_nlen, d_st, d_new_block_crc=d_ncrc, new_cap=whole.total)
    turns = {"ext": [], "pick": []}
    for _ in range(2):
        turns["ext"].append(event_ms(by_extents, reps))
        turns["pick"].append(event_ms(by_picks, reps))
    torch.cuda.synchronize()
    for d_new, d_nfirst, d_noff, d_ncrc, d_nlen, d_st in outs:
        assert not bool(d_st.any()) and whole.same(d_new, d_nfirst, d_noff, d_ncrc) and [int(x) for x in d_nlen.cpu()] == whole.lens
    b_ext, b_pick = profiled(ctx, by_extents, EXT_LAUNCHES), profiled(ctx, by_picks, PICK_LAUNCHES)
    sx.close(); sk.close()
    layout_ext = sum(b_ext[k] for k in EXT_LAUNCHES[:4])
    res = dict(format=fmt, block=B, resources=n, rows=whole.nb, mb=round(whole.total / 1e6, 1), packed_mb=round(whole.packed_bytes / 1e6, 1),
               a_rows=want.nb, a_packed_mb=round(want.packed_bytes / 1e6, 1), a_ms=round(a_ms, 4), a_full_ms=round(a_full, 3), a_ratio=round(a_ms / a_full, 4),
               a_launch_ms=a_launch, b_ext_ms=[round(x, 4) for x in turns["ext"]], b_pick_ms=[round(x, 4) for x in turns["pick"]],
               b_ext_launch_ms=b_ext, b_pick_launch_ms=b_pick, b_layout_ext_ms=round(layout_ext, 4), b_layout_pick_ms=b_pick["sp_layout_kernel"])
    for c in (whole, want):
        c.bk.close()
    return res


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "splice_extents.json")
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
