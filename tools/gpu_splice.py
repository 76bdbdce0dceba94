"""The block splicer (mscomp_amd_splicer_splice) on the bench corpus as block containers: one resource per file (12 files), B = 65536 and 4096.
Reported per format and block size, HIP events after two warm-ups, mean of `reps` executions, the call's own graph:
  a_ms / a_full_ms   drop the largest resource, with checksums, against what it replaces in the same run: BlockContainer.decompress of the
                     rest, then .compress + .crc of it
  b_ms               merge two containers of 6 resources each, picks by turns from one and the other
and from one profiled execution of (a) (plain launches) the time per launch -- layout, move -- and the move's bytes per second beside a
plain device copy of the same number of packed bytes (copy_ms, copy_gbs). Both results are compared with a full compress + crc of the picked
data: packed bytes, the three tables. Prints one line per case and writes the list to profiles/splice_blocks.json (or to `out`).
Usage: python tools/gpu_splice.py [reps] [out]"""
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

z64 = lambda c: torch.zeros(max(1, c), dtype=torch.int64, device="cuda")
z32 = lambda c: torch.zeros(max(1, c), dtype=torch.int32, device="cuda")


class Container:
    """files compressed and checksummed as one block container; the tensors a splice or a decode reads"""

    def __init__(self, ctx, fmt, B, files):
        self.n, self.lens = len(files), [len(f) for f in files]
        self.total = sum(self.lens)
        self.bk = m.BlockContainer(ctx, fmt, B, self.n, self.total)
        self.nbt = self.bk.n_blocks_max
        self.off, _ = m.pack_offsets(self.lens)
        blob = np.zeros(self.total + 16 * self.n + 16, dtype=np.uint8)
        for o, f in zip(self.off, files):
            blob[int(o): int(o) + len(f)] = f
        self.d_in, self.t_off, self.t_len = torch.from_numpy(blob).cuda(), tab(self.off), tab(self.lens)
        self.d_packed = torch.zeros(self.total + 16, dtype=torch.uint8, device="cuda")
        self.d_first, self.d_boff, self.d_st, self.d_crc = z64(self.n + 1), z64(self.nbt + 1), z32(self.n), z32(self.nbt)
        self.bk.compress(self.d_in, self.t_off, self.t_len, self.d_packed, self.d_first, self.d_boff, self.d_st, packed_cap=self.total)
        self.bk.crc(self.d_in, self.t_off, self.t_len, self.d_crc, self.d_st)
        torch.cuda.synchronize()
        assert not bool(self.d_st.any())
        self.nb = int(self.d_first.cpu().numpy()[self.n])
        self.packed_bytes = int(self.d_boff.cpu().numpy()[self.nb])
        self.view = (self.d_packed, self.d_first, self.d_boff, self.t_len, self.d_crc, self.packed_bytes, self.n, self.nbt)

    def same(self, d_new, d_nfirst, d_noff, d_ncrc):
        return (bool((d_nfirst == self.d_first).all()) and bool((d_noff == self.d_boff).all()) and bool((d_ncrc == self.d_crc).all())
                and bool((d_new[: self.packed_bytes] == self.d_packed[: self.packed_bytes]).all()))


def run(ctx, fmt, B, files, reps):
    n = len(files)
    whole = Container(ctx, fmt, B, files)
    # (a) drop the largest resource
    drop = int(np.argmax(whole.lens))
    rest = [r for r in range(n) if r != drop]
    want = Container(ctx, fmt, B, [files[r] for r in rest])    # (what the result must be, and the container object of the full path)
    sp = m.BlockSplicer(ctx, B, 1, n - 1, want.nbt)
    d_pick = tab(np.array([(0, r) for r in rest], dtype=np.uint64).reshape(-1))
    d_new, d_nfirst, d_noff, d_ncrc, d_nlen, d_st = torch.zeros_like(want.d_packed), z64(n), z64(want.nbt + 1), z32(want.nbt), z64(n - 1), z32(n - 1)

    def splice():
        sp.splice([whole.view], d_pick, d_new, d_nfirst, d_noff, d_nlen, d_st, d_new_block_crc=d_ncrc, new_cap=want.total)
    a_ms = event_ms(splice, reps)
    torch.cuda.synchronize()
    assert not bool(d_st.any()) and want.same(d_new, d_nfirst, d_noff, d_ncrc)
    ctx.profile_enable(True)
    splice()
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    layout_ms, move_ms = prof["sp_layout_kernel"][0], prof["bk_move_kernel"][0]
    d_copy = torch.zeros_like(d_new)
    copy_ms = event_ms(lambda: d_copy[: want.packed_bytes].copy_(d_new[: want.packed_bytes]), reps)
    # what it replaces: decode the rest (the dropped resource's range is empty), compress + crc of it
    ranges = np.array([(0, 0 if r == drop else 1 << 40) for r in range(n)], dtype=np.uint64).reshape(-1)
    d_range, d_out, d_olen, d_dst = tab(ranges), torch.zeros_like(whole.d_in), z64(n), z32(n)
    t_roff = tab([whole.off[r] for r in rest])
    d_p2, d_f2, d_b2, d_c2, d_s2 = torch.zeros_like(want.d_packed), z64(n), z64(want.nbt + 1), z32(want.nbt), z32(n - 1)

    def full():
        whole.bk.decompress(whole.d_packed, whole.d_first, whole.d_boff, whole.t_len, d_out, whole.t_off, whole.t_len, d_olen, d_dst, d_range=d_range,
                            packed_len=whole.packed_bytes)
        want.bk.compress(d_out, t_roff, want.t_len, d_p2, d_f2, d_b2, d_s2, packed_cap=want.total)
        want.bk.crc(d_out, t_roff, want.t_len, d_c2, d_s2)
    a_full = event_ms(full, reps)
    torch.cuda.synchronize()
    assert not bool(d_dst.any()) and not bool(d_s2.any()) and want.same(d_p2, d_f2, d_b2, d_c2)
    sp.close()
    # (b) two containers of 6 resources each, merged by turns
    half = n // 2
    one, two = Container(ctx, fmt, B, files[:half]), Container(ctx, fmt, B, files[half: 2 * half])
    picks = [(k % 2, k // 2) for k in range(2 * half)]
    both = Container(ctx, fmt, B, [files[r + half * s] for s, r in picks])
    sp = m.BlockSplicer(ctx, B, 2, 2 * half, both.nbt)
    d_pick = tab(np.array(picks, dtype=np.uint64).reshape(-1))
    d_new, d_nfirst, d_noff, d_ncrc, d_nlen, d_st = torch.zeros_like(both.d_packed), z64(2 * half + 1), z64(both.nbt + 1), z32(both.nbt), z64(2 * half), z32(2 * half)
    b_ms = event_ms(lambda: sp.splice([one.view, two.view], d_pick, d_new, d_nfirst, d_noff, d_nlen, d_st, d_new_block_crc=d_ncrc, new_cap=both.total), reps)
    torch.cuda.synchronize()
    assert not bool(d_st.any()) and both.same(d_new, d_nfirst, d_noff, d_ncrc)
    sp.close()
    res = dict(format=fmt, block=B, resources=n, rows=whole.nb, mb=round(whole.total / 1e6, 1), packed_mb=round(whole.packed_bytes / 1e6, 1),
               a_rows=want.nb, a_packed_mb=round(want.packed_bytes / 1e6, 1), a_ms=round(a_ms, 4), a_full_ms=round(a_full, 3), a_ratio=round(a_ms / a_full, 4),
               layout_ms=round(layout_ms, 4), move_ms=round(move_ms, 4), layout_share=round(layout_ms / (layout_ms + move_ms), 3),
               move_gbs=round(want.packed_bytes / move_ms / 1e6, 1), copy_ms=round(copy_ms, 4), copy_gbs=round(want.packed_bytes / copy_ms / 1e6, 1),
               b_rows=both.nb, b_packed_mb=round(both.packed_bytes / 1e6, 1), b_ms=round(b_ms, 4))
    for c in (whole, want, one, two, both):
        c.bk.close()
    return res


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "splice_blocks.json")
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
