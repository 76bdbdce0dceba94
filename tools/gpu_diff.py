"""The block diff (mscomp_amd_deduper_diff) on the bench corpus as block containers: one resource per file (12 files), B = 65536 and 32768,
with checksums. The new version is the old one after blocks_write of 4 KiB into 1 % of its blocks and blocks_resize of one resource by
three blocks more. Reported per format and block size, HIP events after two warm-ups, mean of `reps` executions, the calls' own graphs:
  diff_ms            the diff alone
  delta_ms           diff, then the splice of the delta lists out of the new container
  both_ms            diff and both splices: the delta container, then base + delta put together again
  decode_ms          what a caller does today: BlockContainer.decompress of both containers, then the data compared block by block on the
                     device (one flag per block; nothing answers on the host before the end)
and from `reps` profiled executions of the diff (plain launches, an event pair around each stage) the mean time per stage -- seed, verdicts,
confirm, runs, counts -- and the confirm pass beside a plain device copy of the bytes it reads (copy_ms, a mean of `reps` too: the stored
bytes of the unchanged blocks, once per version; the confirm pass reads them and writes none, the copy writes them as well). Both run
largely out of the Infinity Cache at these sizes: not HBM rates. The results are checked: the counts against the blocks that were written
and added, and the rebuilt container against the new one, byte for byte.
Prints one line per case and writes the list to profiles/diff_blocks.json (or to `out`).
Usage: python tools/gpu_diff.py [reps] [out]"""
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

GROWN, STAGES = 3, ("df_seed_kernel", "df_verdict_kernel", "df_confirm_kernel", "df_runs", "df_counts_kernel")


class Version:
    """a container from host arrays (what blocks_write and blocks_resize return), on the device as a view takes it"""

    def __init__(self, packed, first, off, lens, crc):
        self.n, self.lens, self.nbt = len(lens), [int(x) for x in lens], len(off) - 1
        self.packed_bytes = len(packed)
        self.d_packed = torch.zeros(self.packed_bytes + 16, dtype=torch.uint8, device="cuda")
        self.d_packed[: self.packed_bytes] = torch.from_numpy(np.ascontiguousarray(packed)).cuda()
        self.d_first, self.d_boff, self.t_len = tab(first), tab(off), tab(self.lens)
        self.d_crc = torch.from_numpy(np.ascontiguousarray(crc, dtype=np.uint32).view(np.int32).copy()).cuda()
        self.view = (self.d_packed, self.d_first, self.d_boff, self.t_len, self.d_crc, self.packed_bytes, self.n, self.nbt)


def next_version(ctx, fmt, B, old):
    """(Version, the blocks that changed as a set of (resource, block)) of `old` a day later"""
    host = lambda t, k: t.cpu().numpy().view(np.uint64)[:k].copy()
    first, off = host(old.d_first, old.n + 1), host(old.d_boff, old.nb + 1)
    packed, crc = old.d_packed.cpu().numpy()[: old.packed_bytes].copy(), old.d_crc.cpu().numpy().view(np.uint32)[: old.nb].copy()
    rs = np.random.RandomState(7)
    blocks = [(r, k) for r, L in enumerate(old.lens) for k in range(L // B)]             # the whole blocks
    hit = sorted(blocks[i] for i in rs.choice(len(blocks), max(1, len(blocks) // 100), replace=False))
    writes = [(r, k * B + 100, rs.bytes(4096)) for r, k in hit]
    packed, off, crc, _, st, rst = m.blocks_write(fmt, packed, first, off, old.lens, B, writes, ctx=ctx, block_crc=crc)
    assert not any(st) and not any(rst)
    lens = list(old.lens)
    lens[GROWN] += 3 * B
    packed, off, crc, first, lens, rst = m.blocks_resize(fmt, packed, first, off, old.lens, B, lens, ctx=ctx, block_crc=crc)
    assert not any(rst)
    nb_old = (old.lens[GROWN] + B - 1) // B
    grown = {(GROWN, nb_old + i) for i in range(3)} | ({(GROWN, nb_old - 1)} if old.lens[GROWN] % B else set())
    return Version(packed, first, off, lens, crc), set(hit) | grown


def run(ctx, fmt, B, files, reps):
    n = len(files)
    old = Container(ctx, fmt, B, files)
    new, touched = next_version(ctx, fmt, B, old)
    rows = int(new.d_first.cpu().numpy()[n])
    d_pair = tab(np.array([(r, r) for r in range(n)], dtype=np.uint64).reshape(-1))
    dd = m.BlockDeduper.for_diff(ctx, B, n, rows)
    d_df, d_de, d_pf, d_pe, d_ch, d_cnt, d_st = z64(n + 1), z64(4 * rows), z64(n + 1), z64(4 * rows), z64(n), z64(4), z32(n)
    diff = lambda: dd.diff(old.view, new.view, d_pair, d_df, d_de, d_pf, d_pe, d_ch, d_cnt, d_st)
    diff_ms = event_ms(diff, reps)
    torch.cuda.synchronize()
    count = [int(x) for x in d_cnt.cpu().tolist()]
    assert count[0] == len(touched) and count[1] == rows and count[3] == 0 and not bool(d_st.any()), (count, len(touched), rows)
    diff()                                                         # (a plain execution first: the profiled ones start warm)
    ctx.profile_enable(True)
    for _ in range(reps):
        diff()
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    assert all(prof[k][1] == reps for k in STAGES)
    stage = {k: prof[k][0] / reps for k in STAGES}
    same = new.packed_bytes - count[2]                             # the stored bytes of the unchanged blocks: what confirm reads, in both versions
    d_copy = torch.zeros(2 * same + 16, dtype=torch.uint8, device="cuda")

    def copy():
        d_copy[:same].copy_(old.d_packed[:same])
        d_copy[same: 2 * same].copy_(new.d_packed[:same])
    copy_ms = event_ms(copy, reps)
    # the delta container, and base + delta
    cap_d, cap_n = count[2] + 16, new.packed_bytes + 16
    s1, s2 = m.BlockSplicer.for_extents(ctx, B, 1, n, rows, rows), m.BlockSplicer.for_extents(ctx, B, 2, n, rows, rows)
    D = (torch.zeros(cap_d, dtype=torch.uint8, device="cuda"), z64(n + 1), z64(rows + 1), z64(n), z32(rows), z32(n))
    N = (torch.zeros(cap_n, dtype=torch.uint8, device="cuda"), z64(n + 1), z64(rows + 1), z64(n), z32(rows), z32(n))
    d_view = (D[0], D[1], D[2], D[3], D[4], cap_d, n, rows)

    def delta():
        diff()
        s1.splice_extents([new.view], d_df, d_de, D[0], D[1], D[2], D[3], D[5], d_new_block_crc=D[4], new_cap=cap_d)

    def both():
        delta()
        s2.splice_extents([old.view, d_view], d_pf, d_pe, N[0], N[1], N[2], N[3], N[5], d_new_block_crc=N[4], new_cap=cap_n)
    delta_ms = event_ms(delta, reps)
    both_ms = event_ms(both, reps)
    torch.cuda.synchronize()
    assert not bool(D[5].any()) and not bool(N[5].any()) and int(D[2].cpu().numpy()[int(D[1].cpu().numpy()[n])]) == count[2]
    assert bool((N[1] == new.d_first).all()) and bool((N[2][: rows + 1] == new.d_boff[: rows + 1]).all()) and bool((N[4][:rows] == new.d_crc[:rows]).all())
    assert bool((N[3] == new.t_len).all()) and bool((N[0][: new.packed_bytes] == new.d_packed[: new.packed_bytes]).all())
    # what a caller does today: decode both containers, compare the data block by block
    total_new = sum(new.lens)
    bk_new = m.BlockContainer(ctx, fmt, B, n, total_new)
    off_new, _ = m.pack_offsets(new.lens)
    t_off_new = tab(off_new)
    outs = [(torch.zeros_like(old.d_in), z64(n), z32(n)), (torch.zeros(total_new + 16 * n + 16 + B, dtype=torch.uint8, device="cuda"), z64(n), z32(n))]

    def decode_and_compare():
        old.bk.decompress(old.d_packed, old.d_first, old.d_boff, old.t_len, outs[0][0], old.t_off, old.t_len, outs[0][1], outs[0][2], packed_len=old.packed_bytes)
        bk_new.decompress(new.d_packed, new.d_first, new.d_boff, new.t_len, outs[1][0], t_off_new, new.t_len, outs[1][1], outs[1][2], packed_len=new.packed_bytes)
        flags = []
        for r in range(n):
            a0, b0, k = int(old.off[r]), int(off_new[r]), min(old.lens[r], new.lens[r])
            whole = k // B * B
            if whole:
                flags.append((outs[0][0][a0: a0 + whole] != outs[1][0][b0: b0 + whole]).view(-1, B).any(dim=1))
            if k > whole:                                          # the short last block of the shorter one; blocks behind it are new
                flags.append((outs[0][0][a0 + whole: a0 + k] != outs[1][0][b0 + whole: b0 + k]).any().view(1) | torch.tensor([old.lens[r] != new.lens[r]], device="cuda"))
        return torch.cat(flags)
    decode_ms = event_ms(decode_and_compare, reps)
    found = int(decode_and_compare().sum().item()) + 3                                  # (the three blocks behind the old end have nothing to be compared with)
    assert found == count[0], (found, count[0])
    for h in (s1, s2, dd, bk_new, old.bk):
        h.close()
    return dict(format=fmt, block=B, resources=n, rows=rows, mb=round(total_new / 1e6, 1), packed_mb=round(new.packed_bytes / 1e6, 1), count=count,
                delta_share=round(count[2] / new.packed_bytes, 5), diff_ms=round(diff_ms, 4), delta_ms=round(delta_ms, 4), both_ms=round(both_ms, 4),
                decode_ms=round(decode_ms, 3), diff_over_decode=round(diff_ms / decode_ms, 4), both_over_decode=round(both_ms / decode_ms, 4),
                seed_ms=round(stage[STAGES[0]], 4), verdict_ms=round(stage[STAGES[1]], 4), confirm_ms=round(stage[STAGES[2]], 4), runs_ms=round(stage[STAGES[3]], 4),
                counts_ms=round(stage[STAGES[4]], 4), confirm_read_gbs=round(2 * same / stage[STAGES[2]] / 1e6, 1), copy_ms=round(copy_ms, 4),
                copy_gbs=round(2 * same / copy_ms / 1e6, 1), confirm_over_copy=round(stage[STAGES[2]] / copy_ms, 3))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "diff_blocks.json")
    torch.cuda.set_device(0)
    ctx = m.Context()
    files = [corpus.file_bytes(i) for i in range(12)]
    out = []
    for B in (65536, 32768):
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
