"""The block match (mscomp_amd_deduper_match) on the bench corpus as block containers: one resource per file (12 files), B = 65536 and 4096,
with checksums. The new version is the base with its resources in another order, one resource with one block inserted at its front, and
4 KiB written into 1 % of the blocks. Reported per format and block size, HIP events after two warm-ups, mean of `reps` executions, the
calls' own graphs:
  match_ms           the match alone
  delta_ms           match, then the splice of the delta lists out of the new container
  both_ms            match and both splices: the delta container, then store + delta put together again
  diff_share         what blocks_diff makes of the same pair (every new resource against the base resource it came from): its delta
                     container's share of the new container, beside delta_share, the match's
  decode_ms          BlockContainer.decompress of both containers: the floor of any method that decodes
and from `reps` profiled executions of the match (plain launches, an event pair around each stage) the mean time per stage -- clear, seed,
rule 3, keys, confirm, settle, runs, counts -- and the confirm pass beside a plain device copy of the bytes it reads (copy_ms: the stored
bytes of the found and shared blocks, once per side). The results are checked first: the counts against a dictionary of the data blocks on
the host (fresh = written blocks + 1 wherever the corpus repeats no block), and the rebuilt container against the new one, byte for byte.
Prints one line per case and writes the list to profiles/match_blocks.json (or to `out`).
Usage: python tools/gpu_match.py [reps] [out]"""
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

ORDER = (7, 2, 11, 0, 5, 9, 1, 10, 3, 8, 6, 4)                   # new resource q holds base resource ORDER[q]
INSERTED = 4                                                    # the new resource that gets a block at its front
STAGES = ("dd_clear_kernel", "mt_seed_kernel", "dd_rows_kernel", "mt_keys_kernel", "mt_confirm_kernel", "mt_settle_kernel", "mt_runs", "mt_counts_kernel")


def next_version(files, B):
    """(the new files, the number of blocks written into)"""
    rs = np.random.RandomState(7)
    new = [np.array(files[k], dtype=np.uint8, copy=True) for k in ORDER]
    blocks = [(q, k) for q, f in enumerate(new) for k in range(len(f) // B)]               # the whole blocks
    hit = sorted(blocks[i] for i in rs.choice(len(blocks), max(1, len(blocks) // 100), replace=False))
    at = min(100, B - 4096)
    for q, k in hit:
        new[q][k * B + at: k * B + at + 4096] = np.frombuffer(rs.bytes(4096), dtype=np.uint8)
    new[INSERTED] = np.concatenate([np.frombuffer(rs.bytes(B), dtype=np.uint8), new[INSERTED]])
    return new, len(hit)


def host_counts(files, new, B):
    """(found, shared, fresh, blocks of the base that repeat an earlier one) by a dictionary of the data blocks"""
    cut = lambda f: (f[at: at + B].tobytes() for at in range(0, len(f), B))
    store, repeats = set(), 0
    for f in files:
        for b in cut(f):
            repeats += b in store
            store.add(b)
    found = shared = fresh = 0
    seen = set()
    for f in new:
        for b in cut(f):
            if b in store:
                found += 1
            elif b in seen:
                shared += 1
            else:
                fresh += 1
                seen.add(b)
    return found, shared, fresh, repeats


def run(ctx, fmt, B, files, reps):
    n = len(files)
    new_files, written = next_version(files, B)
    old, new = Container(ctx, fmt, B, files), Container(ctx, fmt, B, new_files)
    rows, n_all, total = new.nbt, 2 * n, old.nbt + new.nbt
    dd = m.BlockDeduper.for_match(ctx, B, 1, n_all, total, rows)
    d_df, d_de, d_pf, d_pe, d_cl, d_cnt, d_st = z64(n + 1), z64(4 * rows), z64(n + 1), z64(4 * rows), z64(3 * n), z64(6), z32(n_all)
    match = lambda: dd.match([old.view], new.view, d_df, d_de, d_pf, d_pe, d_cl, d_cnt, d_st)
    match_ms = event_ms(match, reps)
    torch.cuda.synchronize()
    count = [int(x) for x in d_cnt.cpu().tolist()]
    found, shared, fresh, repeats = host_counts(files, new_files, B)
    assert count[:4] == [found, shared, fresh, new.nb] and not bool(d_st.any()), (count, found, shared, fresh, new.nb)
    assert repeats or (fresh == written + 1 and shared == 0), (fresh, written, shared, repeats)
    match()                                                        # (a plain execution first: the profiled ones start warm)
    ctx.profile_enable(True)
    for _ in range(reps):
        match()
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    assert all(prof[k][1] == reps for k in STAGES)
    stage = {k: prof[k][0] / reps for k in STAGES}
    same = new.packed_bytes - count[4]                             # the stored bytes of the found and shared blocks: what confirm reads, on both sides
    d_copy = torch.zeros(2 * same + 16, dtype=torch.uint8, device="cuda")

    def copy():
        d_copy[:same].copy_(old.d_packed[:same])
        d_copy[same: 2 * same].copy_(new.d_packed[:same])
    copy_ms = event_ms(copy, reps)
    # the delta container, and store + delta
    cap_d, cap_n = count[4] + 16, new.packed_bytes + 16
    s1, s2 = m.BlockSplicer.for_extents(ctx, B, 1, n, rows, rows), m.BlockSplicer.for_extents(ctx, B, 2, n, rows, rows)
    D = (torch.zeros(cap_d, dtype=torch.uint8, device="cuda"), z64(n + 1), z64(rows + 1), z64(n), z32(rows), z32(n))
    N = (torch.zeros(cap_n, dtype=torch.uint8, device="cuda"), z64(n + 1), z64(rows + 1), z64(n), z32(rows), z32(n))
    d_view = (D[0], D[1], D[2], D[3], D[4], cap_d, n, rows)

    def delta():
        match()
        s1.splice_extents([new.view], d_df, d_de, D[0], D[1], D[2], D[3], D[5], d_new_block_crc=D[4], new_cap=cap_d)

    def both():
        delta()
        s2.splice_extents([old.view, d_view], d_pf, d_pe, N[0], N[1], N[2], N[3], N[5], d_new_block_crc=N[4], new_cap=cap_n)
    delta_ms = event_ms(delta, reps)
    both_ms = event_ms(both, reps)
    torch.cuda.synchronize()
    assert not bool(D[5].any()) and not bool(N[5].any()) and int(D[2].cpu().numpy()[int(D[1].cpu().numpy()[n])]) == count[4]
    assert bool((N[1] == new.d_first).all()) and bool((N[2][: new.nb + 1] == new.d_boff[: new.nb + 1]).all()) and bool((N[4][: new.nb] == new.d_crc[: new.nb]).all())
    assert bool((N[3] == new.t_len).all()) and bool((N[0][: new.packed_bytes] == new.d_packed[: new.packed_bytes]).all())
    # what diff makes of the same pair: every new resource against the base resource it came from
    df = m.BlockDeduper.for_diff(ctx, B, n, rows)
    d_pair = tab(np.array([(ORDER[q], q) for q in range(n)], dtype=np.uint64).reshape(-1))
    f_cnt, f_st = z64(4), z32(n)
    diff = lambda: df.diff(old.view, new.view, d_pair, z64(n + 1), z64(4 * rows), z64(n + 1), z64(4 * rows), z64(n), f_cnt, f_st)
    diff()
    torch.cuda.synchronize()
    diff_count = [int(x) for x in f_cnt.cpu().tolist()]
    assert not bool(f_st.any()) and diff_count[1] == new.nb
    # the floor of any method that decodes: both containers decompressed
    outs = [(torch.zeros_like(c.d_in), z64(n), z32(n)) for c in (old, new)]

    def decode():
        for c, (d_out, d_olen, d_dst) in zip((old, new), outs):
            c.bk.decompress(c.d_packed, c.d_first, c.d_boff, c.t_len, d_out, c.t_off, c.t_len, d_olen, d_dst, packed_len=c.packed_bytes)
    decode_ms = event_ms(decode, reps)
    torch.cuda.synchronize()
    assert not bool(outs[0][2].any()) and not bool(outs[1][2].any())
    for h in (s1, s2, dd, df, old.bk, new.bk):
        h.close()
    r = dict(format=fmt, block=B, resources=n, rows=new.nb, store_rows=old.nb, mb=round(new.total / 1e6, 1), packed_mb=round(new.packed_bytes / 1e6, 1), written=written,
             repeats=repeats, count=count, delta_share=round(count[4] / new.packed_bytes, 5), diff_changed=diff_count[0],
             diff_share=round(diff_count[2] / new.packed_bytes, 5), match_ms=round(match_ms, 4), delta_ms=round(delta_ms, 4), both_ms=round(both_ms, 4),
             decode_ms=round(decode_ms, 3), match_over_decode=round(match_ms / decode_ms, 4), both_over_decode=round(both_ms / decode_ms, 4))
    for k in STAGES:
        r[k.replace("_kernel", "") + "_ms"] = round(stage[k], 4)
    r.update(confirm_read_gbs=round(2 * same / stage["mt_confirm_kernel"] / 1e6, 1), copy_ms=round(copy_ms, 4), copy_gbs=round(2 * same / copy_ms / 1e6, 1),
             confirm_over_copy=round(stage["mt_confirm_kernel"] / copy_ms, 3))
    return r


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "match_blocks.json")
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
