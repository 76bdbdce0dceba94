"""The block transcoder (mscomp_amd_transcoder_transcode) on the bench corpus as one block container: one resource per file (12 files). Legs:
LZNT1 4096 -> 65536 and 65536 -> 4096, each with checksums and without, and one cross-format leg (LZNT1 65536 -> Xpress 65536, with
checksums). groups_max is the group count of the whole container, the choice that never refuses. Reported per leg, HIP events after two
warm-ups, mean of `reps` executions, the calls' own graphs:
  transcode_ms       the transcoder's call
  route_ms           what a caller does today, in the same run: BlockContainer.decompress into a full-size buffer, BlockContainer.compress
                     of a second container at the new format and size, and -- with checksums -- BlockContainer.crc
  tight_ms           the same call from a transcoder whose groups_max is the number of new blocks that were not carried (an upper bound of
                     the worked groups): the inner plans' table passes, which are sized by groups_max and not by the work, shrink with it.
                     Left out where checksums make every group of a split worked
and from `reps` profiled executions (plain launches, an event pair around each launch) the mean time per launch of the call, the three
counts (new blocks carried, source blocks decoded, new blocks encoded), and the move pass beside a plain device copy of the same bytes
(copy_ms). The new container is compared with the second container of the route -- packed bytes, both tables, checksums -- before any
number is printed. Prints one line per leg and writes the list to profiles/transcode_blocks.json (or to `out`).
Usage: python tools/gpu_transcode.py [reps] [out]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ms_compress_amd as m  # noqa: E402
from ms_compress_amd import corpus  # noqa: E402
from gpu_read import event_ms  # noqa: E402
from gpu_splice import Container, z32, z64  # noqa: E402

LZNT1, XPRESS = m.MSCOMP_LZNT1, m.MSCOMP_XPRESS
LEGS = ((LZNT1, 4096, LZNT1, 65536, True), (LZNT1, 4096, LZNT1, 65536, False), (LZNT1, 65536, LZNT1, 4096, True), (LZNT1, 65536, LZNT1, 4096, False),
        (LZNT1, 65536, XPRESS, 65536, True))


def run(ctx, files, leg, reps, made):
    f1, B1, f2, B2, with_crc = leg
    for key in ((f1, B1), (f2, B2)):
        if key not in made:
            made[key] = Container(ctx, key[0], key[1], files)
    src, want = made[(f1, B1)], made[(f2, B2)]
    n, G = src.n, max(B1, B2)
    nbn = sum((x + B2 - 1) // B2 for x in src.lens)
    groups = sum((x + G - 1) // G for x in src.lens)
    tc = m.BlockTranscoder(ctx, f1, B1, f2, B2, n, src.nbt, nbn, groups)
    d_new, d_nfirst, d_noff, d_ncrc, d_st = torch.zeros(src.total + 16, dtype=torch.uint8, device="cuda"), z64(n + 1), z64(nbn + 1), z32(nbn), z32(n)
    crc_in, crc_out = (src.d_crc, d_ncrc) if with_crc else (None, None)

    def transcode():
        tc.transcode(src.d_packed, src.d_first, src.d_boff, src.t_len, d_new, d_nfirst, d_noff, d_st, d_block_crc=crc_in, d_new_block_crc=crc_out,
                     packed_len=src.packed_bytes, new_cap=src.total)
    transcode()
    counts = tc.counts()
    # the bytes first: the route's second container is what a fresh compression writes
    assert not bool(d_st.any())
    assert bool((d_nfirst == want.d_first).all()) and bool((d_noff[: want.nb + 1] == want.d_boff[: want.nb + 1]).all())
    assert bool((d_new[: want.packed_bytes] == want.d_packed[: want.packed_bytes]).all())
    assert not with_crc or bool((d_ncrc[: want.nb] == want.d_crc[: want.nb]).all())
    transcode_ms = event_ms(transcode, reps)
    # what a caller does today
    d_data, d_olen, d_ost = torch.zeros_like(src.d_in), z64(n), z32(n)

    def route():
        src.bk.decompress(src.d_packed, src.d_first, src.d_boff, src.t_len, d_data, src.t_off, src.t_len, d_olen, d_ost, packed_len=src.packed_bytes)
        want.bk.compress(d_data, want.t_off, want.t_len, want.d_packed, want.d_first, want.d_boff, want.d_st, packed_cap=want.total)
        if with_crc:
            want.bk.crc(d_data, want.t_off, want.t_len, want.d_crc, want.d_st)
    route_ms = event_ms(route, reps)
    torch.cuda.synchronize()
    assert not bool(d_ost.any()) and not bool(want.d_st.any()) and bool((d_new[: want.packed_bytes] == want.d_packed[: want.packed_bytes]).all())
    # the launches of the call
    transcode()
    ctx.profile_enable(True)
    for _ in range(reps):
        transcode()
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    stages = {k: round(v[0] / reps, 4) for k, v in sorted(prof.items(), key=lambda kv: -kv[1][0])}
    d_copy = torch.zeros(want.packed_bytes + 16, dtype=torch.uint8, device="cuda")
    copy_ms = event_ms(lambda: d_copy[: want.packed_bytes].copy_(d_new[: want.packed_bytes]), reps)
    tc.close()
    tight, tight_ms = want.nb - counts[0], None
    if tight < groups and not (with_crc and f1 == f2 and B2 < B1):
        tc = m.BlockTranscoder(ctx, f1, B1, f2, B2, n, src.nbt, nbn, tight)
        d_new.zero_()
        transcode()
        assert tc.counts() == counts and not bool(d_st.any()) and bool((d_new[: want.packed_bytes] == want.d_packed[: want.packed_bytes]).all())
        assert bool((d_noff[: want.nb + 1] == want.d_boff[: want.nb + 1]).all())
        tight_ms = round(event_ms(transcode, reps), 3)
        tc.close()
    move = stages.get("bk_move_kernel", 0.0)
    return dict(format=f1, block=B1, new_format=f2, new_block=B2, crc=with_crc, resources=n, rows=src.nb, new_rows=want.nb, groups=groups,
                mb=round(src.total / 1e6, 1), packed_mb=round(src.packed_bytes / 1e6, 1), new_packed_mb=round(want.packed_bytes / 1e6, 1),
                carried=counts[0], decoded=counts[1], encoded=counts[2], carried_share=round(counts[0] / max(1, want.nb), 4),
                transcode_ms=round(transcode_ms, 3), route_ms=round(route_ms, 3), transcode_over_route=round(transcode_ms / route_ms, 4),
                tight_groups=tight, tight_ms=tight_ms, tight_over_route=None if tight_ms is None else round(tight_ms / route_ms, 4),
                move_ms=move, copy_ms=round(copy_ms, 4), move_over_copy=round(move / copy_ms, 3) if copy_ms else None, stages_ms=stages)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "transcode_blocks.json")
    torch.cuda.set_device(0)
    ctx = m.Context()
    files = [corpus.file_bytes(i) for i in range(12)]
    out, made = [], {}
    for leg in LEGS:
        r = run(ctx, files, leg, reps, made)
        print(json.dumps(r), flush=True)
        out.append(r)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
