"""Match by digest (mscomp_amd_deduper_match_digest) beside match (mscomp_amd_deduper_match) on tools/gpu_match.py's workload: the bench corpus
as block containers, one resource per file (12 files), with checksums; the new version is the base with its resources in another order,
one block inserted at the front of a resource, and 4 KiB written into 1 % of the blocks. Per block size (65536 and 4096):
  (a) the same LZNT1 pair through both calls. The outputs are compared on the device first (all seven, the refuted count apart). Then
      `rounds` alternating rounds of `reps` executions each, HIP events, the calls' own graphs: the mean of a call's rounds and their
      spread (min, max). Then `reps` profiled executions of each (plain launches, an event pair around each stage): time per stage.
  (b) across codecs: next as LZNT1 against the same store as Xpress+Huffman. match_digest takes the two as they are; the route that
      exists today transcodes the store to LZNT1 (BlockTranscoder) and then runs match. Both in alternating rounds; the delta's size
      (d_count[4]) and the classes are checked against the one-format answer of (a): equal.
  (c) the digest pass over next (BlockDigester.blocks over its data), the digester's own call: what a caller without a column pays once.
Prints one line per case and writes the list to profiles/match_digest.json (or to `out`).
Usage: python tools/gpu_match_digest.py [reps] [rounds] [out]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ms_compress_amd as m  # noqa: E402
from ms_compress_amd import corpus  # noqa: E402
from gpu_match import STAGES, host_counts, next_version  # noqa: E402
from gpu_read import event_ms  # noqa: E402
from gpu_splice import Container, z32, z64  # noqa: E402

DIGEST_STAGES = ("dd_clear_kernel", "mt_seed_kernel", "dd_rows_kernel", "md_keys_kernel", "md_confirm_kernel", "md_settle_kernel", "mt_runs", "mt_counts_kernel")
LZNT1, XH = m.MSCOMP_LZNT1, m.MSCOMP_XPRESS_HUFF


def column(ctx, con, B):
    """(the container's digest column, the digester, the call that writes it)"""
    dg = m.BlockDigester(ctx, B, con.n, con.total)
    d_dig, d_st = z32(4 * max(con.nbt, dg.n_blocks_max) + 4), z32(con.n)
    call = lambda: dg.blocks(con.d_in, con.t_off, con.t_len, d_dig, d_st)
    call()
    torch.cuda.synchronize()
    assert not bool(d_st.any())
    return d_dig, dg, call


class Outs:
    def __init__(self, n, rows, n_all):
        self.t = (z64(n + 1), z64(4 * rows), z64(n + 1), z64(4 * rows), z64(3 * n), z64(6), z32(n_all))

    def same(self, other):
        """every output but the refuted count"""
        return all(bool((a == b).all()) for a, b in zip(self.t[:5] + self.t[6:], other.t[:5] + other.t[6:])) and bool((self.t[5][:5] == other.t[5][:5]).all())


def alternate(calls, reps, rounds):
    """{name: (mean, min, max) of its rounds' ms per execution}, the calls taking turns round by round"""
    seen = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            seen[k].append(event_ms(fn, reps))
    return {k: (round(sum(v) / len(v), 4), round(min(v), 4), round(max(v), 4)) for k, v in seen.items()}


def stages(ctx, fn, names, reps):
    fn()
    ctx.profile_enable(True)
    for _ in range(reps):
        fn()
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    assert all(prof[k][1] == reps for k in names), prof
    return {k.replace("_kernel", "") + "_ms": round(prof[k][0] / reps, 4) for k in names}


def run(ctx, B, files, reps, rounds):
    n = len(files)
    new_files, written = next_version(files, B)
    old, new = Container(ctx, LZNT1, B, files), Container(ctx, LZNT1, B, new_files)
    rows, n_all, total = new.nbt, 2 * n, old.nbt + new.nbt
    d_old, g_old, _ = column(ctx, old, B)
    d_new, g_new, digest_new = column(ctx, new, B)
    mt, md = m.BlockDeduper.for_match(ctx, B, 1, n_all, total, rows), m.BlockDigestMatcher(ctx, B, 1, n_all, total, rows)
    o_mt, o_md, o_x, o_r = (Outs(n, rows, n_all) for _ in range(4))
    bare = lambda v: (None,) + tuple(v[1:])
    match = lambda: mt.match([old.view], new.view, *o_mt.t)
    digest = lambda: md.match([bare(old.view)], [d_old], bare(new.view), d_new, *o_md.t)
    match(); digest()
    torch.cuda.synchronize()
    count = [int(x) for x in o_md.t[5].cpu().tolist()]
    found, shared, fresh, repeats = host_counts(files, new_files, B)
    assert o_md.same(o_mt) and count[:4] == [found, shared, fresh, new.nb] and count[5] == 0, (count, found, shared, fresh)
    # (a) alternating rounds, then the stages of each
    a = alternate({"match": match, "match_digest": digest}, reps, rounds)
    st_mt, st_md = stages(ctx, match, STAGES, reps), stages(ctx, digest, DIGEST_STAGES, reps)
    # (b) across codecs: the store as Xpress+Huffman
    xh = Container(ctx, XH, B, files)
    d_xh, g_xh, _ = column(ctx, xh, B)
    assert bool((d_xh[: 4 * xh.nb] == d_old[: 4 * old.nb]).all())                      # the column survives the codec
    cross = lambda: md.match([bare(xh.view)], [d_xh], bare(new.view), d_new, *o_x.t)
    groups = sum((x + B - 1) // B for x in xh.lens)
    tc = m.BlockTranscoder(ctx, XH, B, LZNT1, B, n, xh.nbt, old.nbt, groups)
    T = (torch.zeros(xh.total + 16, dtype=torch.uint8, device="cuda"), z64(n + 1), z64(old.nbt + 1), z32(old.nbt), z32(n))
    t_view = (T[0], T[1], T[2], xh.t_len, T[3], xh.total, n, old.nbt)

    def transcode():
        tc.transcode(xh.d_packed, xh.d_first, xh.d_boff, xh.t_len, T[0], T[1], T[2], T[4], d_block_crc=xh.d_crc, d_new_block_crc=T[3], packed_len=xh.packed_bytes,
                     new_cap=xh.total)

    def route():
        transcode()
        mt.match([t_view], new.view, *o_r.t)
    cross(); route()
    torch.cuda.synchronize()
    assert not bool(T[4].any()) and bool((T[0][: old.packed_bytes] == old.d_packed[: old.packed_bytes]).all())
    assert o_x.same(o_md) and o_r.same(o_mt) and int(o_x.t[5][4]) == int(o_r.t[5][4]) == count[4]      # the delta's size: equal
    b = alternate({"match_digest_cross": cross, "transcode_then_match": route, "transcode": transcode}, reps, rounds)
    # (c) the digest pass over next
    c = alternate({"digest_next": digest_new}, reps, rounds)
    for h in (mt, md, tc, g_old, g_new, g_xh, old.bk, new.bk, xh.bk):
        h.close()
    r = dict(block=B, resources=n, rows=new.nb, store_rows=old.nb, mb=round(new.total / 1e6, 1), packed_mb=round(new.packed_bytes / 1e6, 1), written=written,
             repeats=repeats, count=count, reps=reps, rounds=rounds)
    for k, v in {**a, **b, **c}.items():
        r[k + "_ms"], r[k + "_ms_min"], r[k + "_ms_max"] = v
    r["digest_over_match"] = round(a["match_digest"][0] / a["match"][0], 4)
    r["cross_over_route"] = round(b["match_digest_cross"][0] / b["transcode_then_match"][0], 5)
    r["match_stages"], r["match_digest_stages"] = st_mt, st_md
    return r


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "match_digest.json")
    torch.cuda.set_device(0)
    ctx = m.Context()
    files = [corpus.file_bytes(i) for i in range(12)]
    out = []
    for B in (65536, 4096):
        r = run(ctx, B, files, reps, rounds)
        print(json.dumps(r), flush=True)
        out.append(r)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
