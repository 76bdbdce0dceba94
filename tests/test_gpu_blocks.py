"""GPU: block containers (mscomp_amd_blocks_*) against the model of tests/blocks_model.py -- packed bytes, both tables with their tail
entries, statuses, decoded ranges -- byte for byte, with guard regions behind every capacity."""
import numpy as np
import pytest

import blocks_model as M
from blocks_rig import BlockRig, d64, fixture_bufs, FMTS, FILL

pytestmark = pytest.mark.gpu
RANGES = [None, (0, 1), (1, 2), (2, 100), (1000, 5), (1, 0)]     # whole; one block; the middle; clipped at the end; beyond the end; an empty count


@pytest.fixture(scope="module")
def fixture():
    return M.load()


@pytest.mark.parametrize("B", M.BLOCK_SIZES)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_fixture_compress_and_ranged_decode(gpu_ctx, oracle, fixture, fmt, B):
    f = FMTS[fmt]
    bufs = fixture_bufs(fixture, f, B)
    total = sum(len(b) for b in bufs)
    rig = BlockRig(gpu_ctx, f, B, len(bufs), total)
    rig.load(bufs)
    mp, mf, mo, ms = rig.check_compress(oracle)
    assert not ms.any() and len(mp) == int(mo[-1])
    for r, rec in zip(range(len(bufs)), M.recipes_for(fixture, f, B)):     # the committed digests, resource by resource
        a, b = int(mf[r]), int(mf[r + 1])
        assert M.digest(mp[int(mo[a]): int(mo[b])], [0, b - a], list(mo[a: b + 1] - mo[a]) + [mo[b] - mo[a]] * (1 + len(bufs[r]) // B - (b - a))) \
            == fixture["digests"][fmt][str(B)][rec["id"]], rec["id"]
    for rng in RANGES:
        ranges = None if rng is None else [rng] * len(bufs)
        rig.set_out([len(b) for b in bufs])
        got, st = rig.check_decompress(oracle, (mp, len(mp), mf, mo), ranges)
        assert st == [0] * len(bufs)
        assert got == [b if rng is None else b[rng[0] * B: (rng[0] + rng[1]) * B] for b in bufs]
    # a range of its own per resource, and capacities that are exactly the bytes wanted
    ranges = [(r % 3, 1 + r % 2) for r in range(len(bufs))]
    rig.set_out([len(b[f0 * B: (f0 + c) * B]) for b, (f0, c) in zip(bufs, ranges)])
    assert rig.check_decompress(oracle, (mp, len(mp), mf, mo), ranges)[1] == [0] * len(bufs)
    rig.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_short_packed_cap_and_rejects(gpu_ctx, oracle, fixture, fmt):
    f, B = FMTS[fmt], 4096
    bufs = fixture_bufs(fixture, f, B)
    lens = [len(b) for b in bufs]
    total = sum(lens)
    rig = BlockRig(gpu_ctx, f, B, len(bufs), total)
    rig.load(bufs)
    _, mf, mo, _ = rig.check_compress(oracle)
    for cap in (0, 1, int(mo[int(mf[6])]) + 5, int(mo[int(mf[9]) + 1]), int(mo[-1]) - 1):
        mp, _, _, ms = rig.check_compress(oracle, packed_cap=cap)      # (the guard check covers everything behind the last block that fits)
        assert len(mp) <= cap and M.BUF in ms
    rig.close()
    # the resource that crosses in_total_max and every one behind it: rejected; the earlier ones: as before
    cut = sum(lens[:9]) - 1
    rig = BlockRig(gpu_ctx, f, B, len(bufs), cut, in_room=total)
    rig.load(bufs)
    mp, mf, mo, ms = rig.check_compress(oracle)
    assert [int(s) for s in ms] == [0] * 8 + [M.ARG] * (len(bufs) - 8)
    rig.set_out(lens)
    got, st = rig.check_decompress(oracle, (mp, len(mp), mf, mo))
    assert st == [0] * 8 + [M.ARG] * (len(bufs) - 8) and got[:8] == bufs[:8]
    rig.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_damaged_tables_and_payload(gpu_ctx, oracle, fixture, fmt):
    import torch
    f, B = FMTS[fmt], 4096
    bufs = fixture_bufs(fixture, f, B)
    lens = [len(b) for b in bufs]
    n, total = len(bufs), sum(lens)
    rig = BlockRig(gpu_ctx, f, B, n, total)
    rig.load(bufs)
    mp, mf, mo, ms = rig.check_compress(oracle)
    rig.set_out(lens)
    dev = rig.dev
    target = 8                                                    # "mixed", 3 B + 7: raw and compressed blocks
    j = int(mf[target])
    comp = next(k for k in range(j, int(mf[target + 1])) if int(mo[k + 1] - mo[k]) < min(B, lens[target] - (k - j) * B))

    def tables(first=None, off=None):
        return (mp, len(mp), mf if first is None else first, mo if off is None else off), dict(first=None if first is None else d64(first, dev),
                                                                                                boff=None if off is None else d64(off, dev))
    # a decreasing offset
    bad = mo.copy(); bad[j + 1] = bad[j] - 1
    a, kw = tables(off=bad)
    assert rig.check_decompress(oracle, a, **kw)[1][target] == M.DATA
    # s > e (packed_len leaves room for it: the table check alone refuses it), and s == 0
    bad = mo.copy(); bad[j + 1] = bad[j] + np.uint64(B + 1)
    a, kw = tables(off=bad)
    _, st = rig.check_decompress(oracle, (a[0], len(mp) + 2 * B, a[2], a[3]), **kw)
    assert st[target] == M.DATA and st[:target] == [0] * target
    bad = mo.copy(); bad[j + 1] = bad[j]
    a, kw = tables(off=bad)
    assert rig.check_decompress(oracle, a, **kw)[1][target] == M.DATA
    # a wrong block count
    bad = mf.copy(); bad[target + 1] += np.uint64(1)
    a, kw = tables(first=bad)
    _, st = rig.check_decompress(oracle, a, **kw)
    assert st[target] == M.DATA and st[target + 1] == M.DATA and st[:target] == [0] * target
    # block_first beyond n_blocks_max
    bad = mf.copy(); bad[n] = np.uint64(rig.nbmax + 1)
    a, kw = tables(first=bad)
    assert rig.check_decompress(oracle, a, **kw)[1][n - 1] == M.ARG
    # a block ending beyond packed_len
    plen = int(mo[j + 2]) - 1
    _, st = rig.check_decompress(oracle, (mp, plen, mf, mo))
    assert st[:target] == [0] * target and st[target] == M.DATA
    # a corrupted compressed payload: the first byte flip that the reference's decoder refuses with defined behaviour
    o0, o1 = int(mo[comp]), int(mo[comp + 1])
    e = min(B, lens[target] - (comp - j) * B)
    for p in range(o1 - o0):
        blk = bytearray(mp[o0:o1]); blk[p] ^= 0xFF
        ds, got, undefined = oracle.oracle_decompress_ex(f, bytes(blk), e)
        if (ds != 0 or len(got) != e) and not undefined:
            break
    else:
        raise AssertionError("no byte flip damages this block")
    hurt = bytearray(mp); hurt[o0 + p] ^= 0xFF
    d_hurt = rig.d_packed.clone()
    d_hurt[o0 + p] = hurt[o0 + p]
    _, st = rig.check_decompress(oracle, (bytes(hurt), len(mp), mf, mo), packed=d_hurt)
    assert st[target] == M.DATA and [s for r, s in enumerate(st) if r != target] == [0] * (n - 1)
    # d_out_cap one byte short
    caps = list(lens); caps[target] -= 1; caps[5] -= 1
    rig.set_out(caps)
    _, st = rig.check_decompress(oracle, (mp, len(mp), mf, mo))
    assert st[target] == M.BUF and st[5] == M.BUF and sum(s != 0 for s in st) == 2
    rig.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_repeats_and_tables_changed_in_place(gpu_ctx, oracle, fixture, fmt):
    """five executions of one object give the same; then the inputs and tables change behind the same pointers"""
    f, B = FMTS[fmt], 32768
    bufs = fixture_bufs(fixture, f, B)
    n, total = len(bufs), sum(len(b) for b in bufs)
    rig = BlockRig(gpu_ctx, f, B, n, total)
    rig.load(bufs)
    rig.set_out([len(b) for b in bufs])
    seen = set()
    for _ in range(5):
        mp, mf, mo, ms = rig.check_compress(oracle)
        out, olen, st = rig.decompress()
        seen.add((bytes(rig.compressed()[0]), bytes(out), bytes(olen), bytes(st)))
    assert len(seen) == 1
    assert rig.check_decompress(oracle, (mp, len(mp), mf, mo))[0] == bufs
    other = [b[::-1][: len(b) - (len(b) > 5000) * 4097] for b in bufs[::-1]]     # other bytes, other lengths, other block counts
    rig.load(other)
    rig.set_out([len(b) for b in other])
    for _ in range(2):
        mp2, mf2, mo2, ms2 = rig.check_compress(oracle)
        assert not ms2.any() and mp2 != mp
        assert rig.check_decompress(oracle, (mp2, len(mp2), mf2, mo2), [(1, 1)] * n)[0] == [b[B: 2 * B] for b in other]
        assert rig.check_decompress(oracle, (mp2, len(mp2), mf2, mo2))[0] == other
    rig.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_compress_and_decompress_in_one_captured_graph(gpu_ctx, oracle, fixture, fmt):
    """both calls captured together with torch.cuda.graph, the object's first execution inside the capture, then replayed three times
    over inputs rewritten in place -- no host synchronisation between the two calls, the decode reading the tables the compress wrote"""
    import torch
    import ms_compress_amd as m
    f, B = FMTS[fmt], 65536
    base = fixture_bufs(fixture, f, B)
    n, total = len(base), sum(len(b) for b in base)
    s = torch.cuda.Stream()
    ctx = m.Context(stream=s)
    with torch.cuda.stream(s):
        rig = BlockRig(ctx, f, B, n, total)
        rig.load(base)
        rig.set_out([len(b) for b in base])
        rig.d_packed.fill_(FILL); rig.d_out.fill_(FILL)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rig.bk.compress(rig.d_in, rig.d_off, rig.d_len, rig.d_packed, rig.d_first, rig.d_boff, rig.d_cst, packed_cap=total)
        rig.bk.decompress(rig.d_packed, rig.d_first, rig.d_boff, rig.d_len, rig.d_out, rig.d_ooff, rig.d_ocap, rig.d_olen, rig.d_dst, packed_len=total)
    for k in range(3):
        bufs = base[k:] + base[:k]
        if k == 2:
            bufs = [b[: len(b) // 2] for b in bufs]
        with torch.cuda.stream(s):
            rig.load(bufs)
            rig.set_out([len(b) for b in bufs])
            rig.d_packed.fill_(FILL); rig.d_out.fill_(FILL)
            g.replay()
        s.synchronize()
        mp, mf, mo, ms = M.model_compress(oracle, f, bufs, B, total, total)
        packed, first, off, st = rig.compressed()
        assert (first == mf).all() and (off == mo).all() and not st.any() and bytes(packed[: len(mp)]) == mp and (packed[len(mp):] == FILL).all()
        out, olen, dst = rig.d_out.cpu().numpy(), rig.d_olen.cpu().numpy(), rig.d_dst.cpu().numpy()
        for r, b in enumerate(bufs):
            assert dst[r] == 0 and int(olen[r]) == len(b) and bytes(out[rig.ooff[r]: rig.ooff[r] + len(b)]) == b, (k, r)
    del g
    rig.close()
    ctx.close()


def test_tables_compose_with_layout_and_compact_dev(gpu_ctx, oracle, fixture):
    """the stored lengths of d_block_off feed mscomp_amd_layout_dev (which rebuilds d_block_off) and mscomp_amd_compact_dev (which repacks
    the blocks at 16-byte starts), all on the device"""
    import ms_compress_amd as m
    f, B = 3, 4096
    bufs = fixture_bufs(fixture, f, B)
    total = sum(len(b) for b in bufs)
    rig = BlockRig(gpu_ctx, f, B, len(bufs), total)
    rig.load(bufs)
    mp, mf, mo, ms = rig.check_compress(oracle)
    d_slen = rig.d_boff[1:] - rig.d_boff[:-1]
    d_again = m.layout_dev(gpu_ctx, d_slen, align=1)
    d_packed16, d_off16 = m.compact_dev(gpu_ctx, rig.d_packed, rig.d_boff[:-1].contiguous(), d_slen, align=16)
    gpu_ctx.stream.synchronize()
    assert (d_again.cpu().numpy().view(np.uint64) == mo).all()
    p16, o16 = d_packed16.cpu().numpy(), d_off16.cpu().numpy()
    for k in range(int(mf[-1])):
        assert o16[k] % 16 == 0 and bytes(p16[int(o16[k]): int(o16[k]) + int(mo[k + 1] - mo[k])]) == mp[int(mo[k]): int(mo[k + 1])]
    rig.close()


def test_host_conveniences(gpu_ctx, oracle, fixture):
    import ms_compress_amd as m
    f, B = 2, 4096
    bufs = fixture_bufs(fixture, f, B)
    total = sum(len(b) for b in bufs)
    packed, first, off, st = m.blocks_compress(f, bufs, B, ctx=gpu_ctx)
    mp, mf, mo, ms = M.model_compress(oracle, f, bufs, B, total, total)
    nb = int(mf[-1])
    assert bytes(packed) == mp and (first == mf).all() and (off == mo[: nb + 1]).all() and not st.any()
    got, dst = m.blocks_decompress(f, packed, first, off, [len(b) for b in bufs], B, ctx=gpu_ctx)
    assert dst == [0] * len(bufs) and got == bufs
    got, dst = m.blocks_decompress(f, packed, first, off, [len(b) for b in bufs], B, ranges=[(1, 2)] * len(bufs), ctx=gpu_ctx)
    assert dst == [0] * len(bufs) and got == [b[B: 3 * B] for b in bufs]
    assert m.blocks_compress(f, [], B, ctx=gpu_ctx)[1].tolist() == [0]
