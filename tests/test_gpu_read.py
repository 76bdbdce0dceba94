"""GPU: block readers (mscomp_amd_reader_*) against the model of tests/read_model.py -- bytes, lengths, statuses and the sharing counts --
on containers made by BlockContainer.compress, the whole output buffer compared with a sentinel image so that a byte written outside a
request's range fails."""
import numpy as np
import pytest

import blocks_model as M
import read_model as R
from blocks_rig import ReadRig, d64, flip, geometry, memo, same_image, slices, FMTS, BLOCKS, FILL, ALL, MIXED, TEXT, ZEROS5, MIXED5, RANDOM1

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rigs(gpu_ctx):
    yield from memo(lambda fmt, B: ReadRig.make(gpu_ctx, FMTS[fmt], B, R.buffers(B)))


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_geometry(rigs, oracle, fmt, B):
    rig = rigs(fmt, B)
    reqs = geometry(rig)
    order = np.random.RandomState(3).permutation(len(reqs))       # the same resource named many times, unsorted
    reqs = [reqs[i] for i in order]
    mo, ms, mc = rig.check(oracle, reqs)
    assert ms == [0] * len(reqs) and mo == slices(rig, reqs)
    assert mc[0] == rig.budget(reqs) and 0 < mc[2] < mc[1] <= int(rig.first[-1])      # raw and decoded blocks, each once
    mo, ms, _ = rig.check(oracle, reqs, crc=True)
    assert ms == [0] * len(reqs) and mo == slices(rig, reqs)


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_every_source_and_destination_residue(rigs, oracle, fmt, B):
    """40 bytes across the boundary between a raw and a compressed block, and 40 inside each, at every pair of residues mod 16"""
    rig = rigs(fmt, B)
    j = int(rig.first[MIXED])
    assert int(rig.off[j + 1] - rig.off[j]) == B and int(rig.off[j + 2] - rig.off[j + 1]) < B
    reqs, res = [], []
    for a in range(16):
        for d in range(16):
            reqs += [(MIXED, B - 24 + a, 40), (MIXED, 64 + a, 40 - d), (MIXED, B + 160 + a, 25 + d)]
            res += [d, d, d]
    mo, ms, _ = rig.check(oracle, reqs, residues=res)
    assert ms == [0] * len(reqs) and mo == slices(rig, reqs)


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_sharing(rigs, oracle, fmt, B):
    rig = rigs(fmt, B)
    reqs = [(TEXT, B + 31 * k, 100 + k) for k in range(16)]       # 16 requests into one block
    reqs += [(MIXED5, 0, 2 * B), (MIXED5, B, 2 * B), (MIXED5, 2 * B + 5, 2 * B), (MIXED5, 4 * B, B)]   # neighbours overlapping by one block
    reqs += [(ZEROS5, 10, 5 * B - 20), (ZEROS5, 0, ALL), (MIXED, 0, ALL), (MIXED, B - 1, 2)]
    mo, ms, (units, distinct, decoded) = rig.check(oracle, reqs, crc=True)
    assert ms == [0] * len(reqs) and mo == slices(rig, reqs)
    assert units == 16 + 2 + 2 + 3 + 1 + 5 + 5 + 4 + 2 and distinct == 1 + 5 + 5 + 4
    stored = [int(rig.off[k + 1] - rig.off[k]) for k in range(int(rig.first[-1]))]
    sizes = lambda r: [(stored[int(rig.first[r]) + k], min(B, rig.lens[r] - k * B)) for k in range((rig.lens[r] + B - 1) // B)]
    assert decoded == 1 + sum(s < e for r in (MIXED5, ZEROS5, MIXED) for s, e in sizes(r))
    # the same requests one per call
    rd = rig.m.BlockReader(rig.ctx, rig.fmt, B, rig.n, rig.nbt, 1, 5)
    for q, want in zip(reqs, mo):
        out, olen, st, ooff, counts = rig.read([q], 5, reader=rd)
        assert st == [0] and int(olen[0]) == len(want) and bytes(out[ooff[0]: ooff[0] + len(want)]) == want
        assert counts[0] == counts[1] == rig.budget([q])
    rd.close()


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_rejects(rigs, oracle, fmt, B):
    rig = rigs(fmt, B)
    reqs = [(MIXED, 5, 100), (rig.n, 0, 10), (TEXT, B - 1, B + 2), (ALL, 0, 1), (MIXED5, 7, 3 * B), (0, 0, 9), (TEXT, 3 * B, ALL), (RANDOM1, 1, 50)]
    caps = rig.wants(reqs)
    caps[4] -= 1; caps[7] -= 1                                    # a capacity one byte short
    mo, ms, _ = rig.check(oracle, reqs, caps=caps, blocks_max=64)
    assert ms == [0, M.ARG, 0, M.ARG, M.BUF, 0, 0, M.BUF]
    # the budget: covering blocks 1, -, 3, -, 4, 0, 1, 1
    caps = rig.wants(reqs)
    for bmax, want in ((9, [0, M.ARG, 0, M.ARG, 0, 0, 0, M.ARG]), (8, [0, M.ARG, 0, M.ARG, 0, 0, M.ARG, M.ARG]), (4, [0, M.ARG, 0, M.ARG, M.ARG, 0, M.ARG, M.ARG]),
                       (3, [0, M.ARG, M.ARG, M.ARG, M.ARG, 0, M.ARG, M.ARG]), (0, [M.ARG] * 5 + [0, M.ARG, M.ARG]), (10, [0, M.ARG, 0, M.ARG, 0, 0, 0, 0])):
        mo, ms, _ = rig.check(oracle, reqs, caps=caps, blocks_max=bmax)
        assert ms == want, (bmax, ms)
        assert [o for o, s in zip(mo, ms) if s == 0] == [b for b, s in zip(slices(rig, [q if q[0] < rig.n else (0, 0, 0) for q in reqs]), ms) if s == 0]
    # a request that fails the budget does not stop an empty one behind it, and BUF is decided before the budget
    caps[4] -= 1
    assert rig.check(oracle, reqs, caps=caps, blocks_max=5)[1] == [0, M.ARG, 0, M.ARG, M.BUF, 0, 0, M.ARG]
    assert rig.check(oracle, [], blocks_max=4)[1] == []           # no requests: MSCOMP_OK, nothing done


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_damage(rigs, oracle, fmt, B):
    rig = rigs(fmt, B)
    j = int(rig.first[MIXED])                                     # block 0 raw, block 1 compressed, block 2 raw, block 3 (17 bytes)
    assert int(rig.off[j + 1] - rig.off[j]) == B and int(rig.off[j + 2] - rig.off[j + 1]) < B
    reqs = [(MIXED, 0, 10), (MIXED, B - 1, 2), (MIXED, B + 9, B - 9), (MIXED, 2 * B, 5), (TEXT, 0, ALL), (MIXED, 3 * B, ALL), (MIXED, 0, ALL),
            (MIXED - 1, 0, ALL), (MIXED + 1, 0, 4 * B)]
    covers = [{0}, {0, 1}, {1}, {2}, set(), {3}, {0, 1, 2, 3}, set(), set()]
    hit = lambda blocks: [M.DATA if c & blocks else 0 for c in covers]
    off, first = rig.off, rig.first
    # a decreasing table; s > e with room in packed_len; s = 0 (the next block grows beyond its data length with it)
    bad = off.copy(); bad[j + 2] = bad[j + 1] - np.uint64(1)
    assert rig.check(oracle, reqs, boff=bad)[1] == hit({1, 2})      # (block 2 then starts a byte early: longer than its data)
    bad = off.copy(); bad[j + 4] = bad[j + 3] + np.uint64(B + 1)     # (the block behind it, of the next resource, then ends before it starts)
    st = rig.check(oracle, reqs, boff=bad, packed_len=rig.plen + 2 * B)[1]
    assert st[:5] == [0] * 5 and st[5:] == [M.DATA, M.DATA, 0, M.DATA]
    bad = off.copy(); bad[j + 2] = bad[j + 1]
    assert rig.check(oracle, reqs, boff=bad)[1] == hit({1, 2})
    # an end beyond packed_len: everything from block 2 of the target on
    st = rig.check(oracle, reqs, packed_len=int(off[j + 3]) - 1)[1]
    assert st[:4] == [0, 0, 0, M.DATA] and st[5:] == [M.DATA, M.DATA, 0, M.DATA]
    # a wrong block count: the resource and the one behind it
    bad = first.copy(); bad[MIXED + 1] += np.uint64(1)
    assert rig.check(oracle, reqs, first=bad)[1] == [M.DATA] * 4 + [0, M.DATA, M.DATA, 0, M.DATA]
    # block_first beyond the table
    bad = first.copy(); bad[rig.n] = np.uint64(rig.nbt + 1)
    assert rig.check(oracle, reqs + [(rig.n - 1, 0, 1)], first=bad)[1] == [0] * len(reqs) + [M.ARG]
    # payload: a flipped byte in a raw block, a flipped literal in a compressed one -- seen with checksums only; a broken stream -- seen always
    e1 = B
    for at, blocks, always in ((int(off[j]) + 77, {0}, False), (flip(oracle, rig, j + 1, e1, True), {1}, False), (flip(oracle, rig, j + 1, e1, False), {1}, True)):
        hurt = bytearray(rig.packed); hurt[at] ^= 0x01
        d_hurt = rig.d_packed.clone(); d_hurt[at] = int(hurt[at])
        assert rig.check(oracle, reqs, packed=d_hurt, model_packed=bytes(hurt))[1] == (hit(blocks) if always else [0] * len(reqs))
        assert rig.check(oracle, reqs, packed=d_hurt, model_packed=bytes(hurt), crc=True)[1] == hit(blocks)
        # damage in a block that no request covers changes nothing
        few = [q for q, c in zip(reqs, covers) if not c & blocks]
        for crc in (False, True):
            mo, ms, _ = rig.check(oracle, few, packed=d_hurt, model_packed=bytes(hurt), crc=crc)
            assert ms == [0] * len(few) and mo == slices(rig, few)


@pytest.mark.parametrize("fmt", list(FMTS))
def test_repeats_and_arguments_changed(rigs, oracle, fmt):
    """three executions with the same arguments (plain, captured, replayed), the request table rewritten in place between replays, then one
    changed pointer"""
    import torch
    B = 4096
    rig = rigs(fmt, B)
    dev = rig.dev
    sets = [[(MIXED, B - 5, 2 * B), (TEXT, 17, 300), (MIXED5, 0, ALL), (0, 0, 5), (MIXED, 0, B)],
            [(MIXED5, 4 * B + 1, ALL), (MIXED, 3 * B, 17), (TEXT, B, B), (TEXT, B + 1, 64), (RANDOM1, 9, 1)]]
    caps = [5 * B] * 5
    ooff, room = rig.layout(caps)
    rd = rig.m.BlockReader(rig.ctx, rig.fmt, B, rig.n, rig.nbt, 5, 12)
    d_req, d_ooff, d_ocap = d64([0] * 15, dev), d64(ooff, dev), d64(caps, dev)
    d_olen, d_st = torch.zeros(5, dtype=torch.int64, device=dev), torch.zeros(5, dtype=torch.int32, device=dev)
    outs = [torch.empty(room, dtype=torch.uint8, device=dev) for _ in range(2)]

    def run(reqs, d_out, crc):
        d_req.copy_(d64(np.array(reqs, dtype=np.uint64).reshape(-1), dev))
        d_out.fill_(FILL); d_olen.fill_(-1); d_st.fill_(77)
        rd.read(rig.d_packed, rig.d_first, rig.d_boff, rig.d_len, d_req, d_out, d_ooff, d_ocap, d_olen, d_st, d_block_crc=rig.d_crc if crc else None,
                packed_len=rig.plen)
        rig.ctx.stream.synchronize()
        out, olen, st = d_out.cpu().numpy(), d_olen.cpu().numpy(), d_st.cpu().numpy()
        for q, want in enumerate(slices(rig, reqs)):
            assert st[q] == 0 and int(olen[q]) == len(want), (q, st)
        same_image(out, list(zip(ooff, slices(rig, reqs))), FILL, "output")
    for _ in range(3):
        run(sets[0], outs[0], True)
    for k in (1, 0, 1):                                           # the table rewritten in place: the same graph
        run(sets[k], outs[0], True)
    run(sets[0], outs[1], True)                                   # another output buffer
    run(sets[1], outs[1], False)                                  # without checksums
    run(sets[1], outs[1], False)
    rd.close()


@pytest.mark.parametrize("fmt", ["lznt1", "xpress_huff"])
def test_replay_after_the_context_scratch_moved(fmt):
    """a reader's graph is keyed by the context's scratch as a plan's is: three reads (plain, captured, replayed), then a compress dev plan
    of a few hundred 64 KiB units on the same context, which grows the context's scratch, then two more reads (captured again, replayed) --
    all five give the slices of the original bytes"""
    import torch
    import ms_compress_amd as m
    f, B = FMTS[fmt], 4096
    text = (b"the quick brown fox jumps over the lazy dog %d " * 400) % tuple(range(400))
    bufs = [b"", text[:5000], text[5000: 5000 + 3 * B + 17]]
    assert len(bufs[2]) == 3 * B + 17
    s = torch.cuda.Stream()
    ctx = m.Context(stream=s)
    with torch.cuda.stream(s):
        rig = ReadRig.make(ctx, f, B, bufs)
        dev = rig.dev
        reqs = [(1, 100, 4500), (2, B - 7, 2 * B + 9), (2, 3 * B, ALL)]
        caps = [3 * B] * 3
        ooff, room = rig.layout(caps)
        rd = m.BlockReader(ctx, f, B, rig.n, rig.nbt, 3, rig.budget(reqs))
        d_req, d_ooff, d_ocap = d64(np.array(reqs, dtype=np.uint64).reshape(-1), dev), d64(ooff, dev), d64(caps, dev)
        d_olen, d_st = torch.zeros(3, dtype=torch.int64, device=dev), torch.zeros(3, dtype=torch.int32, device=dev)
        d_out = torch.empty(room, dtype=torch.uint8, device=dev)
        image = np.full(room, FILL, dtype=np.uint8)
        for q, want in enumerate(slices(rig, reqs)):
            assert len(want) == (4500, 2 * B + 9, 17)[q]
            image[ooff[q]: ooff[q] + len(want)] = np.frombuffer(want, dtype=np.uint8)

        def run():
            d_out.fill_(FILL); d_olen.fill_(-1); d_st.fill_(77)
            rd.read(rig.d_packed, rig.d_first, rig.d_boff, rig.d_len, d_req, d_out, d_ooff, d_ocap, d_olen, d_st, d_block_crc=rig.d_crc, packed_len=rig.plen)
            s.synchronize()
            assert d_st.cpu().tolist() == [0] * 3 and d_olen.cpu().tolist() == [4500, 2 * B + 9, 17]
            assert (d_out.cpu().numpy() == image).all()
        for _ in range(3):
            run()
        before = m.api.scratch_report(ctx, 0)
        n, U = 300, 65536
        big = m.CompressDevPlan(ctx, f, n, n * U, U)
        cap = m.max_compressed_size(f, U)
        d_in = torch.from_numpy(np.resize(np.frombuffer(text, dtype=np.uint8), n * U)).to(dev)
        d_big = torch.empty(n * cap, dtype=torch.uint8, device=dev)
        d_blen, d_bst = torch.zeros(n, dtype=torch.int64, device=dev), torch.full((n,), 77, dtype=torch.int32, device=dev)
        big.execute(d_in, d64(np.arange(n) * U, dev), d64([U] * n, dev), d_big, d64(np.arange(n) * cap, dev), d64([cap] * n, dev), d_blen, d_bst)
        s.synchronize()
        assert not d_bst.cpu().numpy().any()
        after = m.api.scratch_report(ctx, 0)
        assert any(0 < before[k][1] < after[k][1] for k in before), "the larger plan moved none of the context's buffers"
        for _ in range(2):
            run()
    big.close()
    rd.close()
    rig.close()
    ctx.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_compress_crc_and_read_in_one_captured_graph(oracle, fmt):
    """the container's compress and crc and the reader's read captured together, the reader's first execution inside the capture, then
    replayed over inputs rewritten in place: the read takes the tables and checksums the two calls before it wrote"""
    import torch
    import ms_compress_amd as m
    f, B = FMTS[fmt], 4096
    base = R.buffers(B)
    s = torch.cuda.Stream()
    ctx = m.Context(stream=s)
    with torch.cuda.stream(s):
        rig = ReadRig.make(ctx, f, B, base)
        reqs = [(MIXED, B - 5, 2 * B), (TEXT, 17, 300), (MIXED5, 0, ALL), (0, 0, 5), (MIXED, 0, B), (3, 0, ALL), (TEXT, 2 * B + 9, ALL)]
        caps = [5 * B] * len(reqs)
        ooff, room = rig.layout(caps)
        rd = m.BlockReader(ctx, f, B, rig.n, rig.nbt, len(reqs), 24)
        d_req, d_ooff, d_ocap = d64(np.array(reqs, dtype=np.uint64).reshape(-1), rig.dev), d64(ooff, rig.dev), d64(caps, rig.dev)
        d_olen, d_st = torch.zeros(len(reqs), dtype=torch.int64, device=rig.dev), torch.zeros(len(reqs), dtype=torch.int32, device=rig.dev)
        d_out = torch.empty(room, dtype=torch.uint8, device=rig.dev)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rig.compress()
        rd.read(rig.d_packed, rig.d_first, rig.d_boff, rig.d_len, d_req, d_out, d_ooff, d_ocap, d_olen, d_st, d_block_crc=rig.d_crc, packed_len=rig.total)
    for k in range(3):
        bufs = base[k:] + base[:k] if k < 2 else [b[::-1] for b in base]      # resources move, then other bytes of the same lengths
        with torch.cuda.stream(s):
            rig.load(bufs)
            d_out.fill_(FILL)
            g.replay()
        s.synchronize()
        out, olen, st = d_out.cpu().numpy(), d_olen.cpu().numpy(), d_st.cpu().numpy()
        for q, want in enumerate(slices(rig, reqs)):
            assert st[q] == 0 and int(olen[q]) == len(want), (k, q, st)
        same_image(out, list(zip(ooff, slices(rig, reqs))), FILL, ("output of replay", k))
    del g
    rd.close()
    rig.close()
    ctx.close()


def test_host_convenience(gpu_ctx, oracle):
    import ms_compress_amd as m
    f, B = 3, 4096
    bufs = R.buffers(B)
    lens = [len(b) for b in bufs]
    packed, first, off, st = m.blocks_compress(f, bufs, B, ctx=gpu_ctx)
    bcrc, _ = m.blocks_crc(f, bufs, B, ctx=gpu_ctx)
    reqs = [(MIXED, B - 5, 2 * B), (TEXT, 17, 300), (MIXED5, 0, ALL), (0, 0, 5), (len(bufs), 0, 1), (MIXED, 3 * B + 20, 4), (MIXED, 7, 0), (ZEROS5, 1, ALL)]
    want = [None if r >= len(bufs) else bufs[r][o: o + min(ln, lens[r])] for r, o, ln in reqs]
    for crc in (None, bcrc):
        got, dst = m.blocks_read(f, packed, first, off, lens, B, reqs, ctx=gpu_ctx, block_crc=crc)
        assert dst == [0, 0, 0, 0, M.ARG, 0, 0, 0] and got == want
    wrong = bcrc.copy(); wrong[int(first[TEXT])] ^= 1
    got, dst = m.blocks_read(f, packed, first, off, lens, B, reqs, ctx=gpu_ctx, block_crc=wrong)
    assert dst == [0, M.DATA, 0, 0, M.ARG, 0, 0, 0] and got[1] is None
    assert m.blocks_read(f, packed, first, off, lens, B, [], ctx=gpu_ctx) == ([], [])
