"""GPU: compaction with device tables (mscomp_amd_compact_dev, api.compact_dev) against mscomp_amd_compact_batch, mscomp_amd_layout_dev and a
numpy gather on the same values, and the whole device-table chain (size -> layout -> decode -> re-encode -> pack -> size -> decode) in one
captured graph."""
import numpy as np
import pytest

from plans_rig import FMTS, GUARD, dt

pytestmark = pytest.mark.gpu


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _expected(src, src_off, lens, align):
    """numpy: the offsets (n + 1) and the packed bytes, padding zero"""
    n = len(lens)
    off = np.zeros(n + 1, np.uint64)
    for i in range(n):
        off[i + 1] = int(off[i]) + (int(lens[i]) + align - 1) // align * align
    out = np.zeros(int(off[n]), np.uint8)
    for i in range(n):
        out[int(off[i]): int(off[i]) + int(lens[i])] = src[int(src_off[i]): int(src_off[i]) + int(lens[i])]
    return off, out


def _run(ctx, d_src, src_off, lens, align, cap=None, slack=4096):
    """compact_dev into a guard-filled buffer: (offsets, every byte of the buffer, the room given)"""
    import torch
    import ms_compress_amd as m
    total = sum((int(x) + align - 1) // align * align for x in lens)
    room = total if cap is None else cap
    d_packed = torch.full((max(total, room) + slack,), GUARD, dtype=torch.uint8, device="cuda")
    d_off = torch.full((len(lens) + 1,), -1, dtype=torch.int64, device="cuda")
    m.compact_dev(ctx, d_src, dt(src_off), dt(lens), align, d_packed, d_off, packed_cap=room)
    torch.cuda.synchronize()
    return _u64(d_off), d_packed.cpu().numpy(), room


@pytest.mark.parametrize("fmt", list(FMTS))
def test_compact_dev_matches_compact_batch(gpu_ctx, fmt):
    """a mixed batch compressed by a host plan (0, 1, 4097, 70 000, 700 KiB and 3 MiB units, incompressible ones among them): compact_dev at
    align 1 gives the offsets and bytes of compact_batch, and at align 16 and 4096 the offsets of layout_dev, every unit's bytes and zero
    padding; nothing is written behind the total"""
    import torch
    import ms_compress_amd as m
    from ms_compress_amd import corpus
    f = FMTS[fmt]
    data = corpus.by_name("mozilla", 5_000_000).tobytes()
    rnd = np.random.default_rng(6)
    plain, pos = [], 0
    for s in (0, 1, 4097, 70_000, 700 << 10, 3 << 20, 33, 65536):
        plain.append(data[pos: pos + s])
        pos += s
    plain += [rnd.integers(0, 256, k, dtype=np.uint8).tobytes() for k in (5000, 65536, 200_001)]
    n = len(plain)
    lens = np.array([len(p) for p in plain], np.uint64)
    in_off, in_total = m.pack_offsets([len(p) for p in plain])
    blob = np.zeros(in_total + 16, np.uint8)
    for p, o in zip(plain, in_off):
        blob[int(o): int(o) + len(p)] = np.frombuffer(p, np.uint8)
    caps = np.array([m.max_compressed_size(f, len(p)) + 2 for p in plain], np.uint64)
    out_off, out_total = m.pack_offsets([int(c) for c in caps], align=1)      # capacities back to back: every source alignment occurs
    d_out = torch.zeros(out_total + 16, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
    plan = m.Plan(gpu_ctx, f, in_off, lens, out_off, caps)
    plan.execute(torch.from_numpy(blob).cuda(), d_out, d_len, d_st)
    ref_packed, ref_off = m.compact_batch(gpu_ctx, out_off, caps, d_out, d_len)
    torch.cuda.synchronize()
    plan.close()
    assert (d_st.cpu().numpy() == 0).all()
    clen, h_out = _u64(d_len), d_out.cpu().numpy()
    ref_off, ref_packed = _u64(ref_off), ref_packed.cpu().numpy()

    off, packed, room = _run(gpu_ctx, d_out, out_off, clen, 1)
    assert (off == ref_off).all() and int(off[n]) == int(clen.sum()) == room
    assert (packed[:room] == ref_packed[:room]).all()
    assert (packed[room:] == GUARD).all()
    for align in (16, 4096):
        off, packed, room = _run(gpu_ctx, d_out, out_off, clen, align)
        lay = m.layout_dev(gpu_ctx, d_len, align)
        torch.cuda.synchronize()
        assert (off == _u64(lay)).all()
        exp_off, exp = _expected(h_out, out_off, clen, align)       # (the units' bytes in place, zero in the padding)
        assert (off == exp_off).all() and (packed[:room] == exp).all() and (packed[room:] == GUARD).all()


def test_compact_dev_every_address_residue(gpu_ctx):
    """source offsets of every residue mod 16 with lengths 0..40 and a few around 64 KiB, destination offsets as they fall (align 1) and
    16-byte aligned: a numpy gather is the reference. Then one unit of 32 MiB + 5 among 4 000 small ones, at odd addresses."""
    import torch
    rnd = np.random.default_rng(7)
    lens, src_off, pos = [], [], 0
    for length in list(range(41)) + [65535, 65536, 65537, 65536 + 17, 4096 * 3 + 1]:
        for res in range(16):
            pos += (res - pos) % 16 + 16 * int(rnd.integers(0, 3))      # a gap, then the wanted residue
            src_off.append(pos)
            lens.append(length)
            pos += length
    order = rnd.permutation(len(lens))                               # units need not lie in source order
    lens, src_off = np.array(lens, np.uint64)[order], np.array(src_off, np.uint64)[order]
    src = rnd.integers(1, 256, pos + 16, dtype=np.uint8)             # (no zero byte: a missed byte cannot pass as padding)
    d_src = torch.from_numpy(src).cuda()
    for align in (1, 16):
        off, packed, room = _run(gpu_ctx, d_src, src_off, lens, align)
        exp_off, exp = _expected(src, src_off, lens, align)
        assert (off == exp_off).all() and room == len(exp)
        bad = np.nonzero(packed[:room] != exp)[0]
        assert len(bad) == 0, bad[:8]
        assert (packed[room:] == GUARD).all()

    big = (32 << 20) + 5
    lens = [int(x) for x in rnd.integers(1, 4097, 4000)]
    lens.insert(1234, big)
    src_off, pos = [], 3
    for k in lens:
        src_off.append(pos)
        pos += k + int(rnd.integers(0, 5))
    src = rnd.integers(1, 256, pos + 16, dtype=np.uint8)
    d_src = torch.from_numpy(src).cuda()
    off, packed, room = _run(gpu_ctx, d_src, np.array(src_off, np.uint64), np.array(lens, np.uint64), 1)
    exp_off, exp = _expected(src, src_off, lens, 1)
    assert (off == exp_off).all() and (packed[:room] == exp).all() and (packed[room:] == GUARD).all()


@pytest.mark.parametrize("align", [1, 16])
def test_compact_dev_stops_at_packed_cap(gpu_ctx, align):
    """packed_cap one byte short of a unit's end: that unit and everything behind it are absent, the bytes from its start on (and so from
    packed_cap on) are untouched, the units before it are complete, and d_packed_off[n] tells the device that the batch did not fit"""
    import torch
    rnd = np.random.default_rng(9)
    lens = np.array([int(x) for x in rnd.integers(0, 9000, 300)] + [0, 7], np.uint64)
    lens[150] = 70_001
    n = len(lens)
    src_off, pos = np.zeros(n, np.uint64), 5
    for i in range(n):
        src_off[i] = pos
        pos += int(lens[i]) + 3
    src = rnd.integers(1, 256, pos + 16, dtype=np.uint8)
    d_src = torch.from_numpy(src).cuda()
    exp_off, exp = _expected(src, src_off, lens, align)
    for k in (150, 151, 1, n - 1):
        if lens[k] == 0:
            continue
        cap = int(exp_off[k]) + int(lens[k]) - 1
        off, packed, room = _run(gpu_ctx, d_src, src_off, lens, align, cap=cap)
        start = int(exp_off[k])
        assert (off == exp_off).all() and int(off[n]) > cap
        assert (packed[:start] == exp[:start]).all(), k
        assert (packed[start:] == GUARD).all(), k
    off, packed, _ = _run(gpu_ctx, d_src, src_off, lens, align, cap=0)      # no room at all; and no unit at all
    assert (off == exp_off).all() and (packed == GUARD).all()
    off, packed, _ = _run(gpu_ctx, d_src, src_off[:0], lens[:0], align)
    assert list(off) == [0] and (packed == GUARD).all()


def _chain_batch(m, plain):
    comp, st = m.compress_units(2, plain)
    assert all(s == 0 for s in st)
    ref, st = m.compress_units(4, plain)
    assert all(s == 0 for s in st)
    c_off, c_total = m.pack_offsets([len(c) for c in comp])
    blob = np.zeros(c_total + 16, np.uint8)
    for c, o in zip(comp, c_off):
        blob[int(o): int(o) + len(c)] = np.frombuffer(c, np.uint8)
    return plain, ref, blob, c_off, np.array([len(c) for c in comp], np.uint64)


def test_whole_chain_in_one_captured_graph():
    """LZNT1 units on the device with only their offsets and lengths known: SizeDevPlan -> layout_dev(d_need) -> DevPlan decode ->
    plan_layout_dev(Xpress+Huffman, d_out_len) -> CompressDevPlan -> compact_dev -> SizeDevPlan (Xpress+Huffman) on the packed units ->
    DevPlan decode, captured once with torch.cuda.graph on the stream of the one context every stage shares -- each stage's first
    execution -- and replayed on three batches whose tables and bytes are rewritten in place. Nothing is read back inside the chain."""
    import torch
    import ms_compress_amd as m
    from ms_compress_amd import corpus
    data = corpus.by_name("mozilla", 2_000_000).tobytes()
    sizes = (1, 4097, 70_000, 65536, 300_000, 5000, 17, 131_072, 200_001, 33_000, 999, 8192)
    n = len(sizes)
    batches = []
    for b in range(3):
        plain, pos = [], 100_000 * b
        for s in sizes[b:] + sizes[:b]:
            plain.append(data[pos: pos + s + 7 * b])
            pos += s + 7 * b
        plain[5] = bytes(plain[5][:1]) * len(plain[5]) if b == 1 else plain[5]
        batches.append(_chain_batch(m, plain))
    in_max = max(int(x[4].sum()) for x in batches)
    plain_max = max(sum(len(p) for p in x[0]) for x in batches)
    unit_max = max(len(p) for x in batches for p in x[0])
    p_room = plain_max + 16 * n + 64
    x_room = max(sum(m.max_compressed_size(4, len(p)) for p in x[0]) for x in batches) + 16 * n + 64
    s = torch.cuda.Stream()
    ctx = m.Context(stream=s)
    with torch.cuda.stream(s):
        size1, dec1 = m.SizeDevPlan(ctx, 2, n, in_max), m.DevPlan(ctx, 2, n, in_max, p_room)
        enc = m.CompressDevPlan(ctx, 4, n, plain_max, unit_max)
        size2, dec2 = m.SizeDevPlan(ctx, 4, n, x_room), m.DevPlan(ctx, 4, n, x_room, p_room)
        d_comp = torch.zeros(max(len(x[2]) for x in batches), dtype=torch.uint8, device="cuda")
        d_coff, d_clen = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
        d_plain = torch.full((p_room,), GUARD, dtype=torch.uint8, device="cuda")
        d_x = torch.full((x_room,), GUARD, dtype=torch.uint8, device="cuda")
        d_packed = torch.full((x_room,), GUARD, dtype=torch.uint8, device="cuda")
        d_back = torch.full((p_room,), GUARD, dtype=torch.uint8, device="cuda")
        L = {k: torch.zeros(n, dtype=torch.int64, device="cuda") for k in ("s1", "need1", "plain", "xcap", "x", "s2", "need2", "back")}
        O = {k: torch.zeros(n + 1, dtype=torch.int64, device="cuda") for k in ("plain", "x", "packed")}
        S = [torch.full((n,), 77, dtype=torch.int32, device="cuda") for _ in range(5)]

        def load(batch):
            _, _, blob, c_off, c_len = batch
            d_comp[: len(blob)].copy_(torch.from_numpy(blob))
            d_coff.copy_(dt(c_off))
            d_clen.copy_(dt(c_len))
            for t in (d_plain, d_x, d_packed, d_back):
                t.fill_(GUARD)
            for t in S:
                t.fill_(77)

        def chain():
            size1.execute(d_comp, d_coff, d_clen, L["s1"], L["need1"], S[0])
            m.layout_dev(ctx, L["need1"], 16, d_off=O["plain"])
            dec1.execute(d_comp, d_coff, d_clen, d_plain, O["plain"], L["need1"], L["plain"], S[1])
            m.plan_layout_dev(ctx, 4, L["plain"], 16, d_off=O["x"], d_cap=L["xcap"])
            enc.execute(d_plain, O["plain"], L["plain"], d_x, O["x"], L["xcap"], L["x"], S[2])
            m.compact_dev(ctx, d_x, O["x"], L["x"], 1, d_packed, O["packed"])
            size2.execute(d_packed, O["packed"], L["x"], L["s2"], L["need2"], S[3])
            dec2.execute(d_packed, O["packed"], L["x"], d_back, O["plain"], L["need2"], L["back"], S[4])

        load(batches[0])
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        chain()
    for batch in batches[1:] + batches[:1]:
        with torch.cuda.stream(s):
            load(batch)
            g.replay()
        s.synchronize()
        plain, ref = batch[0], batch[1]
        for st in S:
            assert (st.cpu().numpy() == 0).all(), st.cpu().numpy()
        lens = [len(p) for p in plain]
        assert [int(x) for x in _u64(L["s2"])] == lens and [int(x) for x in _u64(L["need2"])] == lens
        assert [int(x) for x in _u64(L["back"])] == lens and [int(x) for x in _u64(L["plain"])] == lens
        poff, pkoff, back, packed = _u64(O["plain"]), _u64(O["packed"]), d_back.cpu().numpy(), d_packed.cpu().numpy()
        assert [int(x) for x in _u64(L["x"])] == [len(r) for r in ref]
        assert int(pkoff[n]) == sum(len(r) for r in ref) and (packed[int(pkoff[n]):] == GUARD).all()
        for i in range(n):
            assert bytes(packed[int(pkoff[i]): int(pkoff[i + 1])]) == ref[i], i
            assert bytes(back[int(poff[i]): int(poff[i]) + lens[i]]) == plain[i], i
    del g
    for p in (size1, dec1, enc, size2, dec2):
        p.close()
    ctx.close()
