"""GPU: the decompressed-size query (mscomp_amd_plan_create_size / mscomp_amd_plan_execute_size, api.SizePlan / decompressed_sizes /
decompress_units_auto) against the checker's one-shot decoder, the decompress plan and, where it was built, the compiled reference."""
import ctypes as C
import struct

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
FMTS = {"lznt1": 2, "xpress": 3, "xpress_huff": 4}
NO_LIMIT = (1 << 64) - 1


def _sizes(m, ctx, f, units, limits=None):
    ln, need, st = m.decompressed_sizes(f, units, limits, ctx=ctx)
    return [int(x) for x in ln], [int(x) for x in need], [int(x) for x in st]


@pytest.mark.parametrize("fmt", list(FMTS))
def test_sizes_match_checker_decoder_and_reference_at_given_limits(oracle, gpu_ctx, fmt):
    """every (stream, cap) of the decode families as one batch, limit = cap: status and length of the checker, of a decompress plan
    with out_cap = cap, and of the compiled reference; `need` is the smallest capacity that decodes (the checker at need and need - 1)"""
    import ms_compress_amd as m
    f = FMTS[fmt]
    streams = cases.decode_streams(f, lambda d: oracle.oracle_compress(f, d)[1])
    units, caps = [s for s, _ in streams], [c for _, c in streams]
    ln, need, st = _sizes(m, gpu_ctx, f, units, caps)
    outs, dst = m.decompress_units(f, units, caps, ctx=gpu_ctx)
    ref = oracle.load_ref()
    n_ok = n_plus = 0
    for i, (stream, cap) in enumerate(streams):
        assert st[i] == dst[i] and ln[i] == (len(outs[i]) if dst[i] == 0 else 0), (i, len(stream), cap, st[i], dst[i])
        so, oo, undefined = oracle.oracle_decompress_ex(f, stream, cap)
        if undefined:
            continue
        assert (st[i], ln[i]) == (so, len(oo) if so == 0 else 0), (i, len(stream), cap, st[i], so)
        if ref is not None:
            rs, ro = oracle.ref_decompress(f, stream, cap)
            assert (st[i], ln[i]) == (rs, len(ro) if rs == 0 else 0), (i, len(stream), cap)
        if st[i] != 0:
            assert need[i] == 0
            continue
        n_ok += 1
        d = need[i] - ln[i]
        assert d in (0, 1), (i, need[i], ln[i])
        if d:
            assert f == 2 and stream.endswith(b"\0\0"), i
            n_plus += 1
        assert oracle.oracle_decompress_ex(f, stream, need[i])[:2] == (0, oo), (i, need[i])
        if need[i] > 0:
            assert oracle.oracle_decompress_ex(f, stream, need[i] - 1)[0] != 0, (i, need[i])
    assert n_ok > 50
    if f == 2:
        assert n_plus > 0                                           # streams with the End_of_buffer header are among them


@pytest.mark.parametrize("fmt", list(FMTS))
def test_round_trip_with_capacity_need(oracle, gpu_ctx, fmt):
    """GPU-compressed edge units and corpus slices sized without a limit, then decoded with out_cap = need, back to back"""
    import ms_compress_amd as m
    from ms_compress_amd import corpus
    f = FMTS[fmt]
    data = corpus.by_name("mozilla", 900_000).tobytes()
    units = cases.edge_cases() + [cases.mixed_buffer()] + [data[a:b] for a, b in ((0, 65536), (70_000, 300_000), (300_000, 900_000))]
    comp, st = m.compress_units(f, units, ctx=gpu_ctx)
    assert all(s == 0 for s in st)
    ln, need, sst = _sizes(m, gpu_ctx, f, comp)
    for i, u in enumerate(units):
        if f == 3 and len(u) == 0:                                   # the reference's Xpress decoder rejects what its encoder writes for no input
            assert sst[i] == -3 and need[i] == 0 and ln[i] == 0
        else:
            assert sst[i] == 0 and ln[i] == len(u) and need[i] == len(u), (i, sst[i], ln[i], need[i], len(u))
    ok = [i for i in range(len(units)) if sst[i] == 0]
    back, bst = m.decompress_units(f, [comp[i] for i in ok], [need[i] for i in ok], ctx=gpu_ctx)
    assert all(s == 0 for s in bst) and all(b == units[i] for i, b in zip(ok, back))
    if f == 2:                                                       # the uncounted 00 00 that ms_compress writes when there is room
        term = [c + b"\0\0" for c in comp]
        ln2, need2, st2 = _sizes(m, gpu_ctx, f, term)
        assert all(s == 0 for s in st2) and ln2 == [len(u) for u in units] and need2 == [len(u) + 1 for u in units]
        back, bst = m.decompress_units(f, term, need2, ctx=gpu_ctx)
        assert all(s == 0 for s in bst) and back == units
        _, bst = m.decompress_units(f, term, [n - 1 for n in need2], ctx=gpu_ctx)
        assert all(s == m.MSCOMP_BUF_ERROR for s in bst)


@pytest.mark.parametrize("fmt", list(FMTS))
def test_no_scratch_by_limit(oracle, gpu_ctx, fmt):
    """20 000 small units, each with a limit of 2^40: scratch by capacity would be 20 000 TiB; the plan sizes by input"""
    import ms_compress_amd as m
    f = FMTS[fmt]
    srcs = [cases.mixed_buffer()[k * 997: k * 997 + 200 + 37 * k] for k in range(16)]
    comps = [oracle.oracle_compress(f, s)[1] for s in srcs]
    n = 20_000
    units = [comps[i % 16] for i in range(n)]
    ln, need, st = _sizes(m, gpu_ctx, f, units, [1 << 40] * n)
    assert all(s == 0 for s in st)
    assert ln == [len(srcs[i % 16]) for i in range(n)] and need == ln
    # a plan made with no limits at all (NULL), executed twice
    import torch
    dev = torch.device("cuda", gpu_ctx.device)
    lens = [len(u) for u in units]
    off, tot = m.pack_offsets(lens)
    blob = np.zeros(tot + 16, np.uint8)
    for u, o in zip(units, off):
        blob[int(o): int(o) + len(u)] = np.frombuffer(u, np.uint8)
    d_in = torch.from_numpy(blob).to(dev)
    d_len = torch.zeros(n, dtype=torch.int64, device=dev); d_need = torch.zeros_like(d_len); d_st = torch.full((n,), -9, dtype=torch.int32, device=dev)
    p = m.SizePlan(gpu_ctx, f, off, lens)
    for _ in range(2):
        d_len.zero_(); d_need.zero_(); d_st.fill_(-9)
        p.execute(d_in, d_len, d_need, d_st); torch.cuda.synchronize()
        assert bool((d_st == 0).all()) and d_len.cpu().tolist() == ln and d_need.cpu().tolist() == ln
    p.close()


def _xpress_huge(L32):
    """one literal and three matches of offset 1 whose lengths sit in 32-bit length fields: 1 + 3 * (L32 + 3) bytes"""
    m3 = struct.pack("<H", 7)                                        # offset 1, length field 7: a nibble follows
    s = struct.pack("<I", 0x7FFFFFFF) + b"A"                         # flags: a literal, then matches (and all flags behind them set)
    s += m3 + b"\xff" + b"\xff" + b"\0\0" + struct.pack("<I", L32)   # the nibble byte (15 | 15 << 4), length byte 255, 16-bit 0, 32-bit length
    s += m3 + b"\xff" + b"\0\0" + struct.pack("<I", L32)             # the pending high nibble (15)
    s += m3 + b"\x0f" + b"\xff" + b"\0\0" + struct.pack("<I", L32)   # a new nibble byte
    return s


def test_xpress_beyond_4_gib(oracle, gpu_ctx):
    import ms_compress_amd as m
    L32 = 0xB0000000                                                 # below the reference's 32-bit wrap of len + 3
    s = _xpress_huge(L32)
    want = 1 + 3 * (L32 + 3)
    assert want > (1 << 33)
    small = oracle.oracle_compress(3, b"abcabcabc" * 50)[1]
    ln, need, st = _sizes(m, gpu_ctx, 3, [s, small, s])
    assert st == [0, 0, 0] and ln == [want, 450, want] and need == ln
    ln, need, st = _sizes(m, gpu_ctx, 3, [s], [1 << 20])
    so, _, _ = oracle.oracle_decompress_ex(3, s, 1 << 20)
    assert so == m.MSCOMP_BUF_ERROR and st == [so] and ln == [0] and need == [0]


@pytest.mark.parametrize("fmt", list(FMTS))
def test_large_units_alone_and_among_thousands_of_small_ones(oracle, gpu_ctx, fmt):
    """LZNT1: the 51 MB mozilla-like unit; Xpress: a stream of 8 MB or more (segment walk); Xpress+Huffman: a buffer of 8 MB or more (chunk-parallel walk)"""
    import ms_compress_amd as m
    from ms_compress_amd import corpus
    f = FMTS[fmt]
    big = corpus.file_bytes(corpus.NAMES.index("mozilla"), 51_220_480 if f == 2 else 24_000_000).tobytes()
    (cbig,), st = m.compress_units(f, [big], ctx=gpu_ctx)
    assert st == [0] and len(cbig) >= 8_000_000
    ln, need, sst = _sizes(m, gpu_ctx, f, [cbig])
    assert sst == [0] and ln == [len(big)] and need == [len(big)]
    del big
    small_src = [cases.mixed_buffer()[k * 3001: k * 3001 + 1000 + 131 * k] for k in range(24)]
    small = [oracle.oracle_compress(f, s)[1] for s in small_src]
    units, want = [], []
    for i in range(3000):
        if i == 1500:
            units.append(cbig); want.append(ln[0])
        units.append(small[i % 24]); want.append(len(small_src[i % 24]))
    ln2, need2, st2 = _sizes(m, gpu_ctx, f, units)
    assert all(s == 0 for s in st2) and ln2 == want and need2 == want
    # and at limits just below / at the length of the large unit
    lim = [NO_LIMIT] * len(units)
    lim[1500] = want[1500] - 1
    _, _, st3 = _sizes(m, gpu_ctx, f, units, lim)
    assert st3[1500] == m.MSCOMP_BUF_ERROR and all(s == 0 for i, s in enumerate(st3) if i != 1500)


def test_plan_kinds_and_argument_errors(gpu_ctx):
    import torch
    import ms_compress_amd as m
    lib = gpu_ctx.lib
    dev = torch.device("cuda", gpu_ctx.device)
    d = torch.zeros(64, dtype=torch.uint8, device=dev)
    d_len = torch.zeros(1, dtype=torch.int64, device=dev); d_need = torch.zeros_like(d_len); d_st = torch.zeros(1, dtype=torch.int32, device=dev)
    off = np.zeros(1, np.uint64); ln = np.array([8], np.uint64); cap = np.array([100], np.uint64)
    sp = m.SizePlan(gpu_ctx, 2, off, ln)
    assert lib.mscomp_amd_plan_execute(sp._h, C.c_void_p(d.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(d_len.data_ptr()),
                                       C.c_void_p(d_st.data_ptr())) == m.MSCOMP_ARG_ERROR
    dp = m.Plan(gpu_ctx, 2, off, ln, off, cap, decompress=True)
    cp = m.Plan(gpu_ctx, 2, off, ln, off, cap)
    for p in (dp, cp):
        assert lib.mscomp_amd_plan_execute_size(p._h, C.c_void_p(d.data_ptr()), C.c_void_p(d_len.data_ptr()), C.c_void_p(d_need.data_ptr()),
                                                C.c_void_p(d_st.data_ptr())) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_plan_execute_size(sp._h, C.c_void_p(d.data_ptr()), C.c_void_p(d_len.data_ptr()), None,
                                            C.c_void_p(d_st.data_ptr())) == m.MSCOMP_ARG_ERROR
    sp.close(); dp.close(); cp.close()
    h = C.c_void_p()
    for bad in (0, 1, 5):
        assert lib.mscomp_amd_plan_create_size(gpu_ctx._h, bad, 1, off.ctypes.data, ln.ctypes.data, None, C.byref(h)) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_plan_create_size(gpu_ctx._h, 3, 1, None, ln.ctypes.data, None, C.byref(h)) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_plan_create_size(gpu_ctx._h, 3, 1, off.ctypes.data, None, None, C.byref(h)) == m.MSCOMP_ARG_ERROR
    huge = np.array([0xFFFFF001], np.uint64)
    for f in (2, 3, 4):
        assert lib.mscomp_amd_plan_create_size(gpu_ctx._h, f, 1, off.ctypes.data, huge.ctypes.data, None, C.byref(h)) == m.MSCOMP_ARG_ERROR
        assert lib.mscomp_amd_decompressed_size_batch(gpu_ctx._h, f, 1, C.c_void_p(d.data_ptr()), off.ctypes.data, huge.ctypes.data, None,
                                                      C.c_void_p(d_len.data_ptr()), C.c_void_p(d_need.data_ptr()), C.c_void_p(d_st.data_ptr())) == m.MSCOMP_ARG_ERROR
    # the one-call form
    comp = m.compress(2, b"hello hello hello hello")
    d[: len(comp)] = torch.frombuffer(bytearray(comp), dtype=torch.uint8).to(dev)
    ln1 = np.array([len(comp)], np.uint64)
    assert lib.mscomp_amd_decompressed_size_batch(gpu_ctx._h, 2, 1, C.c_void_p(d.data_ptr()), off.ctypes.data, ln1.ctypes.data, None,
                                                  C.c_void_p(d_len.data_ptr()), C.c_void_p(d_need.data_ptr()), C.c_void_p(d_st.data_ptr())) == 0
    assert int(d_st[0]) == 0 and int(d_len[0]) == 23 and int(d_need[0]) == 23


@pytest.mark.parametrize("fmt", list(FMTS))
def test_decompress_units_auto(oracle, gpu_ctx, fmt):
    import ms_compress_amd as m
    f = FMTS[fmt]
    streams = cases.decode_streams(f, lambda d: oracle.oracle_compress(f, d)[1], n_corrupt=20)
    units = [s for s, _ in streams]
    got, gst = m.decompress_units_auto(f, units, ctx=gpu_ctx)
    ln, need, st = _sizes(m, gpu_ctx, f, units)
    ok = [i for i in range(len(units)) if st[i] == 0]
    want, wst = m.decompress_units(f, [units[i] for i in ok], [need[i] for i in ok], ctx=gpu_ctx)
    assert len(ok) > 50
    for j, i in enumerate(ok):
        assert gst[i] == wst[j] == 0 and got[i] == want[j] and len(got[i]) == ln[i]
    for i in range(len(units)):
        if st[i] != 0:
            assert gst[i] == st[i] and got[i] is None
    # with limits: a unit that does not fit its limit keeps the size pass's status
    lim = [max(0, n - 1) if n else NO_LIMIT for n in need]
    got2, gst2 = m.decompress_units_auto(f, units, lim, ctx=gpu_ctx)
    for i in range(len(units)):
        if st[i] == 0 and need[i] > 0:
            assert gst2[i] != 0 and got2[i] is None
