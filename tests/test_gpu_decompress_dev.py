"""GPU: decompress plans with device tables (mscomp_amd_plan_create_decompress_dev / mscomp_amd_plan_execute_dev, api.DevPlan) and
mscomp_amd_layout_dev (api.layout_dev), against host-table decompress plans on the same units."""
import ctypes as C

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
FMTS = {"lznt1": 2, "xpress": 3, "xpress_huff": 4}
GUARD = 0xEE
GAP = 48                                                             # guard bytes between the capacities of two units


def _dt(a):
    """a uint64 host table as an int64 CUDA tensor"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.uint64)).view(np.int64).copy()).cuda()


def _layout(units, caps):
    import ms_compress_amd as m
    lens = [len(u) for u in units]
    in_off, in_total = m.pack_offsets(lens)
    out_off, pos = np.zeros(len(caps), np.uint64), GAP
    for i, c in enumerate(caps):
        out_off[i] = pos
        pos += int(c) + GAP
    blob = np.zeros(in_total + 16, np.uint8)
    for u, o in zip(units, in_off):
        blob[int(o): int(o) + len(u)] = np.frombuffer(bytes(u), np.uint8)
    return blob, in_off, np.array(lens, np.uint64), out_off, np.array(caps, np.uint64), pos + GAP


def _host(ctx, f, blob, in_off, lens, out_off, caps, out_total):
    """a fresh host-table decompress plan: (out_len, status, output bytes incl. guards)"""
    import torch
    import ms_compress_amd as m
    n = len(lens)
    d_in = torch.from_numpy(blob).cuda()
    d_out = torch.full((out_total,), GUARD, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(max(1, n), dtype=torch.int64, device="cuda")
    d_st = torch.zeros(max(1, n), dtype=torch.int32, device="cuda")
    plan = m.Plan(ctx, f, in_off, lens, out_off, caps, decompress=True)
    plan.execute(d_in, d_out, d_len, d_st)
    torch.cuda.synchronize()
    plan.close()
    return d_len.cpu().numpy()[:n], d_st.cpu().numpy()[:n], d_out.cpu().numpy()


class DevRun:
    """one dev plan and the device buffers of its batches: tables and bytes are rewritten in place between executions"""

    def __init__(self, ctx, f, n, in_bytes, out_bytes, in_max, out_max):
        import torch
        import ms_compress_amd as m
        self.plan = m.DevPlan(ctx, f, n, in_max, out_max)
        self.n = n
        self.d_in = torch.zeros(in_bytes, dtype=torch.uint8, device="cuda")
        self.d_out = torch.full((out_bytes,), GUARD, dtype=torch.uint8, device="cuda")
        self.tabs = [torch.zeros(max(1, n), dtype=torch.int64, device="cuda") for _ in range(4)]
        self.d_len = torch.zeros(max(1, n), dtype=torch.int64, device="cuda")
        self.d_st = torch.full((max(1, n),), 77, dtype=torch.int32, device="cuda")

    def load(self, blob, in_off, lens, out_off, caps):
        import torch
        self.d_in[: len(blob)].copy_(torch.from_numpy(blob))
        for t, a in zip(self.tabs, (in_off, lens, out_off, caps)):
            t[: self.n].copy_(_dt(a))
        self.d_out.fill_(GUARD)

    def execute(self):
        i_off, i_len, o_off, o_cap = self.tabs
        self.plan.execute(self.d_in, i_off, i_len, self.d_out, o_off, o_cap, self.d_len, self.d_st)

    def result(self):
        import torch
        torch.cuda.synchronize()
        return self.d_len.cpu().numpy()[: self.n], self.d_st.cpu().numpy()[: self.n], self.d_out.cpu().numpy()


def _same(host, dev, out_off, caps, out_total, accepted=None):
    hl, hs, ho = host
    dl, ds, do = dev
    n = len(caps)
    inside = np.zeros(len(do), bool)
    for i in range(n):
        if accepted is not None and not accepted[i]:
            assert ds[i] == -2 and dl[i] == 0, (i, ds[i], dl[i])
            continue
        assert (ds[i], dl[i]) == (hs[i], hl[i]), (i, ds[i], hs[i], dl[i], hl[i])
        o = int(out_off[i])
        if hs[i] == 0:
            assert bytes(do[o: o + int(dl[i])]) == bytes(ho[o: o + int(hl[i])]), i
        inside[o: o + int(caps[i])] = True
    outside = ~inside
    outside[out_total:] = True
    assert (do[outside] == GUARD).all(), np.nonzero(do[outside] != GUARD)[0][:8]


def _corpus_units(m, f, sizes=(65536, 700 << 10, 3 << 20)):
    from ms_compress_amd import corpus
    data = corpus.by_name("mozilla", sum(sizes) + 1000).tobytes()
    plain, pos = [], 0
    for s in sizes:
        plain.append(data[pos: pos + s])
        pos += s
    comp, st = m.compress_units(f, plain)
    assert all(s == 0 for s in st)
    return plain, comp


@pytest.mark.parametrize("fmt", list(FMTS))
def test_dev_plan_matches_host_plan(oracle, gpu_ctx, fmt):
    """the decode families (valid, cut, concatenated, corrupted streams at their capacities) and corpus units of 64 KiB, 700 KiB and 3 MB,
    where host plans take their optional paths: status, length and bytes as a host plan's; nothing written outside the capacities"""
    import ms_compress_amd as m
    f = FMTS[fmt]
    streams = cases.decode_streams(f, lambda d: oracle.oracle_compress(f, d)[1])
    plain, comp = _corpus_units(m, f)
    units = [s for s, _ in streams] + comp
    caps = [c for _, c in streams] + [len(p) for p in plain]
    blob, in_off, lens, out_off, caps, out_total = _layout(units, caps)
    host = _host(gpu_ctx, f, blob, in_off, lens, out_off, caps, out_total)
    r = DevRun(gpu_ctx, f, len(units), len(blob), out_total + 4096, int(lens.sum()), int(caps.sum()))
    r.load(blob, in_off, lens, out_off, caps)
    r.execute()
    dev = r.result()
    _same(host, dev, out_off, caps, out_total)
    assert (dev[1][-3:] == 0).all() and all(bytes(dev[2][int(out_off[-3 + k]): int(out_off[-3 + k]) + len(plain[k])]) == plain[k] for k in range(3))
    assert sum(int(s) == 0 for s in dev[1]) > 50


@pytest.mark.parametrize("fmt", list(FMTS))
def test_one_dev_plan_several_batches(oracle, gpu_ctx, fmt):
    """one plan, three batches of the same unit count with other lengths, capacities and offsets, tables rewritten in place (the second
    and third executions replay the plan's own graph): each result is that of a fresh host plan"""
    import ms_compress_amd as m
    f = FMTS[fmt]
    streams = cases.decode_streams(f, lambda d: oracle.oracle_compress(f, d)[1], n_corrupt=20)
    rnd = np.random.default_rng(3)
    n = 120
    batches = []
    for b in range(3):
        pick = rnd.choice(len(streams), n, replace=False)
        units = [streams[i][0] for i in pick]
        caps = [streams[i][1] + int(rnd.integers(0, 3)) * b for i in pick]
        batches.append(_layout(units, caps))
    in_max = max(int(x[2].sum()) for x in batches)
    out_max = max(int(x[4].sum()) for x in batches)
    r = DevRun(gpu_ctx, f, n, max(len(x[0]) for x in batches), max(x[5] for x in batches) + 4096, in_max, out_max)
    for blob, in_off, lens, out_off, caps, out_total in batches:
        r.load(blob, in_off, lens, out_off, caps)
        r.execute()
        dev = r.result()
        _same(_host(gpu_ctx, f, blob, in_off, lens, out_off, caps, out_total), dev, out_off, caps, out_total)


@pytest.mark.parametrize("fmt", list(FMTS))
def test_chains_stay_on_the_device(gpu_ctx, fmt):
    """compress plan -> compact_batch -> execute_dev (in_off = the packed offsets, in_len = the compress plan's d_out_len), and size plan ->
    layout_dev(d_need) -> execute_dev (out_cap = d_need): no copy to the host between the stages, both give the original bytes back"""
    import torch
    import ms_compress_amd as m
    from ms_compress_amd import corpus
    f = FMTS[fmt]
    data = corpus.by_name("mozilla", 1_200_000).tobytes()
    cuts = [0, 1, 4097, 70_000, 200_000, 200_100, 600_000, 1_200_000]
    plain = [data[a:b] for a, b in zip(cuts, cuts[1:])] + [bytes(5000), b"abc" * 999]
    n = len(plain)
    blob, in_off, lens, _, _, _ = _layout(plain, [0] * n)
    cap = [m.max_compressed_size(f, len(u)) + 2 for u in plain]
    c_off, c_total = m.pack_offsets(cap)
    d_plain = torch.from_numpy(blob).cuda()
    d_comp = torch.zeros(c_total + 16, dtype=torch.uint8, device="cuda")
    d_clen = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_cst = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_plain_off, d_plain_len = _dt(in_off), _dt(lens)
    cplan = m.Plan(gpu_ctx, f, in_off, lens, c_off, cap)
    cplan.execute(d_plain, d_comp, d_clen, d_cst)
    d_packed, d_poff = m.compact_batch(gpu_ctx, c_off, cap, d_comp, d_clen)
    out_total = int(lens.sum()) + 16 * n + 64
    dplan = m.DevPlan(gpu_ctx, f, n, c_total, int(lens.sum()))
    d_out = torch.full((out_total,), GUARD, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_st = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    dplan.execute(d_packed, d_poff, d_clen, d_out, d_plain_off, d_plain_len, d_len, d_st)
    torch.cuda.synchronize()
    assert (d_cst.cpu().numpy() == 0).all()
    st, ln, out = d_st.cpu().numpy(), d_len.cpu().numpy(), d_out.cpu().numpy()
    for i, u in enumerate(plain):
        o = int(in_off[i])
        assert (st[i], ln[i]) == (0, len(u)) and bytes(out[o: o + len(u)]) == u, (i, st[i], ln[i], len(u))

    # the size query's d_need as the capacities, laid out on the device
    h_clen, h_poff = d_clen.cpu().numpy().view(np.uint64), d_poff.cpu().numpy().view(np.uint64)   # (host tables of the size plan, made beforehand)
    splan = m.SizePlan(gpu_ctx, f, h_poff[:n], h_clen)
    d_slen = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_need = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_sst = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_out.fill_(GUARD)
    d_st.fill_(77)
    torch.cuda.synchronize()
    splan.execute(d_packed, d_slen, d_need, d_sst)
    d_ooff = m.layout_dev(gpu_ctx, d_need, 16)
    dplan.execute(d_packed, d_poff, d_clen, d_out, d_ooff, d_need, d_len, d_st)
    torch.cuda.synchronize()
    ooff, need = d_ooff.cpu().numpy().view(np.uint64), d_need.cpu().numpy().view(np.uint64)
    assert int(ooff[0]) == 0 and all(int(ooff[i + 1]) == int(ooff[i]) + (int(need[i]) + 15) // 16 * 16 for i in range(n))
    st, ln, out = d_st.cpu().numpy(), d_len.cpu().numpy(), d_out.cpu().numpy()
    for i, u in enumerate(plain):
        o = int(ooff[i])
        assert (st[i], ln[i]) == (0, len(u)) and bytes(out[o: o + len(u)]) == u, (i, st[i], ln[i], len(u))
    assert (out[int(ooff[n]):] == GUARD).all()
    for p in (cplan, splan, dplan):
        p.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_units_past_the_bounds_are_refused(oracle, gpu_ctx, fmt):
    """an in_len above 0xFFFFF000, and running totals that cross in_total_max / out_total_max partway: those units get MSCOMP_ARG_ERROR
    with length 0, the others decode as with a host plan, and nothing is written outside the accepted units' capacities"""
    import torch
    f = FMTS[fmt]
    streams = [s for s in cases.decode_streams(f, lambda d: oracle.oracle_compress(f, d)[1], n_corrupt=0) if len(s[0]) > 8 and s[1] > 8][::7][:40]
    units, caps = [s for s, _ in streams], [c for _, c in streams]
    n = len(units)
    blob, in_off, lens, out_off, caps, out_total = _layout(units, caps)
    host = _host(gpu_ctx, f, blob, in_off, lens, out_off, caps, out_total)
    big = 0xFFFFF000 + 1
    # the unit with the long in_len spans an input buffer that really is that long (zeros), its capacity is small
    r = DevRun(gpu_ctx, f, n, big + len(blob) + 64, out_total + 4096, big + int(lens.sum()), int(caps.sum()))
    lens_bad = lens.copy()
    lens_bad[3] = big
    in_off_bad = in_off.copy()
    in_off_bad[3] = 0
    r.load(blob, in_off_bad, lens_bad, out_off, caps)
    r.execute()
    acc = np.ones(n, bool)
    acc[3] = False
    _same(host, r.result(), out_off, caps, out_total, acc)

    for in_cut, out_cut in ((n // 2, None), (None, 2 * n // 3), (n // 4, n // 3)):
        in_max = int(lens[: in_cut].sum()) + int(lens[in_cut]) // 2 if in_cut is not None else int(lens.sum())
        out_max = int(caps[: out_cut].sum()) + int(caps[out_cut]) // 2 if out_cut is not None else int(caps.sum())
        lim = min(x for x in (in_cut, out_cut, n) if x is not None)
        r = DevRun(gpu_ctx, f, n, len(blob), out_total + 4096, in_max, out_max)
        r.load(blob, in_off, lens, out_off, caps)
        r.execute()
        _same(host, r.result(), out_off, caps, out_total, np.arange(n) < lim)
    del r
    torch.cuda.synchronize()


def test_plan_kinds_are_kept_apart(gpu_ctx):
    """each execute function refuses the other kinds of plan with MSCOMP_ARG_ERROR and enqueues nothing"""
    import torch
    import ms_compress_amd as m
    lib = m.load_library()
    n = 2
    off = np.array([0, 16], np.uint64)
    ln = np.array([10, 10], np.uint64)
    host_d = m.Plan(gpu_ctx, 2, off, ln, off, ln, decompress=True)
    host_c = m.Plan(gpu_ctx, 2, off, ln, off, np.array([20, 20], np.uint64))
    size = m.SizePlan(gpu_ctx, 2, off, ln)
    dev = m.DevPlan(gpu_ctx, 2, n, 64, 64)
    d_in = torch.zeros(64, dtype=torch.uint8, device="cuda")
    d_out = torch.full((64,), GUARD, dtype=torch.uint8, device="cuda")
    t = [_dt(off), _dt(ln), _dt(off), _dt(ln)]
    d_len = torch.full((n,), 5, dtype=torch.int64, device="cuda")
    d_need = torch.full((n,), 5, dtype=torch.int64, device="cuda")
    d_st = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    P = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    for p in (host_d, host_c, size):
        assert lib.mscomp_amd_plan_execute_dev(p._h, P(d_in), P(t[0]), P(t[1]), P(d_out), P(t[2]), P(t[3]), P(d_len), P(d_st)) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_plan_execute(dev._h, P(d_in), P(d_out), P(d_len), P(d_st)) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_plan_execute_size(dev._h, P(d_in), P(d_len), P(d_need), P(d_st)) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_plan_execute_dev(dev._h, P(d_in), None, P(t[1]), P(d_out), P(t[2]), P(t[3]), P(d_len), P(d_st)) == m.MSCOMP_ARG_ERROR
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == GUARD).all() and (d_st.cpu().numpy() == 77).all()
    assert (d_len.cpu().numpy() == 5).all() and (d_need.cpu().numpy() == 5).all()
    for p in (host_d, host_c, size, dev):
        p.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_dev_plan_in_a_captured_graph(oracle, gpu_ctx, fmt):
    """execute_dev captured with torch.cuda.graph on the single stream of its context; input bytes and tables rewritten in place, the graph
    replayed: each result is that of a host plan"""
    import torch
    import ms_compress_amd as m
    f = FMTS[fmt]
    streams = cases.decode_streams(f, lambda d: oracle.oracle_compress(f, d)[1], n_corrupt=20)
    rnd = np.random.default_rng(8)
    n = 96
    batches = []
    for _ in range(3):
        pick = rnd.choice(len(streams), n, replace=False)
        batches.append(_layout([streams[i][0] for i in pick], [streams[i][1] for i in pick]))
    s = torch.cuda.Stream()
    ctx = m.Context(stream=s)
    with torch.cuda.stream(s):
        r = DevRun(ctx, f, n, max(len(x[0]) for x in batches), max(x[5] for x in batches) + 4096,
                   max(int(x[2].sum()) for x in batches), max(int(x[4].sum()) for x in batches))
        r.load(*batches[0][:5])
        r.execute()                                                   # (once outside the capture)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        r.execute()
    for blob, in_off, lens, out_off, caps, out_total in batches[1:] + batches[:1]:
        with torch.cuda.stream(s):
            r.load(blob, in_off, lens, out_off, caps)
            r.d_st.fill_(77)
            g.replay()
        s.synchronize()
        _same(_host(gpu_ctx, f, blob, in_off, lens, out_off, caps, out_total), r.result(), out_off, caps, out_total)
    del g
    r.plan.close()
    ctx.close()
