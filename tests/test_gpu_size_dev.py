"""GPU: size plans with device tables (mscomp_amd_plan_create_size_dev / mscomp_amd_plan_execute_size_dev, api.SizeDevPlan) against
host-table size plans (api.SizePlan) on the same offsets, lengths and limits."""
import ctypes as C

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
FMTS = {"lznt1": 2, "xpress": 3, "xpress_huff": 4}
PAD = 8                                                              # guard entries in front of and behind every result array
G_LEN, G_ST = 0x5A5A5A5A5A5A5A5A, 77
ARG = -2


def _dt(a):
    """a uint64 host table as an int64 CUDA tensor"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.uint64)).view(np.int64).copy()).cuda()


def _pack(units):
    import ms_compress_amd as m
    lens = [len(u) for u in units]
    in_off, in_total = m.pack_offsets(lens)
    blob = np.zeros(in_total + 16, np.uint8)
    for u, o in zip(units, in_off):
        blob[int(o): int(o) + len(u)] = np.frombuffer(bytes(u), np.uint8)
    return blob, in_off, np.array(lens, np.uint64)


def _host(ctx, f, blob, in_off, lens, limits):
    """a fresh host-table size plan: (out_len, need, status)"""
    import torch
    import ms_compress_amd as m
    n = len(lens)
    d_in = torch.from_numpy(blob).cuda()
    d_len = torch.zeros(max(1, n), dtype=torch.int64, device="cuda")
    d_need = torch.zeros(max(1, n), dtype=torch.int64, device="cuda")
    d_st = torch.zeros(max(1, n), dtype=torch.int32, device="cuda")
    plan = m.SizePlan(ctx, f, in_off, lens, limits)
    plan.execute(d_in, d_len, d_need, d_st)
    torch.cuda.synchronize()
    plan.close()
    return d_len.cpu().numpy()[:n].view(np.uint64), d_need.cpu().numpy()[:n].view(np.uint64), d_st.cpu().numpy()[:n]


class SizeRun:
    """one size dev plan and the device buffers of its batches: tables and bytes are rewritten in place between executions; the three
    result arrays sit between guard entries"""

    def __init__(self, ctx, f, n, in_bytes, in_max):
        import torch
        import ms_compress_amd as m
        self.plan = m.SizeDevPlan(ctx, f, n, in_max)
        self.n = n
        self.d_in = torch.zeros(max(16, in_bytes), dtype=torch.uint8, device="cuda")
        self.tabs = [torch.zeros(max(1, n), dtype=torch.int64, device="cuda") for _ in range(3)]
        self.d_len = torch.full((n + 2 * PAD,), G_LEN, dtype=torch.int64, device="cuda")
        self.d_need = torch.full((n + 2 * PAD,), G_LEN, dtype=torch.int64, device="cuda")
        self.d_st = torch.full((n + 2 * PAD,), G_ST, dtype=torch.int32, device="cuda")

    def load(self, blob, in_off, lens, limits=None):
        import torch
        self.d_in[: len(blob)].copy_(torch.from_numpy(blob))
        for t, a in zip(self.tabs, (in_off, lens, limits)):
            if a is not None:
                t[: self.n].copy_(_dt(a))
        for t, v in ((self.d_len, G_LEN), (self.d_need, G_LEN), (self.d_st, G_ST)):
            t.fill_(v)

    def execute(self, limited=True):
        n = self.n
        self.plan.execute(self.d_in, self.tabs[0], self.tabs[1], self.d_len[PAD: PAD + n], self.d_need[PAD: PAD + n], self.d_st[PAD: PAD + n],
                          self.tabs[2] if limited else None)

    def result(self):
        """(out_len, need, status) of the n units; the guard entries around them must be untouched"""
        import torch
        torch.cuda.synchronize()
        n = self.n
        ln, need, st = self.d_len.cpu().numpy(), self.d_need.cpu().numpy(), self.d_st.cpu().numpy()
        for a, v in ((ln, G_LEN), (need, G_LEN), (st, G_ST)):
            assert (a[:PAD] == v).all() and (a[PAD + n:] == v).all(), "guard entries overwritten"
        return ln[PAD: PAD + n].view(np.uint64), need[PAD: PAD + n].view(np.uint64), st[PAD: PAD + n]


def _same(host, dev, accepted=None):
    hl, hn, hs = host
    dl, dn, ds = dev
    for i in range(len(hs)):
        if accepted is not None and not accepted[i]:
            assert (ds[i], dl[i], dn[i]) == (ARG, 0, 0), (i, ds[i], dl[i], dn[i])
            continue
        assert (ds[i], dl[i], dn[i]) == (hs[i], hl[i], hn[i]), (i, ds[i], hs[i], dl[i], hl[i], dn[i], hn[i])


@pytest.mark.parametrize("fmt", list(FMTS))
def test_size_dev_plan_matches_host_size_plan(oracle, gpu_ctx, fmt):
    """the decode families (valid, cut, concatenated, corrupted streams) with an empty and a 1-byte unit, as one batch: with the capacities as
    limits and without limits, status, length and need are those of a host size plan, entry for entry"""
    f = FMTS[fmt]
    streams = cases.decode_streams(f, lambda d: oracle.oracle_compress(f, d)[1])
    units = [s for s, _ in streams] + [b"", b"\x00", b"\x41"]
    caps = np.array([c for _, c in streams] + [0, 5, 5], np.uint64)
    blob, in_off, lens = _pack(units)
    r = SizeRun(gpu_ctx, f, len(units), len(blob), int(lens.sum()))
    for limits in (caps, None):
        host = _host(gpu_ctx, f, blob, in_off, lens, limits)
        r.load(blob, in_off, lens, limits)
        r.execute(limited=limits is not None)
        dev = r.result()
        _same(host, dev)
        assert sum(int(s) == 0 for s in dev[2]) > 50
        if f == 2:                                                  # streams that end in the End_of_buffer header need one byte more than they give
            plus = [i for i in range(len(units)) if dev[2][i] == 0 and dev[1][i] == dev[0][i] + 1]
            assert plus and all(units[i].endswith(b"\0\0") for i in plus)
    r.plan.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_one_size_dev_plan_several_batches(oracle, gpu_ctx, fmt):
    """one plan of 120 units, five batches of 90 to 110 live units (the rest have in_len 0), tables and bytes rewritten in place on the device
    (from the second execution on the plan's own graph is replayed): each result is that of a fresh host size plan"""
    f = FMTS[fmt]
    streams = cases.decode_streams(f, lambda d: oracle.oracle_compress(f, d)[1], n_corrupt=20)
    rnd = np.random.default_rng(4)
    n = 120
    batches = []
    for b in range(5):
        live = 90 + 5 * b
        pick = rnd.choice(len(streams), live, replace=False)
        units = [streams[i][0] for i in pick] + [b""] * (n - live)
        limits = np.array([streams[i][1] + int(rnd.integers(0, 3)) * b for i in pick] + [0] * (n - live), np.uint64)
        batches.append(_pack(units) + (limits,))
    r = SizeRun(gpu_ctx, f, n, max(len(x[0]) for x in batches), max(int(x[2].sum()) for x in batches))
    for blob, in_off, lens, limits in batches:
        r.load(blob, in_off, lens, limits)
        r.execute()
        _same(_host(gpu_ctx, f, blob, in_off, lens, limits), r.result())
    r.plan.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_units_past_the_bounds_are_refused(oracle, gpu_ctx, fmt):
    """an in_len above 0xFFFFF000 (never read: the input buffer is nowhere near that long) and running totals that cross in_total_max
    partway: those units get MSCOMP_ARG_ERROR with length and need 0, their neighbours the host plan's results, and the entries around the
    three result arrays stay untouched. Plans of one unit and of none."""
    import torch
    import ms_compress_amd as m
    f = FMTS[fmt]
    streams = [s for s in cases.decode_streams(f, lambda d: oracle.oracle_compress(f, d)[1], n_corrupt=0) if len(s[0]) > 8 and s[1] > 8][::7][:40]
    units, caps = [s for s, _ in streams], np.array([c for _, c in streams], np.uint64)
    n = len(units)
    blob, in_off, lens = _pack(units)
    host = _host(gpu_ctx, f, blob, in_off, lens, caps)
    big = 0xFFFFF000 + 1
    ctx = m.Context()                                               # (its scratch for 4 GiB of input goes away with it)
    r = SizeRun(ctx, f, n, len(blob), big + int(lens.sum()))
    lens_bad = lens.copy()
    lens_bad[3] = big
    r.load(blob, in_off, lens_bad, caps)
    r.execute()
    acc = np.ones(n, bool)
    acc[3] = False
    _same(host, r.result(), acc)
    r.plan.close()
    del r
    torch.cuda.synchronize()
    ctx.close()

    for cut in (n // 2, n // 4, 0):
        in_max = int(lens[:cut].sum()) + int(lens[cut]) // 2
        r = SizeRun(gpu_ctx, f, n, len(blob), in_max)
        r.load(blob, in_off, lens, caps)
        r.execute()
        _same(host, r.result(), np.arange(n) < cut)
        r.plan.close()

    r = SizeRun(gpu_ctx, f, 1, len(blob), int(lens[5]))              # one unit
    r.load(blob, in_off[5:6], lens[5:6], caps[5:6])
    r.execute()
    _same(tuple(x[5:6] for x in host), r.result())
    r.plan.close()
    r = SizeRun(gpu_ctx, f, 0, 16, 0)                                # no unit: nothing is enqueued, nothing written
    r.execute()
    assert len(r.result()[2]) == 0
    r.plan.close()


@pytest.mark.parametrize("fmt", ["xpress", "xpress_huff"])
def test_large_units_among_small_ones(gpu_ctx, fmt):
    """one compressed unit of about 1 MB among 3000 small ones: the host size plan walks a large Xpress stream by segments, the dev plan by
    the one-wave walk (no segment table is built on the device), and both give the same answers. The one-wave walk is the slow path
    (DESIGN_DECODERS.md: 657 ms to decode a 27 MB stream, about 25 ms per MB), so the large unit stays near 1 MB and a run of this test
    belongs under a time limit of a minute or so."""
    import ms_compress_amd as m
    from ms_compress_amd import corpus
    f = FMTS[fmt]
    data = corpus.by_name("mozilla", 9_000_000).tobytes()
    want = 1_000_000
    big_plain = data[:2 * want]
    probe, st = m.compress_units(f, [big_plain], ctx=gpu_ctx)
    assert st[0] == 0
    big_plain = data[: int(len(big_plain) * want / len(probe[0]))]     # scaled so that the compressed unit is near 1 MB
    small = [data[3_000_000 + 2000 * i: 3_000_000 + 2000 * i + 1500 + (i % 7) * 70] for i in range(3000)]
    plain = small[:1500] + [big_plain] + small[1500:]
    comp, st = m.compress_units(f, plain, ctx=gpu_ctx)
    assert all(s == 0 for s in st)
    assert 800_000 < len(comp[1500]) < 1_300_000, len(comp[1500])
    blob, in_off, lens = _pack(comp)
    host = _host(gpu_ctx, f, blob, in_off, lens, None)
    modes = (C.c_uint32 * 8)()
    if f == 3:                                                      # the host plan took the segment path for the large stream ...
        assert gpu_ctx.lib.mscomp_amd_debug_decode_modes(gpu_ctx._h, modes, 8) == 1 and modes[0] == 2
    r = SizeRun(gpu_ctx, f, len(comp), len(blob), int(lens.sum()))
    r.load(blob, in_off, lens)
    r.execute(limited=False)
    dev = r.result()
    if f == 3:                                                      # ... and the dev plan has no such path
        assert gpu_ctx.lib.mscomp_amd_debug_decode_modes(gpu_ctx._h, modes, 8) == 0
    _same(host, dev)
    assert (dev[2] == 0).all() and [int(x) for x in dev[0]] == [len(p) for p in plain] and (dev[1] == dev[0]).all()
    r.plan.close()


def test_plan_kinds_are_kept_apart(gpu_ctx):
    """the four execute functions against the six kinds of plan: each runs its own kind only, returns MSCOMP_ARG_ERROR for the others and
    enqueues nothing for them"""
    import torch
    import ms_compress_amd as m
    lib = m.load_library()
    n = 2
    off = np.array([0, 16], np.uint64)
    ln = np.array([10, 10], np.uint64)
    plans = {"host_c": m.Plan(gpu_ctx, 2, off, ln, off, np.array([20, 20], np.uint64)),
             "host_d": m.Plan(gpu_ctx, 2, off, ln, off, ln, decompress=True),
             "host_s": m.SizePlan(gpu_ctx, 2, off, ln),
             "dev_d": m.DevPlan(gpu_ctx, 2, n, 64, 64),
             "dev_c": m.CompressDevPlan(gpu_ctx, 2, n, 64, 64),
             "dev_s": m.SizeDevPlan(gpu_ctx, 2, n, 64)}
    d_in = torch.zeros(64, dtype=torch.uint8, device="cuda")
    d_out = torch.full((64,), 0xEE, dtype=torch.uint8, device="cuda")
    t = [_dt(off), _dt(ln), _dt(off), _dt(ln)]
    d_len = torch.full((n,), 5, dtype=torch.int64, device="cuda")
    d_need = torch.full((n,), 5, dtype=torch.int64, device="cuda")
    d_st = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    P = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    calls = {"execute": lambda h: lib.mscomp_amd_plan_execute(h, P(d_in), P(d_out), P(d_len), P(d_st)),
             "execute_size": lambda h: lib.mscomp_amd_plan_execute_size(h, P(d_in), P(d_len), P(d_need), P(d_st)),
             "execute_dev": lambda h: lib.mscomp_amd_plan_execute_dev(h, P(d_in), P(t[0]), P(t[1]), P(d_out), P(t[2]), P(t[3]), P(d_len), P(d_st)),
             "execute_size_dev": lambda h: lib.mscomp_amd_plan_execute_size_dev(h, P(d_in), P(t[0]), P(t[1]), P(t[3]), P(d_len), P(d_need), P(d_st))}
    takes = {"execute": ("host_c", "host_d"), "execute_size": ("host_s",), "execute_dev": ("dev_d", "dev_c"), "execute_size_dev": ("dev_s",)}
    for name, call in calls.items():
        for kind, p in plans.items():
            if kind not in takes[name]:
                assert call(p._h) == m.MSCOMP_ARG_ERROR, (name, kind)
    h = plans["dev_s"]._h                                           # a null array
    assert lib.mscomp_amd_plan_execute_size_dev(h, P(d_in), None, P(t[1]), P(t[3]), P(d_len), P(d_need), P(d_st)) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_plan_execute_size_dev(h, P(d_in), P(t[0]), P(t[1]), P(t[3]), P(d_len), None, P(d_st)) == m.MSCOMP_ARG_ERROR
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0xEE).all() and (d_st.cpu().numpy() == 77).all()
    assert (d_len.cpu().numpy() == 5).all() and (d_need.cpu().numpy() == 5).all()
    for name, call in calls.items():                                # and each runs its own kind
        for kind in takes[name]:
            assert call(plans[kind]._h) == m.MSCOMP_OK, (name, kind)
    torch.cuda.synchronize()
    for p in plans.values():
        p.close()
