"""GPU: decompress plans with device tables (mscomp_amd_plan_create_decompress_dev / mscomp_amd_plan_execute_dev, api.DevPlan) and
mscomp_amd_layout_dev (api.layout_dev), against host-table decompress plans on the same units."""
import ctypes as C

import numpy as np
import pytest

import cases
import plans_rig as PR
from plans_rig import FMTS, GUARD

pytestmark = pytest.mark.gpu
SIZES = (65536, 700 << 10, 3 << 20)


@pytest.mark.parametrize("fmt", list(FMTS))
def test_dev_plan_matches_host_plan(oracle, gpu_ctx, fmt):
    """the decode families (valid, cut, concatenated, corrupted streams at their capacities) and corpus units of 64 KiB, 700 KiB and 3 MB,
    where host plans take their optional paths: status, length and bytes as a host plan's; nothing written outside the capacities"""
    import ms_compress_amd as m
    f = FMTS[fmt]
    streams = cases.decode_streams(f, lambda d: oracle.oracle_compress(f, d)[1])
    plain, comp = PR.corpus_streams(f, SIZES)
    units = [s for s, _ in streams] + comp
    caps = [c for _, c in streams] + [len(p) for p in plain]
    batch = PR.layout(units, caps)
    blob, in_off, lens, out_off, caps, out_total = batch
    host = PR.host_run(gpu_ctx, f, batch, "decode")
    r = PR.DevRun(m.DevPlan(gpu_ctx, f, len(units), int(lens.sum()), int(caps.sum())), len(blob), out_total + 4096)
    r.load(batch)
    r.execute()
    dev = r.result()
    PR.same(host, dev, batch)
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
        batches.append(PR.layout(units, caps))
    in_max = max(int(x[2].sum()) for x in batches)
    out_max = max(int(x[4].sum()) for x in batches)
    r = PR.DevRun(m.DevPlan(gpu_ctx, f, n, in_max, out_max), max(len(x[0]) for x in batches), max(x[5] for x in batches) + 4096)
    for batch in batches:
        r.load(batch)
        r.execute()
        dev = r.result()
        PR.same(PR.host_run(gpu_ctx, f, batch, "decode"), dev, batch)


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
    blob, in_off, lens, _, _, _ = PR.layout(plain, [0] * n)
    cap = [m.max_compressed_size(f, len(u)) + 2 for u in plain]
    c_off, c_total = m.pack_offsets(cap)
    d_plain = torch.from_numpy(blob).cuda()
    d_comp = torch.zeros(c_total + 16, dtype=torch.uint8, device="cuda")
    d_clen = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_cst = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_plain_off, d_plain_len = PR.dt(in_off), PR.dt(lens)
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
    import ms_compress_amd as m
    f = FMTS[fmt]
    streams = [s for s in cases.decode_streams(f, lambda d: oracle.oracle_compress(f, d)[1], n_corrupt=0) if len(s[0]) > 8 and s[1] > 8][::7][:40]
    units, caps = [s for s, _ in streams], [c for _, c in streams]
    n = len(units)
    batch = PR.layout(units, caps)
    blob, in_off, lens, out_off, caps, out_total = batch
    host = PR.host_run(gpu_ctx, f, batch, "decode")
    big = 0xFFFFF000 + 1
    # the unit with the long in_len spans an input buffer that really is that long (zeros), its capacity is small
    r = PR.DevRun(m.DevPlan(gpu_ctx, f, n, big + int(lens.sum()), int(caps.sum())), big + len(blob) + 64, out_total + 4096)
    lens_bad = lens.copy()
    lens_bad[3] = big
    in_off_bad = in_off.copy()
    in_off_bad[3] = 0
    r.load(batch._replace(in_off=in_off_bad, lens=lens_bad))
    r.execute()
    acc = np.ones(n, bool)
    acc[3] = False
    PR.same(host, r.result(), batch, acc)

    for in_cut, out_cut in ((n // 2, None), (None, 2 * n // 3), (n // 4, n // 3)):
        in_max = int(lens[: in_cut].sum()) + int(lens[in_cut]) // 2 if in_cut is not None else int(lens.sum())
        out_max = int(caps[: out_cut].sum()) + int(caps[out_cut]) // 2 if out_cut is not None else int(caps.sum())
        lim = min(x for x in (in_cut, out_cut, n) if x is not None)
        r = PR.DevRun(m.DevPlan(gpu_ctx, f, n, in_max, out_max), len(blob), out_total + 4096)
        r.load(batch)
        r.execute()
        PR.same(host, r.result(), batch, np.arange(n) < lim)
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
    t = [PR.dt(off), PR.dt(ln), PR.dt(off), PR.dt(ln)]
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
        batches.append(PR.layout([streams[i][0] for i in pick], [streams[i][1] for i in pick]))
    s = torch.cuda.Stream()
    ctx = m.Context(stream=s)
    with torch.cuda.stream(s):
        r = PR.DevRun(m.DevPlan(ctx, f, n, max(int(x[2].sum()) for x in batches), max(int(x[4].sum()) for x in batches)),
                      max(len(x[0]) for x in batches), max(x[5] for x in batches) + 4096)
        r.load(batches[0])
        r.execute()                                                   # (once outside the capture)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        r.execute()
    for batch in batches[1:] + batches[:1]:
        with torch.cuda.stream(s):
            r.load(batch)
            g.replay()
        s.synchronize()
        PR.same(PR.host_run(gpu_ctx, f, batch, "decode"), r.result(), batch)
    del g
    r.plan.close()
    ctx.close()
