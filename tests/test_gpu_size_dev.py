"""GPU: size plans with device tables (mscomp_amd_plan_create_size_dev / mscomp_amd_plan_execute_size_dev, api.SizeDevPlan) against
host-table size plans (api.SizePlan) on the same offsets, lengths and limits."""
import ctypes as C

import numpy as np
import pytest

import cases
import plans_rig as PR
from plans_rig import FMTS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fmt", list(FMTS))
def test_size_dev_plan_matches_host_size_plan(oracle, gpu_ctx, fmt):
    """the decode families (valid, cut, concatenated, corrupted streams) with an empty and a 1-byte unit, as one batch: with the capacities as
    limits and without limits, status, length and need are those of a host size plan, entry for entry"""
    f = FMTS[fmt]
    streams = cases.decode_streams(f, lambda d: oracle.oracle_compress(f, d)[1])
    units = [s for s, _ in streams] + [b"", b"\x00", b"\x41"]
    caps = np.array([c for _, c in streams] + [0, 5, 5], np.uint64)
    import ms_compress_amd as m
    batch = PR.layout(units, caps)
    r = PR.DevRun(m.SizeDevPlan(gpu_ctx, f, len(units), int(batch.lens.sum())), len(batch.blob), 0)
    for b in (batch, batch._replace(caps=None)):
        host = PR.host_run(gpu_ctx, f, b, "size")
        r.load(b)
        r.execute(limited=b.caps is not None)
        dev = r.result()
        PR.same_sizes(host, dev)
        assert sum(int(s) == 0 for s in dev[1]) > 50
        if f == 2:                                                  # streams that end in the End_of_buffer header need one byte more than they give
            plus = [i for i in range(len(units)) if dev[1][i] == 0 and dev[3][i] == dev[0][i] + 1]
            assert plus and all(units[i].endswith(b"\0\0") for i in plus)
    r.plan.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_one_size_dev_plan_several_batches(oracle, gpu_ctx, fmt):
    """one plan of 120 units, five batches of 90 to 110 live units (the rest have in_len 0), tables and bytes rewritten in place on the device
    (from the second execution on the plan's own graph is replayed): each result is that of a fresh host size plan"""
    import ms_compress_amd as m
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
        batches.append(PR.layout(units, limits))
    r = PR.DevRun(m.SizeDevPlan(gpu_ctx, f, n, max(int(x[2].sum()) for x in batches)), max(len(x[0]) for x in batches), 0)
    for batch in batches:
        r.load(batch)
        r.execute()
        PR.same_sizes(PR.host_run(gpu_ctx, f, batch, "size"), r.result())
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
    batch = PR.layout(units, caps)
    blob, in_off, lens, out_off, caps, _ = batch
    host = PR.host_run(gpu_ctx, f, batch, "size")
    big = 0xFFFFF000 + 1
    ctx = m.Context()                                               # (its scratch for 4 GiB of input goes away with it)
    r = PR.DevRun(m.SizeDevPlan(ctx, f, n, big + int(lens.sum())), len(blob), 0)
    lens_bad = lens.copy()
    lens_bad[3] = big
    r.load(batch._replace(lens=lens_bad))
    r.execute()
    acc = np.ones(n, bool)
    acc[3] = False
    PR.same_sizes(host, r.result(), acc)
    r.plan.close()
    del r
    torch.cuda.synchronize()
    ctx.close()

    for cut in (n // 2, n // 4, 0):
        in_max = int(lens[:cut].sum()) + int(lens[cut]) // 2
        r = PR.DevRun(m.SizeDevPlan(gpu_ctx, f, n, in_max), len(blob), 0)
        r.load(batch)
        r.execute()
        PR.same_sizes(host, r.result(), np.arange(n) < cut)
        r.plan.close()

    r = PR.DevRun(m.SizeDevPlan(gpu_ctx, f, 1, int(lens[5])), len(blob), 0)      # one unit
    r.load(batch._replace(in_off=in_off[5:6], lens=lens[5:6], out_off=out_off[5:6], caps=caps[5:6]))
    r.execute()
    PR.same_sizes(tuple(x[5:6] for x in host), r.result())
    r.plan.close()
    r = PR.DevRun(m.SizeDevPlan(gpu_ctx, f, 0, 0), 16, 0)            # no unit: nothing is enqueued, nothing written
    r.execute()
    assert len(r.result()[1]) == 0
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
    batch = PR.layout(comp)
    host = PR.host_run(gpu_ctx, f, batch, "size")
    modes = (C.c_uint32 * 8)()
    if f == 3:                                                      # the host plan took the segment path for the large stream ...
        assert gpu_ctx.lib.mscomp_amd_debug_decode_modes(gpu_ctx._h, modes, 8) == 1 and modes[0] == 2
    r = PR.DevRun(m.SizeDevPlan(gpu_ctx, f, len(comp), int(batch.lens.sum())), len(batch.blob), 0)
    r.load(batch)
    r.execute(limited=False)
    dev = r.result()
    if f == 3:                                                      # ... and the dev plan has no such path
        assert gpu_ctx.lib.mscomp_amd_debug_decode_modes(gpu_ctx._h, modes, 8) == 0
    PR.same_sizes(host, dev)
    assert (dev[1] == 0).all() and [int(x) for x in dev[0]] == [len(p) for p in plain] and (dev[3] == dev[0]).all()
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
    t = [PR.dt(off), PR.dt(ln), PR.dt(off), PR.dt(ln)]
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
