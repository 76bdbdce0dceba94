"""GPU: compress plans with device tables (mscomp_amd_plan_create_compress_dev executed by mscomp_amd_plan_execute_dev, api.CompressDevPlan)
and mscomp_amd_plan_layout_dev (api.plan_layout_dev), against fresh host-table compress plans on the same units."""
import ctypes as C
import random

import numpy as np
import pytest

import cases
import plans_rig as PR
from plans_rig import FMTS, GUARD

pytestmark = pytest.mark.gpu


def _exact(ctx, f, units):
    """the exact compressed length of every unit (a host plan at the largest capacity)"""
    import ms_compress_amd as m
    caps = [m.max_compressed_size(f, len(u)) + 2 for u in units]
    hl, hs, _ = PR.host_run(ctx, f, PR.layout(units, caps), "compress")
    assert (hs == 0).all()
    return [int(x) for x in hl]


def _cap_variants(f, n, exact):
    import ms_compress_amd as m
    v = [m.max_compressed_size(f, n) + (2 if f == 2 else 0), exact, max(0, exact - 1)]
    return v + ([exact + 1, exact + 2] if f == 2 else [])


def _with_caps(ctx, f, units, every):
    """(units, caps): the capacities cycle through the largest, the exact one, one short (and exact + 1 / + 2 for LZNT1); the units in
    `every` are repeated with each of them"""
    ex = _exact(ctx, f, units)
    out_u, out_c = [], []
    for i, u in enumerate(units):
        vs = _cap_variants(f, len(u), ex[i])
        for k, c in enumerate(vs):
            if i in every or k == i % len(vs):
                out_u.append(u)
                out_c.append(c)
    return out_u, out_c


def _check(ctx, f, units, caps, unit_max, in_max=None):
    import torch
    import ms_compress_amd as m
    batch = PR.layout(units, caps)
    host = PR.host_run(ctx, f, batch, "compress")
    plan = m.CompressDevPlan(ctx, f, len(units), int(batch.lens.sum()) if in_max is None else in_max, unit_max)
    r = PR.DevRun(plan, len(batch.blob), batch.out_total + 4096)
    r.load(batch)
    r.execute()
    dev = r.result()
    PR.same(host, dev, batch, tail=2)
    r.plan.close()
    del r
    torch.cuda.synchronize()
    return dev


CORPUS_SIZES = (0, 1, 4095, 4097, 65535, 65536, 65537, 700 << 10, 3 << 20)


@pytest.mark.parametrize("fmt", list(FMTS))
def test_compress_dev_plan_matches_host_plan(gpu_ctx, fmt):
    """edge-case families and corpus units from 0 bytes to 3 MB, at the largest, the exact and one byte short of the exact capacity (and
    exact + 1 / + 2 for LZNT1's terminator): status, length and bytes as a fresh host plan's, nothing written outside the capacities. Once
    with in_unit_max = 64 KiB on the units up to 64 KiB (the lazy Xpress finder), once with in_unit_max = 3 MB on all of them."""
    f = FMTS[fmt]
    edge = cases.edge_cases()
    corp = PR.corpus_units(CORPUS_SIZES)
    units = edge + corp
    every = set(range(len(edge), len(units)))
    small = [u for u in units if len(u) <= 65536]
    small_every = set(i for i, u in enumerate(small) if i >= len([e for e in edge if len(e) <= 65536]))
    u, c = _with_caps(gpu_ctx, f, small, small_every)
    st = _check(gpu_ctx, f, u, c, 65536)[1]
    assert (st == 0).sum() > 100 and (st == -5).sum() > 50
    u, c = _with_caps(gpu_ctx, f, units, every)
    st = _check(gpu_ctx, f, u, c, 3 << 20)[1]
    assert (st == 0).sum() > 100 and (st == -5).sum() > 50


@pytest.mark.parametrize("shape", ["few_long", "300x64k", "1500_mixed"])
def test_xpress_emit_modes_by_batch_shape(gpu_ctx, shape):
    """Xpress: the emit kernels a dev plan takes follow its unit count and chunk bound -- a few long units (a block per super-block),
    300 units of 64 KiB (four waves per unit), 1500 units of 4 to 64 KiB (one wave per unit); each equals a host plan"""
    import ms_compress_amd as m
    f = 3
    rnd = random.Random(17)
    if shape == "few_long":
        units, unit_max = PR.corpus_units((700 << 10, 3 << 20, 1 << 20, 200_000)), 3 << 20
    elif shape == "300x64k":
        units, unit_max = PR.corpus_units((65536,) * 300), 65536
    else:
        units, unit_max = PR.corpus_units(tuple(rnd.randint(4096, 65536) for _ in range(1500))), 65536
    caps = [m.max_compressed_size(f, len(u)) for u in units]
    st = _check(gpu_ctx, f, units, caps, unit_max)[1]
    assert (st == 0).all()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_one_compress_dev_plan_several_batches(gpu_ctx, fmt):
    """one plan, three batches of the same unit count with other units, lengths, capacities and offsets, tables and input rewritten in
    place (the second and third executions replay the plan's own graph): each result is that of a fresh host plan"""
    import ms_compress_amd as m
    f = FMTS[fmt]
    pool = cases.edge_cases(seed=4) + PR.corpus_units((65536, 100_000, 131072))
    rnd = np.random.default_rng(3)
    n = 150
    batches = []
    for b in range(3):
        pick = rnd.choice(len(pool), n, replace=False)
        units = [pool[i] for i in pick]
        caps = [m.max_compressed_size(f, len(u)) - int(rnd.integers(0, 40)) * b for u in units]
        batches.append(PR.layout(units, [max(0, c) for c in caps]))
    in_max = max(int(x[2].sum()) for x in batches)
    r = PR.DevRun(m.CompressDevPlan(gpu_ctx, f, n, in_max, max(len(u) for u in pool)), max(len(x[0]) for x in batches), max(x[5] for x in batches) + 4096)
    for batch in batches:
        r.load(batch)
        r.execute()
        dev = r.result()
        PR.same(PR.host_run(gpu_ctx, f, batch, "compress"), dev, batch, tail=2)
    r.plan.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_units_past_the_bounds_are_refused(gpu_ctx, fmt):
    """an in_len above in_unit_max in the middle of the batch, and a running total of in_len that crosses in_total_max partway: those units
    get MSCOMP_ARG_ERROR with length 0, the others compress as with a host plan, nothing is written outside the accepted capacities"""
    import ms_compress_amd as m
    f = FMTS[fmt]
    units = [u for u in cases.edge_cases(seed=6) if 8 < len(u) <= 65536][::5][:40] + PR.corpus_units((30_000, 65536, 70_000))
    n = len(units)
    caps = [m.max_compressed_size(f, len(u)) + 2 for u in units]
    batch = PR.layout(units, caps)
    blob, in_off, lens, out_off, caps, out_total = batch
    host = PR.host_run(gpu_ctx, f, batch, "compress")
    unit_max = 65536
    acc = lens <= unit_max
    assert not acc[-1] and acc[:-1].all()
    mid = n // 2                                                      # a long in_len in the middle, over the input of the units behind it
    lens_bad = lens.copy()
    lens_bad[mid] = unit_max + 1
    r = PR.DevRun(m.CompressDevPlan(gpu_ctx, f, n, int(lens_bad.sum()), unit_max), len(blob) + unit_max, out_total + 4096)
    r.load(batch._replace(lens=lens_bad))
    r.execute()
    a = acc.copy()
    a[mid] = False
    PR.same(host, r.result(), batch, a, tail=2)
    r.plan.close()
    cut = 3 * n // 4                                                  # in_total_max crossed inside unit `cut`
    in_max = int(lens[:cut].sum()) + int(lens[cut]) // 2
    r = PR.DevRun(m.CompressDevPlan(gpu_ctx, f, n, in_max, unit_max), len(blob), out_total + 4096)
    r.load(batch)
    r.execute()
    PR.same(host, r.result(), batch, acc & (np.cumsum(lens) <= in_max), tail=2)
    r.plan.close()


def test_lznt1_suffix_array_flavour(gpu_ctx):
    """a plan created in a context with the suffix-array dictionary compresses as a host plan of that context"""
    import ms_compress_amd as m
    ctx = m.Context()
    ctx.set_lznt1_sa_dict(True)
    units = cases.edge_cases(seed=7)[::3] + PR.corpus_units((0, 4097, 65537, 300_000))
    u, c = _with_caps(ctx, 2, units, set(range(len(units) - 4, len(units))))
    _check(ctx, 2, u, c, 300_000)
    ctx.close()


def test_plan_kinds_are_kept_apart(gpu_ctx):
    """execute / execute_size refuse a compress dev plan, execute_dev still refuses host plans; nothing is written"""
    import torch
    import ms_compress_amd as m
    lib = m.load_library()
    n = 2
    off = np.array([0, 16], np.uint64)
    ln = np.array([10, 10], np.uint64)
    host_c = m.Plan(gpu_ctx, 2, off, ln, off, np.array([20, 20], np.uint64))
    host_d = m.Plan(gpu_ctx, 2, off, ln, off, ln, decompress=True)
    dev = m.CompressDevPlan(gpu_ctx, 2, n, 64, 32)
    d_in = torch.zeros(64, dtype=torch.uint8, device="cuda")
    d_out = torch.full((64,), GUARD, dtype=torch.uint8, device="cuda")
    t = [PR.dt(off), PR.dt(ln), PR.dt(off), PR.dt(ln)]
    d_len = torch.full((n,), 5, dtype=torch.int64, device="cuda")
    d_need = torch.full((n,), 5, dtype=torch.int64, device="cuda")
    d_st = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    P = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    assert lib.mscomp_amd_plan_execute(dev._h, P(d_in), P(d_out), P(d_len), P(d_st)) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_plan_execute_size(dev._h, P(d_in), P(d_len), P(d_need), P(d_st)) == m.MSCOMP_ARG_ERROR
    for p in (host_c, host_d):
        assert lib.mscomp_amd_plan_execute_dev(p._h, P(d_in), P(t[0]), P(t[1]), P(d_out), P(t[2]), P(t[3]), P(d_len), P(d_st)) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_plan_execute_dev(dev._h, P(d_in), P(t[0]), P(t[1]), None, P(t[2]), P(t[3]), P(d_len), P(d_st)) == m.MSCOMP_ARG_ERROR
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == GUARD).all() and (d_st.cpu().numpy() == 77).all()
    assert (d_len.cpu().numpy() == 5).all() and (d_need.cpu().numpy() == 5).all()
    for p in (host_c, host_d, dev):
        p.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_compress_dev_plan_in_a_captured_graph(gpu_ctx, fmt):
    """execute_dev captured with torch.cuda.graph on the single stream of its context -- its first execution, so the kernels' one-time
    attributes must come from plan creation -- then input and tables rewritten in place and the graph replayed over three batches: each
    result is that of a host plan (Xpress+Huffman included: its fallback counter is zeroed by a kernel, not a memset)"""
    import torch
    import ms_compress_amd as m
    f = FMTS[fmt]
    pool = cases.edge_cases(seed=8) + PR.corpus_units((65536, 65537, 200_000))
    rnd = np.random.default_rng(8)
    n = 96
    batches = []
    for b in range(3):
        pick = rnd.choice(len(pool), n, replace=False)
        units = [pool[i] for i in pick]
        batches.append(PR.layout(units, [max(0, m.max_compressed_size(f, len(u)) - 30 * b) for u in units]))
    s = torch.cuda.Stream()
    ctx = m.Context(stream=s)
    with torch.cuda.stream(s):
        r = PR.DevRun(m.CompressDevPlan(ctx, f, n, max(int(x[2].sum()) for x in batches), 200_000),
                      max(len(x[0]) for x in batches), max(x[5] for x in batches) + 4096)
        r.load(batches[0])
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        r.execute()
    for batch in batches:
        with torch.cuda.stream(s):
            r.load(batch)
            g.replay()
        s.synchronize()
        PR.same(PR.host_run(gpu_ctx, f, batch, "compress"), r.result(), batch, tail=2)
    del g
    r.plan.close()
    ctx.close()


def test_transcode_lznt1_to_xpress_huff_on_the_device(gpu_ctx):
    """LZNT1 streams -> decompress dev plan -> plan_layout_dev(Xpress+Huffman, d_out_len) -> compress dev plan (in_off = the decode offsets,
    in_len = d_out_len) -> decompress dev plan again, with no host copy between the stages: the final bytes are the plain units, the
    compressed ones those of a host compress of the plain units"""
    import torch
    import ms_compress_amd as m
    plain = PR.corpus_units(CORPUS_SIZES[1:7] + (300_000,)) + [bytes(5000), b"abc" * 999]
    n = len(plain)
    comp, st = m.compress_units(2, plain)
    assert all(s == 0 for s in st)
    ref, st = m.compress_units(4, plain)
    assert all(s == 0 for s in st)
    c_off, c_total = m.pack_offsets([len(c) for c in comp])
    p_off, p_total = m.pack_offsets([len(p) for p in plain])
    blob = np.zeros(c_total + 16, np.uint8)
    for c, o in zip(comp, c_off):
        blob[int(o): int(o) + len(c)] = np.frombuffer(c, np.uint8)
    d_comp, d_coff, d_clen = torch.from_numpy(blob).cuda(), PR.dt(c_off), PR.dt([len(c) for c in comp])
    d_poff, d_pcap = PR.dt(p_off), PR.dt([len(p) for p in plain])
    plain_total = sum(len(p) for p in plain)
    x_total = sum(m.max_compressed_size(4, len(p)) for p in plain) + 16 * n + 64
    d_plain = torch.full((p_total + 64,), GUARD, dtype=torch.uint8, device="cuda")
    d_x = torch.full((x_total,), GUARD, dtype=torch.uint8, device="cuda")
    d_back = torch.full((p_total + 64,), GUARD, dtype=torch.uint8, device="cuda")
    lens = [torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(3)]
    sts = [torch.full((n,), 77, dtype=torch.int32, device="cuda") for _ in range(3)]
    dec1 = m.DevPlan(gpu_ctx, 2, n, c_total, p_total)
    enc = m.CompressDevPlan(gpu_ctx, 4, n, plain_total, max(len(p) for p in plain))
    dec2 = m.DevPlan(gpu_ctx, 4, n, x_total, p_total)
    torch.cuda.synchronize()
    dec1.execute(d_comp, d_coff, d_clen, d_plain, d_poff, d_pcap, lens[0], sts[0])
    d_xoff, d_xcap = m.plan_layout_dev(gpu_ctx, 4, lens[0], 16)
    enc.execute(d_plain, d_poff, lens[0], d_x, d_xoff, d_xcap, lens[1], sts[1])
    dec2.execute(d_x, d_xoff, lens[1], d_back, d_poff, lens[0], lens[2], sts[2])
    torch.cuda.synchronize()
    for s in sts:
        assert (s.cpu().numpy() == 0).all()
    xl, xo, xb = lens[1].cpu().numpy(), d_xoff.cpu().numpy(), d_x.cpu().numpy()
    back, bl = d_back.cpu().numpy(), lens[2].cpu().numpy()
    for i, p in enumerate(plain):
        o = int(xo[i])
        assert int(xl[i]) == len(ref[i]) and bytes(xb[o: o + len(ref[i])]) == ref[i], i
        o = int(p_off[i])
        assert int(bl[i]) == len(p) and bytes(back[o: o + len(p)]) == p, i
    for p in (dec1, enc, dec2):
        p.close()


@pytest.mark.parametrize("align", [1, 16, 4096])
@pytest.mark.parametrize("fmt", list(FMTS))
def test_plan_layout_dev_matches_host_layout(gpu_ctx, fmt, align):
    """plan_layout_dev equals the host mscomp_amd_plan_layout for random lengths, 0, 1 and 2^32 + 5 among them"""
    import torch
    import ms_compress_amd as m
    f = FMTS[fmt]
    lib = m.load_library()
    rnd = np.random.default_rng(align + f)
    lens = np.concatenate([np.array([0, 1, (1 << 32) + 5, 4096, 65536], np.uint64),
                           rnd.integers(0, 1 << 22, 3000, dtype=np.uint64)])
    rnd.shuffle(lens)
    n = len(lens)
    off = np.zeros(n, np.uint64)
    cap = np.zeros(n, np.uint64)
    total = lib.mscomp_amd_plan_layout(f, n, lens.ctypes.data, align, off.ctypes.data, cap.ctypes.data)
    d_off, d_cap = m.plan_layout_dev(gpu_ctx, f, PR.dt(lens), align)
    torch.cuda.synchronize()
    got_off, got_cap = d_off.cpu().numpy().view(np.uint64), d_cap.cpu().numpy().view(np.uint64)
    assert (got_cap == cap).all() and (got_off[:n] == off).all() and int(got_off[n]) == int(total)
    d_off2 = torch.zeros(n + 1, dtype=torch.int64, device="cuda")    # d_out_cap may be NULL
    assert lib.mscomp_amd_plan_layout_dev(gpu_ctx._h, f, n, C.c_void_p(PR.dt(lens).data_ptr()), align, C.c_void_p(d_off2.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert (d_off2.cpu().numpy().view(np.uint64) == got_off).all()
