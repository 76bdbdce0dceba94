"""GPU: dev plans for batches with large units (MSCOMP_AMD_DEV_LARGE_UNITS: api.DevPlan / api.SizeDevPlan with large_units=True). The
segment table, the tables of the all-CU byte stage and the candidate token scratch are built on the device; the checker is a host plan on
the same tables (bytes, statuses, and the paths taken: mscomp_amd_debug_plan_paths), plus the oracle for the corpus units.

Every test asserts first that its large units are past the thresholds of the paths (512 KiB of compressed Xpress input, 1 MiB of
capacity). The largest unit is 12 MB: on a regression to the one-wave walk it still decodes in well under a second."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import plans_rig as PR
from plans_rig import FMTS, GUARD

pytestmark = pytest.mark.gpu
XFMTS = ["xpress", "xpress_huff"]
SIZES = (65536, 700 << 10, 3 << 20, 12 << 20)
_cache = {}


def _small(m, ctx, f, count):
    key = (f, "small", count)
    if key not in _cache:
        from ms_compress_amd import corpus
        data = corpus.by_name("mozilla", 40_000_000).tobytes()
        plain = [data[30_000_000 + 2000 * i: 30_000_000 + 2000 * i + 1500 + (i % 7) * 70] for i in range(count)]
        comp, st = m.compress_units(f, plain, ctx=ctx)
        assert all(s == 0 for s in st)
        _cache[key] = (plain, comp)
    return _cache[key]


def _mixed_batch(m, ctx, oracle, f, order=0):
    """the decode families and the corpus units (exact, one short, generous capacities), the large ones at places that depend on `order`"""
    plain, comp = PR.corpus_streams(f, SIZES, ctx)
    PR.assert_large(f, comp[2], len(plain[2]))
    PR.assert_large(f, comp[3], len(plain[3]))
    streams = cases.decode_streams(f, lambda d: oracle.oracle_compress(f, d)[1], n_corrupt=20)
    big = [(comp[0], len(plain[0])), (comp[1], len(plain[1])), (comp[2], len(plain[2])), (comp[3], len(plain[3])),
           (comp[2], len(plain[2]) - 1), (comp[2], len(plain[2]) + (1 << 20)), (comp[3], len(plain[3]) + 5000)]
    pairs = list(streams)
    step = max(1, len(pairs) // (len(big) + 1))
    for k, b in enumerate(big):
        pairs.insert(min(len(pairs), (k + order) * step + order), b)
    return pairs


@pytest.mark.parametrize("fmt", XFMTS)
def test_same_results_as_a_host_plan(oracle, gpu_ctx, fmt):
    """corpus units of 64 KiB, 700 KiB, 3 MB and 12 MB among the decode families (valid, cut, concatenated, corrupted streams), capacities
    exact, one short and generous: status, length, bytes on MSCOMP_OK as a host plan's and the oracle's; guard bytes outside every capacity
    untouched; the paths taken are the host plan's"""
    import ms_compress_amd as m
    f = FMTS[fmt]
    pairs = _mixed_batch(m, gpu_ctx, oracle, f)
    batch = PR.layout([s for s, _ in pairs], [c for _, c in pairs])
    blob, in_off, lens, out_off, caps, out_total = batch
    host, hpaths, _ = PR.host_run(gpu_ctx, f, batch, "decode", want_paths=True)
    r = PR.DevRun(m.DevPlan(gpu_ctx, f, len(pairs), int(lens.sum()), int(caps.sum()), large_units=True), len(blob), out_total + 4096)
    r.load(batch)
    r.execute()
    dev = r.result()
    PR.same(host, dev, batch)
    assert m.api.plan_paths(r.plan) == hpaths and hpaths[1] >= 4 and (f != 3 or hpaths[0] >= 4), (m.api.plan_paths(r.plan), hpaths)
    n_big = 0
    for i, (stream, cap) in enumerate(pairs):
        if cap >= 60000 and len(stream) > 30000:                    # the corpus units, against the oracle
            so, oo, undefined = oracle.oracle_decompress_ex(f, stream, cap)
            if undefined:                                           # (a corrupted stream of the families whose outcome the reference leaves open)
                continue
            assert dev[1][i] == so, (i, dev[1][i], so)
            assert so != 0 or bytes(dev[2][int(out_off[i]): int(out_off[i]) + int(dev[0][i])]) == oo, i
            n_big += 1
    assert n_big >= 7 and sum(int(s) == 0 for s in dev[1]) > 50
    r.plan.close()


def _one_large_among_small(m, ctx, f, count=3000):
    plain, comp = PR.corpus_streams(f, SIZES, ctx)
    sp, sc = _small(m, ctx, f, count)
    PR.assert_large(f, comp[3], len(plain[3]))
    units = sc[: count // 2] + [comp[3]] + sc[count // 2:]
    caps = [len(p) for p in sp[: count // 2]] + [len(plain[3])] + [len(p) for p in sp[count // 2:]]
    return units, caps, count // 2


@pytest.mark.parametrize("fmt", XFMTS)
def test_same_paths_as_a_host_plan(oracle, gpu_ctx, fmt):
    """mscomp_amd_debug_plan_paths gives the same triple for the dev plan and the host plan on (a) one 12 MB unit among 3 000 small ones,
    (b) 300 units of 1 MiB capacity (the all-CU stage does not pay), (c) small units only, (d) a unit with room for 0xFFFFFF00 bytes and
    more beside a 3 MB one (no all-CU stage). On (a) the segment walk reports mode 2 and the pointer passes leave their counters, as for a
    host plan; a plan created without the flag reports no path at all."""
    import torch
    import ms_compress_amd as m
    f = FMTS[fmt]
    plain, comp = PR.corpus_streams(f, SIZES, gpu_ctx)
    # (a)
    units, caps, at = _one_large_among_small(m, gpu_ctx, f)
    batch = PR.layout(units, caps)
    blob, in_off, lens, out_off, caps, out_total = batch
    host, hpaths, hmodes = PR.host_run(gpu_ctx, f, batch, "decode", want_paths=True)
    assert hpaths[0] == (1 if f == 3 else 0) and hpaths[1] == 1 and (f == 3 or hpaths[2] > 0), hpaths
    r = PR.DevRun(m.DevPlan(gpu_ctx, f, len(units), int(lens.sum()), int(caps.sum()), large_units=True), len(blob), out_total + 4096)
    r.load(batch)
    r.execute()
    dev = r.result()
    assert m.api.plan_paths(r.plan) == hpaths, (m.api.plan_paths(r.plan), hpaths)
    if f == 3:
        assert PR.decode_modes(gpu_ctx) == [2] and hmodes == [2]
    opened = (C.c_uint32 * 33)()
    gpu_ctx.lib.mscomp_amd_debug_lzg_open.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    assert gpu_ctx.lib.mscomp_amd_debug_lzg_open(gpu_ctx._h, int(caps[at]) + 64, opened) == 0
    opened = list(opened)
    assert opened[0] > 0 and 0 in opened and all(x == 0 for x in opened[opened.index(0):]), opened   # the path ran, took several passes, and ended
    PR.same(host, dev, batch)
    assert dev[1][at] == 0 and bytes(dev[2][int(out_off[at]): int(out_off[at]) + len(plain[3])]) == plain[3]
    r.plan.close()
    plainp = PR.DevRun(m.DevPlan(gpu_ctx, f, len(units), int(lens.sum()), int(caps.sum())), len(blob), out_total + 4096)
    plainp.load(batch)
    assert m.api.plan_paths(plainp.plan) == (0, 0, 0)
    plainp.plan.close()                                              # (not executed: the one-wave walk of 12 MB is what the flag is for)
    del r, plainp

    # (b) the same 1 MiB unit 300 times (one stream in the input, 300 outputs)
    one = plain[3][: 1 << 20]
    c1, st = m.compress_units(f, [one], ctx=gpu_ctx)
    assert st[0] == 0
    PR.assert_large(f, c1[0], len(one))
    n = 300
    blob = np.zeros(len(c1[0]) + 16, np.uint8)
    blob[: len(c1[0])] = np.frombuffer(c1[0], np.uint8)
    in_off, lens = np.zeros(n, np.uint64), np.full(n, len(c1[0]), np.uint64)
    caps = np.full(n, len(one), np.uint64)
    out_off = np.arange(n, dtype=np.uint64) * np.uint64(len(one) + 64) + np.uint64(64)
    out_total = int(out_off[-1]) + len(one) + 64
    d_in = torch.from_numpy(blob).cuda()
    h_out = torch.full((out_total,), GUARD, dtype=torch.uint8, device="cuda")
    h_len = torch.zeros(n, dtype=torch.int64, device="cuda")
    h_st = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    hp = m.Plan(gpu_ctx, f, in_off, lens, out_off, caps, decompress=True)
    hp.execute(d_in, h_out, h_len, h_st)
    hpaths = m.api.plan_paths(hp)
    hp.close()
    assert hpaths[0] == (n if f == 3 else 0) and hpaths[1] == 0, hpaths
    r = PR.DevRun(m.DevPlan(gpu_ctx, f, n, int(lens.sum()), int(caps.sum()), large_units=True), len(blob), out_total)
    r.load(PR.Batch(blob, in_off, lens, out_off, caps, out_total))
    r.execute()
    torch.cuda.synchronize()
    assert m.api.plan_paths(r.plan) == hpaths, (m.api.plan_paths(r.plan), hpaths)
    mine = slice(PR.PAD, PR.PAD + n)                                  # (compared on the device: 300 MiB of output stay there)
    assert torch.equal(r.d_out, h_out) and torch.equal(r.d_len[mine], h_len) and torch.equal(r.d_st[mine], h_st)
    assert (h_st.cpu().numpy() == 0).all() and bytes(r.d_out[int(out_off[n - 1]): int(out_off[n - 1]) + len(one)].cpu().numpy()) == one
    r.plan.close()
    del r, h_out

    # (c) small units only
    sp, sc = _small(m, gpu_ctx, f, 3000)
    batch = PR.layout(sc[:500], [len(p) for p in sp[:500]])
    host, hpaths, _ = PR.host_run(gpu_ctx, f, batch, "decode", want_paths=True)
    r = PR.DevRun(m.DevPlan(gpu_ctx, f, 500, 64 << 20, 64 << 20, large_units=True), len(batch.blob), batch.out_total + 4096)   # (bounds with room for large units: none comes)
    r.load(batch)
    r.execute()
    PR.same(host, r.result(), batch)
    assert m.api.plan_paths(r.plan) == hpaths == (0, 0, 0)
    r.plan.close()
    del r

    # (d) a capacity of 0xFFFFFF00 and more: its bytes end long before the buffer does
    PR.assert_large(f, comp[2], len(plain[2]))
    units = [comp[2], sc[0], comp[1]]
    caps = np.array([len(plain[2]), len(sp[0]), 0xFFFFFF00], np.uint64)
    blob, in_off, lens, _, _, _ = PR.layout(units, [0, 0, 0])
    out_off = np.array([64, len(plain[2]) + 128, len(plain[2]) + len(sp[0]) + 192], np.uint64)
    out_bytes = int(out_off[2]) + len(plain[1]) + 4096
    batch = PR.Batch(blob, in_off, lens, out_off, caps, out_bytes)
    host, hpaths, _ = PR.host_run(gpu_ctx, f, batch, "decode", want_paths=True)
    assert hpaths[1] == 0 and hpaths[0] == (1 if f == 3 else 0), hpaths
    ctx = m.Context()                                               # (a plan of its own: its all-CU scratch for more than 4 GiB goes away with the context)
    r = PR.DevRun(m.DevPlan(ctx, f, 3, int(lens.sum()), int(caps.sum()), large_units=True), len(blob), out_bytes)
    r.load(batch)
    r.execute()
    dl, ds, do = r.result()
    assert m.api.plan_paths(r.plan) == hpaths, (m.api.plan_paths(r.plan), hpaths)
    assert list(ds) == [0, 0, 0] == list(host[1]) and list(dl) == list(host[0]) == [len(plain[2]), len(sp[0]), len(plain[1])]
    assert (do == host[2]).all()
    assert bytes(do[int(out_off[2]): int(out_off[2]) + len(plain[1])]) == plain[1] and bytes(do[64: 64 + len(plain[2])]) == plain[2]
    r.plan.close()
    del r
    torch.cuda.synchronize()
    ctx.close()


@pytest.mark.parametrize("fmt", XFMTS)
def test_one_plan_changing_batches(oracle, gpu_ctx, fmt):
    """three batches on one plan, tables and bytes rewritten in place: large units present, absent, present at other indices. The second
    and third executions replay the plan's own graph; each equals a fresh host plan, paths included"""
    import ms_compress_amd as m
    f = FMTS[fmt]
    with_large = _mixed_batch(m, gpu_ctx, oracle, f, 0)
    n = len(with_large)
    streams = cases.decode_streams(f, lambda d: oracle.oracle_compress(f, d)[1], n_corrupt=20)
    without = (streams * 2)[:n]
    others = _mixed_batch(m, gpu_ctx, oracle, f, 3)
    assert len(without) == n == len(others) and [c for _, c in others] != [c for _, c in with_large]
    batches = [PR.layout([s for s, _ in b], [c for _, c in b]) for b in (with_large, without, others)]
    r = PR.DevRun(m.DevPlan(gpu_ctx, f, n, max(int(x[2].sum()) for x in batches), max(int(x[4].sum()) for x in batches), large_units=True),
                  max(len(x[0]) for x in batches), max(x[5] for x in batches) + 4096)
    seen = []
    for batch in batches:
        r.load(batch)
        r.execute()
        dev = r.result()
        host, hpaths, _ = PR.host_run(gpu_ctx, f, batch, "decode", want_paths=True)
        PR.same(host, dev, batch)
        assert m.api.plan_paths(r.plan) == hpaths, (m.api.plan_paths(r.plan), hpaths)
        seen.append(hpaths)
    assert seen[0][1] >= 4 and seen[1][1] == 0 and seen[2][1] >= 4 and (f != 3 or (seen[0][0] >= 4 and seen[1][0] == 0))
    r.plan.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_in_a_callers_graph(oracle, gpu_ctx, fmt):
    """execute_dev of a plan with the flag captured with torch.cuda.graph on the single stream of its context; input bytes and tables
    rewritten in place, the graph replayed: each result is that of a host plan (LZNT1: the flag changes nothing)"""
    import torch
    import ms_compress_amd as m
    f = FMTS[fmt]
    if f == 2:
        streams = cases.decode_streams(f, lambda d: oracle.oracle_compress(f, d)[1], n_corrupt=20)
        rnd = np.random.default_rng(8)
        sets = [[streams[i] for i in rnd.choice(len(streams), 96, replace=False)] for _ in range(3)]
    else:
        sets = [_mixed_batch(m, gpu_ctx, oracle, f, 0), _mixed_batch(m, gpu_ctx, oracle, f, 2), _mixed_batch(m, gpu_ctx, oracle, f, 5)]
    n = len(sets[0])
    batches = [PR.layout([s for s, _ in b], [c for _, c in b]) for b in sets]
    s = torch.cuda.Stream()
    ctx = m.Context(stream=s)
    with torch.cuda.stream(s):
        r = PR.DevRun(m.DevPlan(ctx, f, n, max(int(x[2].sum()) for x in batches), max(int(x[4].sum()) for x in batches), large_units=True),
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
        host, hpaths, _ = PR.host_run(gpu_ctx, f, batch, "decode", want_paths=True)
        PR.same(host, r.result(), batch)
        assert m.api.plan_paths(r.plan) == (hpaths if f != 2 else (0, 0, 0)), (m.api.plan_paths(r.plan), hpaths)
    del g
    r.plan.close()
    ctx.close()


@pytest.mark.parametrize("fmt", XFMTS)
def test_rejected_large_units_take_no_path(oracle, gpu_ctx, fmt):
    """a 3 MB unit whose running in_len total crosses in_total_max, and one whose running out_cap total crosses out_total_max: ARG_ERROR,
    length 0, nothing written, not counted by plan_paths; the units before it decode as with a host plan, the empty ones behind it too"""
    import ms_compress_amd as m
    f = FMTS[fmt]
    plain, comp = PR.corpus_streams(f, SIZES, gpu_ctx)
    sp, sc = _small(m, gpu_ctx, f, 3000)
    PR.assert_large(f, comp[2], len(plain[2]))
    units = [sc[0], comp[2], sc[1], comp[2], b"", b""]
    caps = [len(sp[0]), len(plain[2]), len(sp[1]), len(plain[2]), 0, 0]
    batch = PR.layout(units, caps)
    blob, in_off, lens, out_off, caps, out_total = batch
    host, hpaths, _ = PR.host_run(gpu_ctx, f, batch, "decode", want_paths=True)
    assert hpaths[0] == (2 if f == 3 else 0) and hpaths[1] == 2, hpaths
    # (an empty unit behind the rejected one adds nothing to a running total, but the total it is judged at is past the bound: rejected too)
    acc_behind = np.array([True, True, True, False, False, False])
    for in_max, out_max in ((int(lens[:4].sum()) - 1, int(caps.sum())), (int(lens.sum()), int(caps[:4].sum()) - 1)):
        r = PR.DevRun(m.DevPlan(gpu_ctx, f, len(units), in_max, out_max, large_units=True), len(blob), out_total + 4096)
        r.load(batch)
        r.execute()
        dev = r.result()
        PR.same(host, dev, batch, acc_behind)
        assert list(dev[1][:3]) == [0, 0, 0] and dev[1][3] == -2 and dev[0][3] == 0
        o = int(out_off[3])
        assert (dev[2][o: o + int(caps[3])] == GUARD).all()
        got = m.api.plan_paths(r.plan)
        assert got[0] == (1 if f == 3 else 0) and got[1] == 1, got
        r.plan.close()


@pytest.mark.parametrize("fmt", XFMTS)
def test_size_plans_walk_large_streams_by_segments(gpu_ctx, fmt):
    """SizeDevPlan(large_units=True) on one 12 MB unit among 3 000 small ones: status, length and need equal the host size plan's, with
    and without limits, and at limits just below and at the large unit's length; the large Xpress stream is sized by segments"""
    import ms_compress_amd as m
    f = FMTS[fmt]
    plain, _ = PR.corpus_streams(f, SIZES, gpu_ctx)
    units, caps, at = _one_large_among_small(m, gpu_ctx, f)
    batch = PR.layout(units)
    caps = np.array(caps, np.uint64)

    r = PR.DevRun(m.SizeDevPlan(gpu_ctx, f, len(units), int(batch.lens.sum()), large_units=True), len(batch.blob), 0)
    below, at_len = caps.copy(), caps.copy()
    below[at] = len(plain[3]) - 1
    for limits in (None, caps, below, at_len):
        b = batch._replace(caps=limits)
        host = PR.host_run(gpu_ctx, f, b, "size")
        hmodes = PR.decode_modes(gpu_ctx)
        r.load(b)
        r.execute(limited=limits is not None)
        dev = r.result()
        dmodes = PR.decode_modes(gpu_ctx)
        PR.same_sizes(host, dev)
        paths = m.api.plan_paths(r.plan)
        assert paths == ((1, 0, 0) if f == 3 else (0, 0, 0)), paths
        if f == 3:
            assert dmodes == hmodes and len(dmodes) == 1, (dmodes, hmodes)
            if limits is not below:
                assert dmodes == [2]
        if limits is not below:
            assert dev[1][at] == 0 and int(dev[0][at]) == len(plain[3]) == int(dev[3][at])
        else:
            assert dev[1][at] != 0
    r.plan.close()


_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np, torch
import ms_compress_amd as m
import plans_rig as PR
ctx = m.Context()
for f in (3, 4):
    plain, comp = PR.corpus_streams(f, %r, ctx)
    PR.assert_large(f, comp[2], len(plain[2])); PR.assert_large(f, comp[3], len(plain[3]))
    units, caps = [comp[0], comp[3], comp[1], comp[2]], [len(plain[0]), len(plain[3]), len(plain[1]), len(plain[2])]
    batch = PR.layout(units, caps)
    blob, in_off, lens, out_off, caps, out_total = batch
    host, hpaths, _ = PR.host_run(ctx, f, batch, "decode", want_paths=True)
    r = PR.DevRun(m.DevPlan(ctx, f, 4, int(lens.sum()), int(caps.sum()), large_units=True), len(blob), out_total + 4096)
    r.load(batch)
    r.execute()
    dev = r.result()
    PR.same(host, dev, batch)
    for k, i in enumerate((0, 3, 1, 2)):
        assert dev[1][k] == 0 and bytes(dev[2][int(out_off[k]): int(out_off[k]) + len(plain[i])]) == plain[i]
    got = m.api.plan_paths(r.plan)
    assert got == hpaths and got[1] == 0 and got[2] == 0 and got[0] == (2 if f == 3 else 0), (got, hpaths)
    r.plan.close()
ctx.close()
print("BUDGETS-OFF-OK")
""" % (SIZES,)


def test_budgets_off(gpu_ctx):
    """MSCOMP_AMD_LZG_MAX_MB=0 and MSCOMP_AMD_XHC_SCR_MAX_MB=0 (read once, so in a fresh process): creation succeeds, no unit on the all-CU
    stage, no token scratch, the segment walk still runs, the bytes are right"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MSCOMP_AMD_LZG_MAX_MB="0", MSCOMP_AMD_XHC_SCR_MAX_MB="0", MSCOMP_AMD_TEST_HOOKS="1")
    p = subprocess.run([sys.executable, "-c", _CHILD, root], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "BUDGETS-OFF-OK" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])


@pytest.mark.parametrize("fmt", XFMTS)
def test_the_whole_chain_with_a_large_unit(gpu_ctx, fmt):
    """size dev plan -> layout_dev(d_need) -> decompress dev plan -> CompressDevPlan -> compact_dev -> decompress dev plan, all three dev
    plans for large units, nothing copied to the host in between: the original bytes come back"""
    import torch
    import ms_compress_amd as m
    f = FMTS[fmt]
    plain, comp = PR.corpus_streams(f, SIZES, gpu_ctx)
    sp, sc = _small(m, gpu_ctx, f, 3000)
    PR.assert_large(f, comp[3], len(plain[3]))
    PR.assert_large(f, comp[2], len(plain[2]))
    orig = [sp[0], plain[3], sp[1], plain[1], plain[2], sp[2]]
    units = [sc[0], comp[3], sc[1], comp[1], comp[2], sc[2]]
    n = len(units)
    blob, in_off, lens, _, _, _ = PR.layout(units, [0] * n)
    total_plain = sum(len(p) for p in orig)
    d_in, d_in_off, d_in_len = torch.from_numpy(blob).cuda(), PR.dt(in_off), PR.dt(lens)
    Z = lambda dt=torch.int64: torch.zeros(n, dtype=dt, device="cuda")  # noqa: E731
    d_slen, d_need, d_sst = Z(), Z(), Z(torch.int32)
    d_len1, d_st1, d_clen, d_cst, d_len2, d_st2 = Z(), Z(torch.int32), Z(), Z(torch.int32), Z(), Z(torch.int32)
    out_room = total_plain + 16 * n + 64
    d_out1 = torch.full((out_room,), GUARD, dtype=torch.uint8, device="cuda")
    d_out2 = torch.full((out_room,), GUARD, dtype=torch.uint8, device="cuda")
    comp_room = sum(m.max_compressed_size(f, len(p)) + 2 + 16 for p in orig)
    d_comp = torch.zeros(comp_room + 64, dtype=torch.uint8, device="cuda")
    splan = m.SizeDevPlan(gpu_ctx, f, n, int(lens.sum()), large_units=True)
    dplan = m.DevPlan(gpu_ctx, f, n, comp_room, total_plain, large_units=True)
    cplan = m.CompressDevPlan(gpu_ctx, f, n, total_plain, max(len(p) for p in orig))
    torch.cuda.synchronize()
    splan.execute(d_in, d_in_off, d_in_len, d_slen, d_need, d_sst)
    d_ooff = m.layout_dev(gpu_ctx, d_need, 16)
    dplan.execute(d_in, d_in_off, d_in_len, d_out1, d_ooff, d_need, d_len1, d_st1)
    d_coff, d_ccap = m.api.plan_layout_dev(gpu_ctx, f, d_len1, 16)
    cplan.execute(d_out1, d_ooff, d_len1, d_comp, d_coff, d_ccap, d_clen, d_cst)
    d_packed, d_poff = m.api.compact_dev(gpu_ctx, d_comp, d_coff, d_clen, align=8)
    dplan.execute(d_packed, d_poff, d_clen, d_out2, d_ooff, d_need, d_len2, d_st2)
    torch.cuda.synchronize()
    assert m.api.plan_paths(dplan)[1] == 2 and m.api.plan_paths(splan)[0] == (2 if f == 3 else 0)
    ooff = d_ooff.cpu().numpy()
    for name, st in (("size", d_sst), ("decode", d_st1), ("compress", d_cst), ("decode again", d_st2)):
        assert (st.cpu().numpy() == 0).all(), (name, st.cpu().numpy())
    out1, out2, ln2 = d_out1.cpu().numpy(), d_out2.cpu().numpy(), d_len2.cpu().numpy()
    for i, p in enumerate(orig):
        o = int(ooff[i])
        assert int(ln2[i]) == len(p) and bytes(out1[o: o + len(p)]) == p and bytes(out2[o: o + len(p)]) == p, i
    for p in (splan, dplan, cplan):
        p.close()
