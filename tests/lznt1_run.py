"""The GPU side of the tests/test_gpu_lznt1_*.py case files: the two test hooks of the LZNT1 chunk kernels, the oracle's bytes of a unit, a batch
through compress_units and a batch through a plan, each compared byte for byte with the oracle. torch and the library are imported inside the
functions, so a case file can be imported (and its builders tested) without a GPU."""
import contextlib

import numpy as np

LZNT1 = 2
GUARD = 0xEE
PATHS = ("host-tables", "device-tables", "serial-atomics")


@contextlib.contextmanager
def hooks(gpu_ctx, mode=0, serial=0):
    """the chunk-kernel mode and the order-independent form of the atomics, both back at 0 afterwards"""
    lib = gpu_ctx.lib
    try:
        lib.mscomp_amd_debug_set_lznt1(mode)
        lib.mscomp_amd_debug_set_serial_atomics(serial)
        yield
    finally:
        lib.mscomp_amd_debug_set_lznt1(0)
        lib.mscomp_amd_debug_set_serial_atomics(0)


_ORACLE_OUT = {}


def expected(oracle, unit):
    """the oracle's bytes of a unit, computed once per session and shared by every test, mode and path"""
    key = unit if isinstance(unit, bytes) else unit.tobytes()
    if key not in _ORACLE_OUT:
        es, exp = oracle.oracle_compress(LZNT1, unit)
        assert es == 0, (len(unit), es)
        _ORACLE_OUT[key] = exp
    return _ORACLE_OUT[key]


def _label(names, i):
    return names[i] if names else "unit %d" % i


def check_batch(oracle, gpu_ctx, units, mode, serial, what, copies=1, passes=1, names=None):
    """the units through compress_units against the oracle; with `copies`, that many concurrent copies of every unit per batch, `passes` batches,
    identical bytes demanded of every copy of every pass"""
    import ms_compress_amd as m
    want = [expected(oracle, u) for u in units]
    with hooks(gpu_ctx, mode, serial):
        for pas in range(passes):
            got, st = m.compress_units(LZNT1, [u for u in units for _ in range(copies)], ctx=gpu_ctx)
            if copies > 1:
                assert all(s == 0 for s in st)
                bad = [i for i, g in enumerate(got) if g != want[i // copies]]
                assert not bad, "pass %d, mode %d, serial %d: %d of %d copies differ from the oracle, first: copy %d of unit %d" % (pas, mode, serial, len(bad), len(got), bad[0] % copies, bad[0] // copies)
                continue
            for i, (u, g, s, exp) in enumerate(zip(units, got, st, want)):
                assert s == 0, (what, _label(names, i), len(u), s)
                assert g == exp, "%s, mode %d, serial %d, %s (len %d): GPU bytes differ from the oracle (%d vs %d B)" % (what, mode, serial, _label(names, i), len(u), len(g), len(exp))


def _dt(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def run_plan(gpu_ctx, units, mode, path, executions=1):
    """One batch of all units (bytes) executed by one plan: ([(lengths, statuses, output)] per execution, output offsets, capacities). Input offsets
    are odd (unit i starts at an odd byte, a gap of 1 or 2 behind the unit before), guard bytes lie around every capacity, and nothing outside a
    capacity may change. The device-table plan's bound lies eight chunks above the batch: the blocks past the real chunk count run too."""
    import torch
    import ms_compress_amd as m
    in_off, pos = [], 1
    for u in units:
        in_off.append(pos)
        pos += len(u)
        pos += 1 if pos % 2 == 0 else 2
    assert all(o % 2 == 1 for o in in_off)
    blob = np.zeros(pos + 32, np.uint8)
    for u, o in zip(units, in_off):
        blob[o: o + len(u)] = np.frombuffer(u, np.uint8)
    caps = [m.max_compressed_size(LZNT1, len(u)) + 2 for u in units]
    out_off, total = [], 16
    for cp in caps:
        out_off.append(total)
        total += cp + 16
    in_off, lens, out_off, caps = (np.array(a, np.uint64) for a in (in_off, [len(u) for u in units], out_off, caps))
    inside = np.zeros(total, bool)
    for o, cp in zip(out_off, caps):
        inside[int(o): int(o) + int(cp)] = True
    n = len(units)
    d_in = torch.from_numpy(blob).cuda()
    d_len = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
    if path == "device-tables":
        plan = m.CompressDevPlan(gpu_ctx, LZNT1, n, int(lens.sum()) + 8 * 4096, int(lens.max()))
        tabs = [_dt(a) for a in (in_off, lens, out_off, caps)]
    else:
        plan = m.Plan(gpu_ctx, LZNT1, in_off, lens, out_off, caps)
    res = []
    try:
        with hooks(gpu_ctx, mode, 1 if path == "serial-atomics" else 0):
            for k in range(executions):
                d_out = torch.full((total,), GUARD, dtype=torch.uint8, device="cuda")
                d_len.fill_(-1)
                d_st.fill_(77)
                if path == "device-tables":
                    plan.execute(d_in, tabs[0], tabs[1], d_out, tabs[2], tabs[3], d_len, d_st)
                else:
                    plan.execute(d_in, d_out, d_len, d_st)
                torch.cuda.synchronize()
                res.append((d_len.cpu().numpy().copy(), d_st.cpu().numpy().copy(), d_out.cpu().numpy().copy()))
    finally:
        plan.close()
    for k, (_, _, out) in enumerate(res):
        assert (out[~inside] == GUARD).all(), (mode, path, k, np.nonzero(out[~inside] != GUARD)[0][:8])
    return res, out_off, caps


def check_plan(oracle, gpu_ctx, units, mode, path, what, first=0, executions=1, names=None):
    """units[first:] through a plan against the oracle (the units in front only move the chunk indices): status 0 for every unit, the oracle's
    bytes, nothing written outside a capacity, and all executions equal"""
    res, out_off, _ = run_plan(gpu_ctx, units, mode, path, executions)
    for k, (ln, st, out) in enumerate(res):
        for i, u in enumerate(units):
            assert st[i] == 0, (what, mode, path, k, _label(names, i), len(u), st[i])
            if i < first:
                continue
            exp = expected(oracle, u)
            got = bytes(out[int(out_off[i]): int(out_off[i]) + max(int(ln[i]), 0)])
            assert got == exp, "%s, mode %d, %s, execution %d, %s (len %d): GPU bytes differ from the oracle (%d vs %d B)" % (what, mode, path, k, _label(names, i), len(u), len(got), len(exp))
    for k in range(1, executions):
        assert all((a == b).all() for a, b in zip(res[0], res[k])), "%s, mode %d, %s: two executions of one plan differ" % (what, mode, path)
