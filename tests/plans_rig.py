"""What the GPU tests of the plan family (host-table plans, device-table plans for decompress, compress and size, large units, compaction,
scratch) share: the constants, the table upload (dt), the unit layout of a batch (layout), the corpus slices (corpus_units,
corpus_streams), a host-table plan executed into guard-filled outputs (host_plan / host_execute / host_run), one device-table plan with
the buffers of its batches (DevRun), and the comparisons (same, same_sizes, unit, guards_intact, strip_guards). A result is the tuple
(out_len, status, output bytes incl. guards), with need as a fourth entry for a size plan; every array of it is filled before the
execution, so that two executions can be compared whole. The comparisons run on host arrays, so tests/test_plans_rig.py pins them without
a device. torch is imported inside the functions that need it. Not collected as a test."""
import collections
import ctypes as C

import numpy as np

FMTS = {"lznt1": 2, "xpress": 3, "xpress_huff": 4}
GUARD = 0xEE                                                         # what output bytes hold before an execution
GAP = 48                                                             # guard bytes between the capacities of two units
PAD = 8                                                              # guard entries in front of and behind every result array of a DevRun
G_LEN, G_ST = 0x5A5A5A5A5A5A5A5A, 77                                 # what lengths / needs and statuses hold before an execution, guard entries included
ARG = -2                                                             # MSCOMP_ARG_ERROR
XPS_MIN_IN, LZG_MIN_CAP = 512 << 10, 1 << 20                         # csrc/kernels.h: the thresholds of the paths for large units

Batch = collections.namedtuple("Batch", "blob in_off lens out_off caps out_total")
_memo = {}


def dt(a):
    """a uint64 host table as an int64 CUDA tensor"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.uint64)).view(np.int64).copy()).cuda()


def layout(units, caps=None):
    """the units packed at 16-byte offsets with 16 spare bytes behind them; the outputs capacity after capacity with GAP guard bytes in
    front, between and behind (a capacity of 0 still gets an offset of its own). No capacities: the batch of a size plan without limits."""
    import ms_compress_amd as m
    lens = [len(u) for u in units]
    in_off, in_total = m.pack_offsets(lens)
    out_off, pos = np.zeros(len(units), np.uint64), GAP
    for i, c in enumerate([0] * len(units) if caps is None else caps):
        out_off[i] = pos
        pos += int(c) + GAP
    blob = np.zeros(in_total + 16, np.uint8)
    for u, o in zip(units, in_off):
        blob[int(o): int(o) + len(u)] = np.frombuffer(bytes(u), np.uint8)
    return Batch(blob, in_off, np.array(lens, np.uint64), out_off, None if caps is None else np.array(caps, np.uint64), pos + GAP)


def corpus_units(sizes, name="mozilla"):
    """consecutive slices of the generated corpus"""
    from ms_compress_amd import corpus
    data = corpus.by_name(name, sum(sizes) + 1000).tobytes()
    out, pos = [], 0
    for s in sizes:
        out.append(data[pos: pos + s])
        pos += s
    return out


def corpus_streams(f, sizes, ctx=None):
    """(corpus_units(sizes), their compressed streams), made once per format and sizes"""
    import ms_compress_amd as m
    key = (f, tuple(sizes))
    if key not in _memo:
        plain = corpus_units(sizes)
        comp, st = m.compress_units(f, plain, ctx=ctx)
        assert all(s == 0 for s in st)
        _memo[key] = (plain, comp)
    return _memo[key]


def assert_large(f, stream, cap):
    """the unit really takes the paths for large units"""
    assert cap >= LZG_MIN_CAP, cap
    if f == 3:
        assert len(stream) >= XPS_MIN_IN, len(stream)


def decode_modes(ctx, cap=8):
    out = (C.c_uint32 * cap)()
    k = ctx.lib.mscomp_amd_debug_decode_modes(ctx._h, out, cap)
    assert k >= 0
    return [int(x) for x in out[: min(k, cap)]]


# ---- host-table plans -------------------------------------------------------------------------------------------------------------------
def host_plan(ctx, f, batch, kind):
    """a host-table plan on the batch's tables; kind: "compress", "decode" or "size" (the capacities are the limits, None = no limit)"""
    import ms_compress_amd as m
    if kind == "size":
        return m.SizePlan(ctx, f, batch.in_off, batch.lens, batch.caps)
    return m.Plan(ctx, f, batch.in_off, batch.lens, batch.out_off, batch.caps, decompress=kind == "decode")


def host_execute(plan, batch):
    """one execution into freshly filled outputs, synchronised: the result. The device buffers are made on the plan's first execution and
    stay with it, so that its later executions pass the same addresses and replay the plan's own graph."""
    import torch
    import ms_compress_amd as m
    n = len(batch.lens)
    if not hasattr(plan, "rig_bufs"):
        plan.rig_bufs = (torch.from_numpy(batch.blob).cuda(), torch.empty(batch.out_total, dtype=torch.uint8, device="cuda")) + tuple(
            torch.empty(max(1, n), dtype=t, device="cuda") for t in (torch.int64, torch.int64, torch.int32))
    d_in, d_out, d_len, d_need, d_st = plan.rig_bufs
    for t, v in ((d_out, GUARD), (d_len, G_LEN), (d_need, G_LEN), (d_st, G_ST)):
        t.fill_(v)
    size = isinstance(plan, m.SizePlan)
    if size:
        plan.execute(d_in, d_len, d_need, d_st)
    else:
        plan.execute(d_in, d_out, d_len, d_st)
    torch.cuda.synchronize()
    return (d_len.cpu().numpy()[:n], d_st.cpu().numpy()[:n], d_out.cpu().numpy()) + ((d_need.cpu().numpy()[:n],) if size else ())


def host_run(ctx, f, batch, kind, want_paths=False):
    """a fresh host-table plan, executed once and closed: the result; want_paths: (result, the plan's paths, the context's decode modes)"""
    import ms_compress_amd as m
    plan = host_plan(ctx, f, batch, kind)
    res = host_execute(plan, batch)
    seen = (m.api.plan_paths(plan), decode_modes(ctx)) if want_paths else None
    plan.close()
    return (res,) + seen if want_paths else res


# ---- device-table plans -----------------------------------------------------------------------------------------------------------------
class DevRun:
    """one device-table plan (DevPlan, CompressDevPlan or SizeDevPlan, made by the caller) and the device buffers of its batches: tables
    and bytes are rewritten in place between executions, every output is refilled, and the three result arrays sit between guard entries"""

    def __init__(self, plan, in_bytes, out_bytes):
        import torch
        import ms_compress_amd as m
        self.plan, self.n, self.size = plan, plan.n_units, isinstance(plan, m.SizeDevPlan)
        self.d_in = torch.zeros(max(16, in_bytes), dtype=torch.uint8, device="cuda")
        self.d_out = torch.full((out_bytes,), GUARD, dtype=torch.uint8, device="cuda")
        self.tabs = [torch.zeros(max(1, self.n), dtype=torch.int64, device="cuda") for _ in range(4)]
        self.d_len = torch.full((self.n + 2 * PAD,), G_LEN, dtype=torch.int64, device="cuda")
        self.d_need = torch.full((self.n + 2 * PAD,), G_LEN, dtype=torch.int64, device="cuda")
        self.d_st = torch.full((self.n + 2 * PAD,), G_ST, dtype=torch.int32, device="cuda")

    def load(self, batch):
        """(a table that is None stays as it is: a size plan executed without limits)"""
        import torch
        self.d_in[: len(batch.blob)].copy_(torch.from_numpy(batch.blob))
        for t, a in zip(self.tabs, (batch.in_off, batch.lens, batch.out_off, batch.caps)):
            if a is not None:
                t[: self.n].copy_(dt(a))
        for t, v in ((self.d_out, GUARD), (self.d_len, G_LEN), (self.d_need, G_LEN), (self.d_st, G_ST)):
            t.fill_(v)

    def execute(self, limited=True):
        i_off, i_len, o_off, o_cap = self.tabs
        ln, need, st = (t[PAD: PAD + self.n] for t in (self.d_len, self.d_need, self.d_st))
        if self.size:
            self.plan.execute(self.d_in, i_off, i_len, ln, need, st, o_cap if limited else None)
        else:
            self.plan.execute(self.d_in, i_off, i_len, self.d_out, o_off, o_cap, ln, st)

    def result(self):
        """the result of the n units; the guard entries around the three arrays must be untouched"""
        import torch
        torch.cuda.synchronize()
        ln, need, st = (strip_guards(t.cpu().numpy(), self.n, v) for t, v in ((self.d_len, G_LEN), (self.d_need, G_LEN), (self.d_st, G_ST)))
        return (ln, st, self.d_out.cpu().numpy()) + ((need,) if self.size else ())

    def run(self, batch):
        self.load(batch)
        self.execute()
        return self.result()


# ---- comparisons, on host arrays ----------------------------------------------------------------------------------------------------------
def strip_guards(a, n, fill):
    """the n entries between the PAD guard entries of a result array, which must still hold ``fill``"""
    assert len(a) == n + 2 * PAD and (a[:PAD] == fill).all() and (a[PAD + n:] == fill).all(), "guard entries overwritten"
    return a[PAD: PAD + n]


def same(host, dev, batch, accepted=None, tail=0):
    """status and length of every unit as the host plan's, and its bytes where the host's status is 0 -- over the length, or for a
    compress plan over min(capacity, length + tail) with tail = 2 (LZNT1's uncounted 00 00 included); units outside ``accepted``:
    (ARG, 0) and nothing written; every byte outside the accepted capacities, and past out_total, still the guard"""
    (hl, hs, ho), (dl, ds, do) = host[:3], dev[:3]
    inside = np.zeros(len(do), bool)
    for i in range(len(batch.caps)):
        if accepted is not None and not accepted[i]:
            assert ds[i] == ARG and dl[i] == 0, (i, ds[i], dl[i])
            continue
        assert (ds[i], dl[i]) == (hs[i], hl[i]), (i, ds[i], hs[i], dl[i], hl[i])
        o = int(batch.out_off[i])
        if hs[i] == 0:
            end = min(int(batch.caps[i]), int(hl[i]) + tail)
            assert bytes(do[o: o + end]) == bytes(ho[o: o + end]), i
        inside[o: o + int(batch.caps[i])] = True
    outside = ~inside
    outside[batch.out_total:] = True
    assert (do[outside] == GUARD).all(), np.nonzero(do[outside] != GUARD)[0][:8]


def same_sizes(host, dev, accepted=None):
    """status, length and need of every unit as the host size plan's; units outside ``accepted``: (ARG, 0, 0)"""
    (hl, hs, _, hn), (dl, ds, _, dn) = host, dev
    assert len(ds) == len(hs)
    for i in range(len(hs)):
        if accepted is not None and not accepted[i]:
            assert (ds[i], dl[i], dn[i]) == (ARG, 0, 0), (i, ds[i], dl[i], dn[i])
            continue
        assert (ds[i], dl[i], dn[i]) == (hs[i], hl[i], hn[i]), (i, ds[i], hs[i], dl[i], hl[i], dn[i], hn[i])


def unit(res, batch, i):
    """the bytes unit i wrote"""
    return bytes(res[2][int(batch.out_off[i]): int(batch.out_off[i]) + int(res[0][i])])


def guards_intact(res, batch):
    keep = np.ones(len(res[2]), bool)
    for o, c in zip(batch.out_off, batch.caps):
        keep[int(o): int(o) + int(c)] = False
    keep[batch.out_total:] = True
    assert (res[2][keep] == GUARD).all(), "written outside every capacity"
