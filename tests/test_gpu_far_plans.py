"""GPU: the plan family at unit offsets that need more than 31 and more than 32 bits (tests/far_rig.py: one arena of 4 GiB + 64 MiB, of
which a case writes two small windows). Per format and base one batch of five units -- 70 000 bytes of LZ data (two Xpress+Huffman chunks,
18 LZNT1 chunks), 4 097 bytes of words, 300 random bytes (raw fallback), 1 byte, nothing -- at the odd spacings of plans_rig.layout, the
input side at one base and the output side at another. Expected values are the oracle's; the aliases of the input window hold a decoy
(the same units from another seed), the aliases of the output window canaries.

A host plan's tables are fixed at creation, so its second execution replays its graph at the same offsets into refilled windows; a dev
plan's tables are rewritten in place, so its second execution runs with both windows moved to other bases (far_rig.MOVED)."""
import numpy as np
import pytest

import far_rig as FR
import plans_rig as PR
from plans_rig import FMTS, G_LEN, G_ST, PAD

pytestmark = pytest.mark.gpu


class Outs:
    """out_len, need and status of n units between PAD guard entries, as plans_rig.DevRun keeps them"""

    def __init__(self, n):
        import torch
        self.n = n
        self.t = [torch.empty(n + 2 * PAD, dtype=d, device="cuda") for d in (torch.int64, torch.int64, torch.int32)]

    def fill(self):
        for t, v in zip(self.t, (G_LEN, G_LEN, G_ST)):
            t.fill_(v)
        return [t[PAD: PAD + self.n] for t in self.t]

    def pull(self):
        import torch
        torch.cuda.synchronize()
        return [PR.strip_guards(t.cpu().numpy(), self.n, v).copy() for t, v in zip(self.t, (G_LEN, G_LEN, G_ST))]


def _far(arena, near, decoy, pair):
    """the far run of a near batch with its input and its output at the (input place, output place) of ``pair``"""
    run = FR.FarRun(arena, near, FR.PLACES[pair[0]], FR.PLACES[pair[1]], decoy.blob)
    for name, at, n in ((pair[0], run.batch.in_off[0], near.lens[0]), (pair[1], run.batch.out_off[0], near.caps[0])):
        assert name.startswith("above") or FR.straddles(name, int(at), int(n))
    return run


def _host(ctx, f, arena, run, kind, outs, times=2):
    """a host-table plan on the far tables, executed ``times`` times into refilled windows: the results"""
    plan = PR.host_plan(ctx, f, run.batch, kind)
    res = []
    for _ in range(times):
        run.wout.refill()
        ln, need, st = outs.fill()
        if kind == "size":
            plan.execute(arena.t, ln, need, st)
        else:
            plan.execute(arena.t, arena.t, ln, st)
        ln, need, st = outs.pull()
        res.append((ln, st, run.wout.get()) + ((need,) if kind == "size" else ()))
        run.intact()
    plan.close()
    return res


class Dev:
    """one device-table plan and its four tables, rewritten in place between executions"""

    def __init__(self, plan, n):
        import torch
        self.plan, self.n = plan, n
        self.tabs = [torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(4)]

    def run(self, arena, run, outs, size=False):
        b = run.batch
        for t, a in zip(self.tabs, (b.in_off, b.lens, b.out_off, b.caps)):
            t.copy_(PR.dt(a))
        ln, need, st = outs.fill()
        if size:
            self.plan.execute(arena.t, self.tabs[0], self.tabs[1], ln, need, st, self.tabs[3])
        else:
            self.plan.execute(arena.t, self.tabs[0], self.tabs[1], arena.t, self.tabs[2], self.tabs[3], ln, st)
        ln, need, st = outs.pull()
        run.intact()
        return (ln, st, run.wout.get()) + ((need,) if size else ())


def _is_oracle_compress(oracle, f, res, near, units):
    """status, length and bytes of every unit are oracle_compress's at the unit's capacity; nothing is written outside the capacities"""
    for i, u in enumerate(units):
        so, oo = oracle.oracle_compress(f, u, int(near.caps[i]))
        assert (int(res[1][i]), int(res[0][i])) == (so, len(oo)), (i, res[1][i], so, res[0][i], len(oo))
        assert PR.unit(res, near, i) == oo, i
    PR.guards_intact(res, near)


def _is_oracle_decode(oracle, f, res, near, streams):
    for i, s in enumerate(streams):
        so, oo, undefined = oracle.oracle_decompress_ex(f, s, int(near.caps[i]))
        assert not undefined
        assert int(res[1][i]) == so, (i, res[1][i], so)
        if so == 0:
            assert int(res[0][i]) == len(oo) and PR.unit(res, near, i) == oo, i
    PR.guards_intact(res, near)


@pytest.mark.parametrize("base", list(FR.BASES))
@pytest.mark.parametrize("fmt", list(FMTS))
def test_compress_at_far_offsets(oracle, gpu_ctx, fmt, base):
    """host plan and CompressDevPlan: every unit's status, length and bytes are oracle_compress's; guards and aliases intact; the host
    plan's replay gives the same, the dev plan's second execution runs at moved windows"""
    import ms_compress_amd as m
    f, arena = FMTS[fmt], FR.arena(gpu_ctx)
    units, decoys = FR.units(1), FR.units(2)
    caps = [m.max_compressed_size(f, len(u)) + 2 for u in units]
    near, decoy = PR.layout(units, caps), PR.layout(decoys, caps)
    outs = Outs(len(units))
    with arena.case():
        run = _far(arena, near, decoy, FR.PAIR[base])
        host = _host(gpu_ctx, f, arena, run, "compress", outs)
        for h in host:
            _is_oracle_compress(oracle, f, h, near, units)
        dev = Dev(m.CompressDevPlan(gpu_ctx, f, len(units), int(near.lens.sum()), 70000), len(units))
        run.wout.refill()
        first = dev.run(arena, run, outs)
        _is_oracle_compress(oracle, f, first, near, units)
        PR.same(host[0], first, near, tail=2)
    with arena.case():
        run = _far(arena, near, decoy, FR.MOVED[base])
        second = dev.run(arena, run, outs)
        _is_oracle_compress(oracle, f, second, near, units)
        PR.same(host[0], second, near, tail=2)
    dev.plan.close()


@pytest.mark.parametrize("base", list(FR.BASES))
@pytest.mark.parametrize("fmt", list(FMTS))
def test_decompress_at_far_offsets(oracle, gpu_ctx, fmt, base):
    """host plan and DevPlan at exact, one short and generous capacities, both sides far: status, length and bytes are the oracle's and
    plans_rig.same holds between host and dev run. The one dev plan runs the three batches in turn, each at windows moved from the last."""
    import ms_compress_amd as m
    f, arena = FMTS[fmt], FR.arena(gpu_ctx)
    plain, comp, decoys = FR.streams(oracle, f)
    outs = Outs(len(comp))
    lens = sum(len(c) for c in comp)
    dev = Dev(m.DevPlan(gpu_ctx, f, len(comp), lens, sum(len(p) for p in plain) + 5000 * len(plain)), len(comp))
    for (kind, cap), at in zip(FR.CAPS.items(), (FR.PAIR[base], FR.MOVED[base], FR.PAIR[base])):
        caps = [cap(len(p)) for p in plain]
        near, decoy = PR.layout(comp, caps), PR.layout(decoys, caps)
        with arena.case():
            run = _far(arena, near, decoy, at)
            host = _host(gpu_ctx, f, arena, run, "decode", outs)
            for h in host:
                _is_oracle_decode(oracle, f, h, near, comp)
            run.wout.refill()
            got = dev.run(arena, run, outs)
            _is_oracle_decode(oracle, f, got, near, comp)
            PR.same(host[0], got, near)
    dev.plan.close()


@pytest.mark.parametrize("base", list(FR.BASES))
@pytest.mark.parametrize("fmt", list(FMTS))
def test_size_query_at_far_offsets(oracle, gpu_ctx, fmt, base):
    """SizePlan, mscomp_amd_decompressed_size_batch and SizeDevPlan on far in_off, with limits exact, one short and generous: status,
    length and need are those of the same call at near offsets (and the need of a sized unit is the oracle's length)"""
    import torch
    import ms_compress_amd as m
    from ms_compress_amd._core import _run
    f, arena = FMTS[fmt], FR.arena(gpu_ctx)
    plain, comp, decoys = FR.streams(oracle, f)
    n = len(comp)
    outs = Outs(n)
    dev = Dev(m.SizeDevPlan(gpu_ctx, f, n, sum(len(c) for c in comp)), n)
    for (kind, cap), at in zip(FR.CAPS.items(), (FR.PAIR[base], FR.MOVED[base], FR.PAIR[base])):
        caps = [cap(len(p)) for p in plain]
        near, decoy = PR.layout(comp, caps), PR.layout(decoys, caps)
        want = PR.host_run(gpu_ctx, f, near, "size")
        for i, p in enumerate(plain):
            assert want[1][i] != 0 or int(want[3][i]) == len(p)
        with arena.case():
            run = _far(arena, near, decoy, at)
            for h in _host(gpu_ctx, f, arena, run, "size", outs):
                PR.same_sizes(want, h)
            ln, need, st = outs.fill()
            b = run.batch
            _run(gpu_ctx, "mscomp_amd_decompressed_size_batch", gpu_ctx._h, f, n, arena.t, b.in_off.ctypes.data, b.lens.ctypes.data,
                 b.caps.ctypes.data, ln, need, st)
            ln, need, st = outs.pull()
            PR.same_sizes(want, (ln, st, None, need))
            PR.same_sizes(want, dev.run(arena, run, outs, size=True))
            run.wout.guards_intact()
    dev.plan.close()
    torch.cuda.synchronize()


@pytest.mark.parametrize("base", list(FR.BASES))
@pytest.mark.parametrize("fmt", list(FMTS))
def test_one_shot_batches_at_far_offsets(oracle, gpu_ctx, fmt, base):
    """mscomp_amd_compress_batch and mscomp_amd_decompress_batch (host tables, no plan kept) with both sides far: the oracle's answers"""
    import ms_compress_amd as m
    from ms_compress_amd._core import _run
    f, arena = FMTS[fmt], FR.arena(gpu_ctx)
    plain, comp, decoys = FR.streams(oracle, f)
    outs = Outs(len(plain))
    for export, units, dec, caps, check in (
            ("mscomp_amd_compress_batch", plain, FR.units(2), [m.max_compressed_size(f, len(u)) + 2 for u in plain], _is_oracle_compress),
            ("mscomp_amd_decompress_batch", comp, decoys, [len(p) for p in plain], _is_oracle_decode)):
        near, decoy = PR.layout(units, caps), PR.layout(dec, caps)
        with arena.case():
            run = _far(arena, near, decoy, FR.PAIR[base])
            b = run.batch
            ln, need, st = outs.fill()
            _run(gpu_ctx, export, gpu_ctx._h, f, len(units), arena.t, b.in_off.ctypes.data, b.lens.ctypes.data,
                 arena.t, b.out_off.ctypes.data, b.caps.ctypes.data, ln, st)
            ln, need, st = outs.pull()
            run.intact()
            check(oracle, f, (ln, st, run.wout.get()), near, units)


@pytest.mark.parametrize("base", list(FR.BASES))
def test_crc_plan_at_far_offsets(gpu_ctx, base):
    """CrcDevPlan on far d_in_off: zlib's crc32 of every unit, first at ``base``, then -- tables rewritten in place -- at the moved base"""
    import zlib
    import torch
    import ms_compress_amd as m
    arena = FR.arena(gpu_ctx)
    units, decoys = FR.units(1), FR.units(2)
    n = len(units)
    near, decoy = PR.layout(units, [0] * n), PR.layout(decoys, [0] * n)
    plan = m.CrcDevPlan(gpu_ctx, n, int(near.lens.sum()))
    d_off, d_len = torch.zeros(n, dtype=torch.int64, device="cuda"), PR.dt(near.lens)
    for at in (base, FR.MOVED[base][0]):
        with arena.case():
            win = FR.Window(arena, FR.PLACES[at], len(near.blob), "input")
            win.put(0, near.blob)
            win.put_alias(0, decoy.blob)
            d_off.copy_(PR.dt(near.in_off + np.uint64(FR.PLACES[at])))
            d_crc = torch.full((n + 2 * PAD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            d_st = torch.full((n + 2 * PAD,), G_ST, dtype=torch.int32, device="cuda")
            plan.execute(arena.t, d_off, d_len, d_crc[PAD: PAD + n], d_st[PAD: PAD + n])
            torch.cuda.synchronize()
            crc = PR.strip_guards(d_crc.cpu().numpy(), n, 0x5A5A5A5A).view(np.uint32)
            assert not PR.strip_guards(d_st.cpu().numpy(), n, G_ST).any()
            assert [int(x) for x in crc] == [zlib.crc32(u) for u in units]
            assert win.aliases_intact() and bytes(win.get()) == bytes(near.blob)
    plan.close()


@pytest.mark.parametrize("base", list(FR.BASES))
def test_compaction_at_far_offsets(gpu_ctx, base):
    """compact_dev with caller-given far d_src_off, and mscomp_amd_compact_batch with a far host out_off: the units back to back, as
    the same call packs them from near offsets. (The packed offsets are the calls' own running sums: nothing far about them.)"""
    import torch
    import ms_compress_amd as m
    arena = FR.arena(gpu_ctx)
    units, decoys = FR.units(1), FR.units(2)
    n = len(units)
    lens = [len(u) for u in units]
    near, decoy = PR.layout(units, lens), PR.layout(decoys, lens)
    d_len = PR.dt(near.lens)
    want_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    with arena.case():
        win = FR.Window(arena, FR.BASES[base], len(near.blob), "source")
        win.put(0, near.blob)
        win.put_alias(0, decoy.blob)
        far_off = near.in_off + np.uint64(FR.BASES[base])
        d_packed = torch.full((sum(lens) + 64,), PR.GUARD, dtype=torch.uint8, device="cuda")
        _, d_poff = m.compact_dev(gpu_ctx, arena.t, PR.dt(far_off), d_len, 1, d_packed=d_packed, packed_cap=sum(lens))
        torch.cuda.synchronize()
        assert (d_poff.cpu().numpy().view(np.uint64) == want_off).all()
        got = d_packed.cpu().numpy()
        assert bytes(got[: sum(lens)]) == b"".join(units) and (got[sum(lens):] == PR.GUARD).all()
        d_packed2, d_poff2 = m.compact_batch(gpu_ctx, far_off, near.lens, arena.t, d_len)
        torch.cuda.synchronize()
        assert (d_poff2.cpu().numpy().view(np.uint64) == want_off).all()
        assert bytes(d_packed2.cpu().numpy()[: sum(lens)]) == b"".join(units)
        assert win.aliases_intact() and bytes(win.get()) == bytes(near.blob)
