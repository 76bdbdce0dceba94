"""GPU: CRC-32 of batches in HBM (CrcDevPlan) and the block container's checksums (BlockContainer.crc / .check) against zlib.crc32
(tests/crc_model.py). Integer work: every value must be equal.
The container tests stand on the rig and recipes of tests/blocks_rig.py that test_gpu_blocks.py drives too (BlockRig under CrcRig,
fixture_bufs under crc_bufs): both files drive one container the same way."""
import numpy as np
import pytest

import blocks_model as M
import crc_model as K
from blocks_rig import CrcRig, crc_bufs, d64, u32, FILL, FMTS

pytestmark = pytest.mark.gpu
SMALL = [0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 255, 256, 4095, 4096, 4097]


@pytest.fixture(scope="module")
def fixture():
    return M.load()


def _i32(n, dev, fill=0):
    import torch
    return torch.full((max(1, n),), fill, dtype=torch.int32, device=dev)


class PlanRig:
    """a CrcDevPlan with device buffers that stay where they are"""

    def __init__(self, ctx, n, in_total_max, room):
        import torch
        import ms_compress_amd as m
        self.ctx, self.n, self.itm = ctx, n, in_total_max
        self.dev = dev = torch.device("cuda", ctx.device)
        self.plan = m.CrcDevPlan(ctx, n, in_total_max)
        self.d_in = torch.zeros(room + 64, dtype=torch.uint8, device=dev)
        self.d_off = torch.zeros(max(1, n), dtype=torch.int64, device=dev)
        self.d_len = torch.zeros(max(1, n), dtype=torch.int64, device=dev)
        self.d_crc, self.d_st = _i32(n, dev), _i32(n, dev)

    def run(self, mem, offs, lens):
        import torch
        self.d_in[: len(mem)].copy_(torch.from_numpy(mem))
        self.d_off.copy_(d64(offs, self.dev)); self.d_len.copy_(d64(lens, self.dev))
        self.d_crc.fill_(0x5A5A5A5A); self.d_st.fill_(77)
        self.plan.execute(self.d_in, self.d_off, self.d_len, self.d_crc, self.d_st)
        self.ctx.stream.synchronize()
        want, wst = K.units(mem, offs, lens, self.itm)
        got, st = u32(self.d_crc, self.n), self.d_st.cpu().numpy()[: self.n]
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, ("crc of units", [(int(i), int(offs[i]), int(lens[i]), hex(int(got[i])), hex(int(want[i]))) for i in bad[:8]])
        assert (st == wst).all()
        return got, st


def test_plan_one_batch_of_every_shape(gpu_ctx):
    row, slc = K.kernel_sizes()
    rs = np.random.RandomState(11)
    big1, big2 = (1 << 20) + 5, (16 << 20) + 3
    mem = rs.randint(0, 256, size=big2 + big1 + (4 << 20), dtype=np.uint8)
    offs, lens, pos = [], [], 0

    def place(n, align):
        nonlocal pos
        pos = (pos + 15) // 16 * 16 + align
        offs.append(pos); lens.append(n)
        pos += n
    for n in SMALL:                                               # every length at every start alignment
        for a in range(16):
            place(n, a)
    for n in (row - 1, row, row + 1, slc - 1, slc, slc + 1, 2 * row + 17, slc + row + 1):   # the kernel's own sizes
        for a in (0, 1, 15):
            place(n, a)
    place(big1, 3)                                                # spans many waves' slices
    place(big2, 5)                                                # the high bits of the exponent
    for k in range(5000):                                         # crosses the 1024-wide tiles of the table pass
        place(int(rs.randint(0, 41)), int(rs.randint(0, 16)))
    offs += [offs[-3] + 1, 100]; lens += [77, 3 * row + 9]       # two units that overlap others (and each other's neighbours)
    assert pos <= len(mem)
    order = rs.permutation(len(offs))                             # units out of address order
    offs, lens = [offs[i] for i in order], [lens[i] for i in order]
    rig = PlanRig(gpu_ctx, len(offs), sum(lens), len(mem))
    got, _ = rig.run(mem, offs, lens)
    assert int(got[list(order).index(0)]) == 0                    # (the first unit placed is empty)
    rig.plan.close()


def test_plan_known_answers_and_empty_plan(gpu_ctx):
    import ms_compress_amd as m
    assert m.crc32_units([b"123456789", b"", b"a"], ctx=gpu_ctx).tolist() == [0xCBF43926, 0, K.crc(b"a")]
    assert m.crc32_units([], ctx=gpu_ctx).tolist() == []
    rig = PlanRig(gpu_ctx, 0, 0, 16)                              # n_units = 0: nothing to do, and nothing written
    rig.plan.execute(rig.d_in, rig.d_off, rig.d_len, rig.d_crc, rig.d_st)
    gpu_ctx.stream.synchronize()
    rig.plan.close()
    # wrong plan kinds, both ways
    d = m.DevPlan(gpu_ctx, 2, 4, 1024, 1024)
    p = [t.data_ptr() for t in (rig.d_in, rig.d_off, rig.d_len, rig.d_crc, rig.d_st)]
    lib = gpu_ctx.lib
    assert lib.mscomp_amd_plan_execute_crc_dev(d._h, *p) == m.MSCOMP_ARG_ERROR
    c = m.CrcDevPlan(gpu_ctx, 4, 1024)
    q = p[0]
    assert lib.mscomp_amd_plan_execute_dev(c._h, q, q, q, q, q, q, q, q) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_plan_execute(c._h, q, q, q, q) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_plan_execute_size(c._h, q, q, q, q) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_plan_execute_size_dev(c._h, q, q, q, q, q, q, q) == m.MSCOMP_ARG_ERROR
    d.close(); c.close()


def test_null_required_arrays_are_refused(gpu_ctx, fixture):
    """a null required array is MSCOMP_ARG_ERROR before anything is enqueued; the optional ones (d_res_crc, d_range) may be null"""
    import ms_compress_amd as m
    lib = gpu_ctx.lib
    rig = PlanRig(gpu_ctx, 3, 1024, 1024)
    p = [t.data_ptr() for t in (rig.d_in, rig.d_off, rig.d_len, rig.d_crc, rig.d_st)]
    for k in range(5):
        q = list(p); q[k] = None
        assert lib.mscomp_amd_plan_execute_crc_dev(rig.plan._h, *q) == m.MSCOMP_ARG_ERROR, k
    assert lib.mscomp_amd_plan_execute_crc_dev(rig.plan._h, *p) == m.MSCOMP_OK
    rig.plan.close()
    bufs = crc_bufs(fixture, 2, 4096)
    r = CrcRig(gpu_ctx, 2, 4096, len(bufs), sum(len(b) for b in bufs))
    r.load(bufs)
    r.set_out([len(b) for b in bufs])
    a = [t.data_ptr() for t in (r.d_in, r.d_off, r.d_len, r.d_bcrc, r.d_rcrc, r.d_kst)]
    for k in (0, 1, 2, 3, 5):                                     # d_block_crc (3) with n_blocks_max > 0 included
        q = list(a); q[k] = None
        assert lib.mscomp_amd_blocks_crc(r.bk._h, *q) == m.MSCOMP_ARG_ERROR, k
    q = list(a); q[4] = None                                      # d_res_crc is optional
    assert lib.mscomp_amd_blocks_crc(r.bk._h, *q) == m.MSCOMP_OK
    r.check_crc(); r.compress()
    st, st2, _ = r.decode_and_check()
    assert st2 == [0] * r.n
    c = [t.data_ptr() for t in (r.d_out, r.d_ooff, r.d_len, r.d_first, r.d_range, r.d_bcrc, r.d_olen, r.d_dst)]
    for k in (0, 1, 2, 3, 5, 6, 7):
        q = list(c); q[k] = None
        assert lib.mscomp_amd_blocks_check(r.bk._h, *q) == m.MSCOMP_ARG_ERROR, k
    q = list(c); q[4] = None                                      # d_range is optional
    assert lib.mscomp_amd_blocks_check(r.bk._h, *q) == m.MSCOMP_OK
    gpu_ctx.stream.synchronize()
    assert not r.d_dst.cpu().numpy()[: r.n].any()
    r.close()


def test_plan_total_crosses_the_bound_mid_list(gpu_ctx):
    rs = np.random.RandomState(12)
    mem = rs.randint(0, 256, size=40000, dtype=np.uint8)
    lens = [100, 0, 5000, 4097, 1, 0, 300, 7]
    offs = [1, 0, 200, 6000, 11000, 0, 12000, 13001]
    rig = PlanRig(gpu_ctx, len(lens), 100 + 5000 + 4096, len(mem))    # the fourth unit crosses it by one byte
    got, st = rig.run(mem, offs, lens)
    assert st.tolist() == [0, 0, 0] + [M.ARG] * 5 and not got[3:].any() and got[0] != 0
    rig.plan.close()


def test_plan_five_executions_changed_in_place(gpu_ctx):
    """seeding and graph replay: data, offsets and lengths change behind the same pointers"""
    rs = np.random.RandomState(13)
    n, room = 300, 1 << 20
    rig = PlanRig(gpu_ctx, n, room, room)
    for k in range(5):
        mem = rs.randint(0, 256, size=room, dtype=np.uint8)
        lens = [int(x) for x in rs.randint(0, 3000 + 900 * k, size=n)]
        lens[7 * k] = 70000 + k
        offs = [int(x) for x in rs.randint(0, room - 80000, size=n)]
        if k == 3:
            lens[n // 2] = room                                   # ... and a running total that crosses the bound
        rig.run(mem, offs, lens)
    rig.plan.close()


@pytest.mark.parametrize("B", (4096, 65536))
@pytest.mark.parametrize("fmt", list(FMTS))
def test_container_crc_roundtrip_and_ranges(gpu_ctx, oracle, fixture, fmt, B):
    f = FMTS[fmt]
    bufs = crc_bufs(fixture, f, B)
    n, total = len(bufs), sum(len(b) for b in bufs)
    rig = CrcRig(gpu_ctx, f, B, n, total)
    rig.load(bufs)
    rig.check_crc()
    rig.compress()
    rig.set_out([len(b) for b in bufs])
    st, st2, _ = rig.decode_and_check()
    assert st == [0] * n and st2 == [0] * n
    nblk = [(len(b) + B - 1) // B for b in bufs]
    for rng in ((0, 1), "last", (1, 0), (1000, 5)):               # first block; the last, short block; an empty range; a range past the end
        ranges = [(max(0, k - 1), 1) for k in nblk] if rng == "last" else [rng] * n
        st, st2, _ = rig.decode_and_check(ranges)
        assert st == [0] * n and st2 == [0] * n, rng
    # a resource crc of None, and a second call on the same pointers (the call's own graph)
    rig.bk.crc(rig.d_in, rig.d_off, rig.d_len, rig.d_bcrc, rig.d_kst)
    rig.check_crc(); rig.check_crc()
    rig.close()


def test_container_crc_rejects_as_compress_does(gpu_ctx, oracle, fixture):
    f, B = 2, 4096
    bufs = crc_bufs(fixture, f, B)
    lens = [len(b) for b in bufs]
    cut = sum(lens[:9]) - 1
    rig = CrcRig(gpu_ctx, f, B, len(bufs), cut, in_room=sum(lens))
    rig.load(bufs)
    _, rc, st = rig.check_crc()
    assert st.tolist() == [0] * 8 + [M.ARG] * (len(bufs) - 8) and not rc[8:].any()
    rig.compress()
    rig.ctx.stream.synchronize()
    assert (rig.d_cst.cpu().numpy()[: rig.n] == st).all()
    rig.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_damage_that_the_decoders_accept(gpu_ctx, oracle, fixture, fmt):
    f, B = FMTS[fmt], 4096
    bufs = crc_bufs(fixture, f, B)
    n, lens, total = len(bufs), [len(b) for b in bufs], sum(len(b) for b in bufs)
    mp, mf, mo, ms = M.model_compress(oracle, f, bufs, B, total, total)
    raw = K.find_raw_block(mf, mo, lens, B)
    acc = K.find_accepted_corruption(oracle, f, mp, mf, mo, bufs, B)
    assert raw is not None and acc is not None, "every codec has a raw-block case and an accepted-corruption case"
    rig = CrcRig(gpu_ctx, f, B, n, total)
    rig.load(bufs)
    rig.check_crc()
    rig.compress()
    rig.set_out(lens)
    cases = [(raw[0], int(mo[raw[1]]), mp[int(mo[raw[1]])] ^ 0x10), acc]     # one bit inside a raw block; one byte inside a compressed one
    for r, pos, val in cases:
        hurt = rig.d_packed.clone()
        hurt[pos] = int(val)
        st, st2, olen = rig.decode_and_check(packed=hurt)
        assert st == [0] * n, "the decoder accepts the damage"
        assert st2 == [M.DATA if k == r else 0 for k in range(n)] and olen == [0 if k == r else lens[k] for k in range(n)]
    rig.close()


def test_check_leaves_failed_resources_alone(gpu_ctx, oracle, fixture):
    """statuses alone: a resource that is not MSCOMP_OK on entry keeps its status and its length, whatever its bytes are"""
    f, B = 3, 4096
    bufs = crc_bufs(fixture, f, B)
    n, lens = len(bufs), [len(b) for b in bufs]
    rig = CrcRig(gpu_ctx, f, B, n, sum(lens))
    rig.load(bufs)
    rig.check_crc()
    rig.compress()
    caps = list(lens); caps[8] -= 1                               # MSCOMP_BUF_ERROR from decompress: nothing of it was written
    rig.set_out(caps)
    st, st2, olen = rig.decode_and_check()
    assert st[8] == M.BUF and st2 == st and olen[8] == 0
    rig.d_bcrc[int(rig.d_first[3])] ^= 1                          # a wrong checksum for resource 3, and for resource 8, which is not looked at
    rig.d_bcrc[int(rig.d_first[8])] ^= 1
    st, st2, olen = rig.decode_and_check()
    assert st2 == [M.DATA if k == 3 else M.BUF if k == 8 else 0 for k in range(n)]
    # damaged block_first: checks 1 and 2 give decompress's statuses
    bad = rig.d_first.clone(); bad[n] = rig.nbmax + 1
    rig.d_dst.fill_(0); rig.d_olen.fill_(5)
    rig.bk.check(rig.d_out, rig.d_ooff, rig.d_len, bad, rig.d_bcrc, rig.d_olen, rig.d_dst)
    rig.ctx.stream.synchronize()
    assert int(rig.d_dst[n - 1]) == M.ARG and int(rig.d_olen[n - 1]) == 0
    rig.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_four_calls_in_one_captured_graph(gpu_ctx, oracle, fixture, fmt):
    import torch
    import ms_compress_amd as m
    f, B = FMTS[fmt], 65536
    base = crc_bufs(fixture, f, B)
    n, total = len(base), sum(len(b) for b in base)
    s = torch.cuda.Stream()
    ctx = m.Context(stream=s)
    with torch.cuda.stream(s):
        rig = CrcRig(ctx, f, B, n, total)
        rig.load(base)
        rig.set_out([len(b) for b in base])
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rig.bk.crc(rig.d_in, rig.d_off, rig.d_len, rig.d_bcrc, rig.d_kst, d_res_crc=rig.d_rcrc)
        rig.bk.compress(rig.d_in, rig.d_off, rig.d_len, rig.d_packed, rig.d_first, rig.d_boff, rig.d_cst, packed_cap=total)
        rig.bk.decompress(rig.d_packed, rig.d_first, rig.d_boff, rig.d_len, rig.d_out, rig.d_ooff, rig.d_ocap, rig.d_olen, rig.d_dst, packed_len=total)
        rig.bk.check(rig.d_out, rig.d_ooff, rig.d_len, rig.d_first, rig.d_bcrc, rig.d_olen, rig.d_dst)
    for k in range(3):
        bufs = base[k:] + base[:k]
        if k == 2:
            bufs = [b[: len(b) // 2] for b in bufs]
        with torch.cuda.stream(s):
            rig.load(bufs)
            rig.set_out([len(b) for b in bufs])
            rig.d_out.fill_(FILL); rig.d_bcrc.fill_(7); rig.d_rcrc.fill_(7)
            g.replay()
        s.synchronize()
        bc, rc, st = K.blocks(bufs, B, total)
        assert (u32(rig.d_bcrc, rig.nbmax) == bc).all() and (u32(rig.d_rcrc, n) == rc).all(), k
        out, olen, dst = rig.d_out.cpu().numpy(), rig.d_olen.cpu().numpy(), rig.d_dst.cpu().numpy()
        for r, b in enumerate(bufs):
            assert dst[r] == 0 and int(olen[r]) == len(b) and bytes(out[rig.ooff[r]: rig.ooff[r] + len(b)]) == b, (k, r)
    del g
    rig.close()
    ctx.close()


def test_python_conveniences(gpu_ctx, oracle, fixture):
    import ms_compress_amd as m
    f, B = 2, 4096
    bufs = crc_bufs(fixture, f, B)
    bc, rc = m.blocks_crc(f, bufs, B, ctx=gpu_ctx)
    wb, wr, _ = K.blocks(bufs, B, sum(len(b) for b in bufs))
    assert (bc == wb[: len(bc)]).all() and len(bc) == sum((len(b) + B - 1) // B for b in bufs) and (rc == wr).all()
    assert (m.crc32_units(bufs, ctx=gpu_ctx) == wr).all()
    packed, first, off, st = m.blocks_compress(f, bufs, B, ctx=gpu_ctx)
    got, dst = m.blocks_decompress(f, packed, first, off, [len(b) for b in bufs], B, ctx=gpu_ctx, block_crc=bc)
    assert dst == [0] * len(bufs) and got == bufs
    r, j = K.find_raw_block(first, off, [len(b) for b in bufs], B)
    hurt = packed.copy(); hurt[int(off[j])] ^= 0x80
    got, dst = m.blocks_decompress(f, hurt, first, off, [len(b) for b in bufs], B, ctx=gpu_ctx)
    assert dst == [0] * len(bufs) and got[r] != bufs[r]            # today's behaviour: the damage goes unnoticed
    got, dst = m.blocks_decompress(f, hurt, first, off, [len(b) for b in bufs], B, ctx=gpu_ctx, block_crc=bc)
    assert dst == [M.DATA if k == r else 0 for k in range(len(bufs))] and got[r] is None
    got, dst = m.blocks_decompress(f, hurt, first, off, [len(b) for b in bufs], B, ranges=[(0, 1)] * len(bufs), ctx=gpu_ctx, block_crc=bc)
    assert dst[r] == (M.DATA if j == int(first[r]) else 0)
