"""GPU: ms_compress_amd/device.py (DeviceBlocks, BlockOps) against the blocks_* host conveniences, at the smallest shapes at which its
plumbing can go wrong: B = 4096, four resources of 0, 1, 4096 and 2 * 4096 + 5 bytes -- an empty one, a one-byte block, a random block
that is stored raw, and soft data whose blocks are encoded, the last one short -- in a shape of 6 * 4096 bytes so that resize has room.
Every expected byte comes from blocks_compress + blocks_crc over data this file edits on the host with numpy. tests/test_device_sizes.py
proves the entry counts on the CPU; the canaries here watch the same thing on the device."""
import numpy as np
import pytest

from blocks_rig import FMTS, d64, memo, odd_offsets, rand, soft

pytestmark = pytest.mark.gpu

B, N, LENS, TOTAL = 4096, 4, (0, 1, 4096, 2 * 4096 + 5), 6 * 4096
# (resource, offset, length): inside a block, across a block boundary, clipped by the resource's end (96 bytes are left), into the empty resource
WRITES = ((3, 100, 50), (3, 4090, 20), (2, 4000, 200), (0, 0, 10))
WANTS = (50, 20, 96, 0)
SRC_OFF = (1, 67, 131, 400)                                     # where each request's bytes lie in d_src: any alignment
WANT_LEN = (0, 1 + 2 * B + 7, 4096, 5000)                       # extended by two blocks and 7 bytes, left alone, cut inside its second block


def make_bufs(seed):
    return [b"", rand(seed, 1), rand(seed + 1, 4096), soft(seed + 2, 2 * 4096 + 5)]


def make_src(seed):
    """(the payload of every request, the buffer they lie in at SRC_OFF)"""
    pay = [rand(seed + 10 + q, ln) for q, (_, _, ln) in enumerate(WRITES)]
    blob = np.full(700, 0x5A, dtype=np.uint8)
    for o, p in zip(SRC_OFF, pay):
        blob[o: o + len(p)] = np.frombuffer(p, dtype=np.uint8)
    return pay, blob


def written(bufs, pay, writes=WRITES):
    """the data after the writes, on the host: each clipped to its resource, in request order"""
    out = [bytearray(b) for b in bufs]
    for (r, o, ln), p in zip(writes, pay):
        if r < len(out):
            o = min(o, len(out[r]))
            w = min(ln, len(out[r]) - o)
            out[r][o: o + w] = p[:w]
    return [bytes(b) for b in out]


def resized(bufs, want=WANT_LEN):
    return [b[:w] + bytes(max(0, w - len(b))) for b, w in zip(bufs, want)]


def same_container(got, want, what):
    """two containers as host() and the conveniences give them: packed bytes, block_first, block_off, lengths, checksums -- entry for entry"""
    for k, name in enumerate(("packed", "block_first", "block_off", "lengths", "block_crc")):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and (a == b).all(), (what, name)


@pytest.fixture(scope="module")
def expected(gpu_ctx):
    """get(fmt, bufs as a tuple) = (packed, block_first, block_off, lengths, block_crc) from blocks_compress + blocks_crc, made once per data"""
    import ms_compress_amd as m

    def make(fmt, bufs):
        packed, first, off, st = m.blocks_compress(fmt, list(bufs), B, ctx=gpu_ctx)
        crc, _ = m.blocks_crc(fmt, list(bufs), B, ctx=gpu_ctx)
        assert not st.any()
        return packed, first, off, [len(b) for b in bufs], crc
    yield from memo(make)


class Inputs:
    """the device tensors a chain reads: the data at odd offsets, its tables, the requests and their payload; load() overwrites them in place"""

    def __init__(self, dev):
        import torch
        self.dev = dev
        self.d_data = torch.zeros(TOTAL + 64, dtype=torch.uint8, device=dev)
        self.d_off, self.d_len = d64([], dev, N), d64(LENS, dev)
        self.d_req, self.d_src_off = d64(np.array(WRITES, dtype=np.uint64).reshape(-1), dev), d64(SRC_OFF, dev)
        self.d_src = torch.zeros(700, dtype=torch.uint8, device=dev)
        self.d_want = d64(WANT_LEN, dev)

    def load(self, seed):
        import torch
        self.bufs = make_bufs(seed)
        self.pay, blob = make_src(seed)
        off, data = odd_offsets(self.bufs, self.d_data.numel())
        self.d_data.copy_(torch.from_numpy(data).to(self.dev))
        self.d_off.copy_(d64(off, self.dev, N))
        self.d_src.copy_(torch.from_numpy(blob).to(self.dev))
        self.final = resized(written(self.bufs, self.pay))
        return self


def chain(ops, x):
    """compress, write, resize, delta against the first container, patch: every container and result on the way"""
    a = ops.compress(x.d_data, x.d_off, x.d_len)
    b, d_wr, d_st = ops.write(a, x.d_req, x.d_src, x.d_src_off)
    c = ops.resize(b, x.d_want)
    d, df = ops.delta(a, c)
    p = ops.patch(a, d, df)
    return {"a": a, "b": b, "c": c, "d": d, "p": p, "df": df, "written": d_wr, "status": d_st}


def check_chain(got, x, fmt, expected):
    for name in "abcdp":
        assert not got[name].status.cpu().numpy()[:N].any(), name
    assert got["written"].cpu().tolist()[:4] == list(WANTS) and not got["status"].cpu().numpy().any()       # the empty resource: 0 bytes, MSCOMP_OK
    assert not got["df"].status.cpu().numpy()[:N].any()
    want = expected(fmt, tuple(x.final))
    same_container(got["c"].host(), want, "the resized container")
    same_container(got["p"].host(), got["c"].host(), "the patched container against the resized one")
    same_container(got["p"].host(), want, "the patched container")
    same_container(got["a"].host(), expected(fmt, tuple(x.bufs)), "the first container")
    same_container(got["b"].host(), expected(fmt, tuple(written(x.bufs, x.pay))), "the written container")
    # the delta holds what changed and nothing else: resource 2's one block, resource 1's three, resource 3's two
    count = got["df"].count.cpu().tolist()
    assert got["df"].changed.cpu().tolist()[:N] == [0, 3, 1, 2] and count[0] == 6 and count[1] == 6 and count[2] == got["d"].packed_len()


@pytest.fixture(scope="module")
def dev(gpu_ctx):
    import torch
    return torch.device("cuda", gpu_ctx.device)


@pytest.mark.parametrize("fmt", list(FMTS))
def test_compress_is_blocks_compress_and_decompress_gives_the_data_back(gpu_ctx, dev, expected, fmt):
    import ms_compress_amd as m
    ops = m.BlockOps(gpu_ctx, FMTS[fmt], B, N, TOTAL)
    x = Inputs(dev).load(3)
    a = ops.compress(x.d_data, x.d_off, x.d_len)
    want = expected(FMTS[fmt], tuple(x.bufs))
    same_container(a.host(), want, "compress")
    stored = np.diff(want[2].astype(np.int64))
    assert stored[1] == 4096 and (stored[2:] < 4096).all()                     # the random block is stored raw, the soft ones encoded
    assert a.packed_len() == len(a.host()[0]) == len(want[0]) and a.cap == TOTAL and a.view()[5:] == (TOTAL, N, N + TOTAL // B)
    d_out, d_off, d_len, d_st = ops.decompress(a)
    out, off = d_out.cpu().numpy(), d_off.cpu().tolist()
    assert d_st.cpu().tolist()[:N] == [0] * N and d_len.cpu().tolist()[:N] == list(LENS) and off == [0, 0, 16, 16 + 4096, 16 + 4096 + 8208]
    for r, b in enumerate(x.bufs):
        assert bytes(out[off[r]: off[r] + len(b)]) == b, r
    # one block of each resource that has a second one: resource 3's bytes [4096, 8192)
    d_out, d_off, d_len, d_st = ops.decompress(a, d_range=d64([0, 0, 0, 1, 0, 1, 1, 1], dev))
    out, off = d_out.cpu().numpy(), d_off.cpu().tolist()
    assert d_st.cpu().tolist()[:N] == [0] * N and d_len.cpu().tolist()[:N] == [0, 1, 4096, 4096]
    assert bytes(out[off[3]: off[3] + 4096]) == x.bufs[3][4096: 8192] and bytes(out[off[2]: off[2] + 4096]) == x.bufs[2]
    # a flipped stored byte of the raw block decodes, and only the check against the checksums tells
    a.packed[int(want[2][1]) + 7] ^= 0xFF
    assert ops.decompress(a, check=False)[3].cpu().tolist()[:N] == [0] * N
    assert ops.decompress(a)[3].cpu().tolist()[:N] == [0, 0, m.MSCOMP_DATA_ERROR, 0]
    ops.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_the_chain_stays_on_the_device_and_every_table_keeps_its_canaries(gpu_ctx, dev, expected, fmt):
    """compress, write, resize, delta, patch through a BlockOps whose every tensor lies between 64 bytes of 0xA5 in front and behind: the
    patched container is the resized one and both are blocks_compress + blocks_crc of the data edited on the host, the two edited ranges
    read back as written, and no canary byte changed"""
    import torch
    import ms_compress_amd as m
    guards = []

    class Guarded(m.BlockOps):
        def _alloc(self, name, entries, dtype, fill=0):
            size = max(1, int(entries)) * np.dtype(dtype).itemsize
            raw = torch.full((64 + (size + 63) // 64 * 64 + 64,), 0xA5, dtype=torch.uint8, device=dev)
            guards.append((name, raw, size))
            t = raw[64: 64 + size].view(getattr(torch, dtype))
            return t if fill is None else t.fill_(fill)

    ops = Guarded(gpu_ctx, FMTS[fmt], B, N, TOTAL)
    x = Inputs(dev).load(5)
    got = chain(ops, x)
    check_chain(got, x, FMTS[fmt], expected)
    d_out, d_off, d_len, d_st = ops.read(got["p"], d64(np.array(WRITES[:2], dtype=np.uint64).reshape(-1), dev), 50)
    out = d_out.cpu().numpy()
    assert d_st.cpu().tolist() == [0, 0] and d_len.cpu().tolist() == [50, 20] and d_off.cpu().tolist() == [0, 64]
    assert bytes(out[:50]) == x.pay[0] and bytes(out[64: 84]) == x.pay[1]
    gpu_ctx.stream.synchronize()
    assert len(guards) >= 40
    for name, raw, size in guards:
        h = raw.cpu().numpy()
        assert (h[:64] == 0xA5).all() and (h[64 + size:] == 0xA5).all(), (name, size)
    ops.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_the_chain_in_one_captured_graph(expected, fmt):
    """the same chain captured once on a stream of its own -- a synchronisation or a fetch inside would fail the capture --, replayed, and
    replayed again over other data and another payload written into the same tensors"""
    import torch
    import ms_compress_amd as m
    s = torch.cuda.Stream()
    ctx = m.Context(stream=s)
    ops = m.BlockOps(ctx, FMTS[fmt], B, N, TOTAL)
    with torch.cuda.stream(s):
        x = Inputs(torch.device("cuda", ctx.device)).load(7)
    ops.prepare("write", n_req=len(WRITES))
    s.synchronize()
    with ops.graph("container", "write", "resize", "diff", "splice_extents") as g:
        got = chain(ops, x)
    for seed in (7, 11):
        with torch.cuda.stream(s):
            x.load(seed)
            g.replay()
        s.synchronize()
        check_chain(got, x, FMTS[fmt], expected)
    with pytest.raises(ValueError):                              # a context on the default stream cannot capture
        with m.BlockOps(m.Context(), FMTS[fmt], B, N, TOTAL).graph("container"):
            pass
    del g, got
    ops.close()
    ctx.close()


def test_per_request_errors_stay_in_the_status_tensor(gpu_ctx, dev, expected):
    """A writer whose budget is one block short of the requests' four, and a request that names resource n_res: both get MSCOMP_ARG_ERROR in
    d_status, nothing raises, and the other requests are applied. blocks_write sizes its own budget from its requests, so it is fed the
    same list without the request the budget refuses: its container is the layer's, and its answers to the three are the layer's."""
    import torch
    import ms_compress_amd as m
    fmt = FMTS["xpress"]
    reqs = [(3, 100, 50), (3, 4090, 20), (N, 0, 10), (2, 0, 10)]                # 1 block, 2 blocks, no such resource, 1 block: over a budget of 3
    pay = [rand(40 + q, ln) for q, (_, _, ln) in enumerate(reqs)]
    ops = m.BlockOps(gpu_ctx, fmt, B, N, TOTAL)
    ops.prepare("write", n_req=4, blocks_max=3)
    x = Inputs(dev).load(9)
    blob = np.zeros(256, dtype=np.uint8)
    for q, p in enumerate(pay):
        blob[64 * q: 64 * q + len(p)] = np.frombuffer(p, dtype=np.uint8)
    a = ops.compress(x.d_data, x.d_off, x.d_len)
    b, d_wr, d_st = ops.write(a, d64(np.array(reqs, dtype=np.uint64).reshape(-1), dev), torch.from_numpy(blob).to(dev), d64([0, 64, 128, 192], dev))
    assert d_st.cpu().tolist() == [0, 0, m.MSCOMP_ARG_ERROR, m.MSCOMP_ARG_ERROR] and d_wr.cpu().tolist() == [50, 20, 0, 0]
    assert not b.status.cpu().numpy().any()
    host = a.host()
    packed, off, crc, wr, st, rst = m.blocks_write(fmt, *host[:4], B, [(r, o, p) for (r, o, _), p in zip(reqs[:3], pay)], ctx=gpu_ctx, block_crc=host[4])
    assert (wr, st, rst) == ([50, 20, 0], [0, 0, m.MSCOMP_ARG_ERROR], [0] * N)
    same_container(b.host(), (packed, host[1], off, host[3], crc), "the written container")
    same_container(b.host(), expected(fmt, tuple(written(x.bufs, pay, reqs[:3]))), "the written container against the edited data")
    ops.close()


def test_a_container_of_another_shape_is_refused(gpu_ctx, dev):
    import ms_compress_amd as m
    fmt = FMTS["lznt1"]
    ops, wider = m.BlockOps(gpu_ctx, fmt, B, N, TOTAL), m.BlockOps(gpu_ctx, fmt, B, N, TOTAL + B)
    x = Inputs(dev).load(13)
    a, other = ops.compress(x.d_data, x.d_off, x.d_len), wider.compress(x.d_data, x.d_off, x.d_len)
    assert other.n_blocks_table == a.n_blocks_table + 1
    for call in (lambda: ops.decompress(other), lambda: ops.resize(other, x.d_want), lambda: ops.write(other, x.d_req, x.d_src, x.d_src_off),
                 lambda: ops.delta(a, other), lambda: ops.splice([a, other], d64([0, 0] * N, dev)), lambda: ops.resize(a, x.d_want[:3])):
        with pytest.raises(ValueError):
            call()
    # from_host into the shape, and out of it
    up = m.DeviceBlocks.from_host(gpu_ctx, fmt, B, a.host(), n_blocks_table=ops.n_blocks_max, cap=TOTAL)
    assert up.packed_len() == a.packed_len() == len(a.host()[0])
    same_container(ops.resize(up, x.d_len).host(), a.host(), "a container uploaded and carried through a resize that changes nothing")
    with pytest.raises(ValueError):
        ops.resize(m.DeviceBlocks.from_host(gpu_ctx, fmt, B, a.host()), x.d_len)
    # a splice of whole resources: reversed
    sp = ops.splice([a], d64([0, 3, 0, 2, 0, 1, 0, 0], dev))
    assert sp.host()[3] == list(LENS)[::-1] and not sp.status.cpu().numpy().any()
    ops.close()
    wider.close()
