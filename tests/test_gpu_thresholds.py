"""GPU: the encoders at their raw / fallback decisions. Every case of tests/golden/thresholds.json (recipes, tests/thresholds.py) is rebuilt,
the oracle's live probe must report the recorded delta, and the GPU's bytes must be the oracle's bytes with the SHA-256 the compiled reference
gave when the fixture was made. Reads the repository and oracle/ only.

LZNT1 (a chunk is stored raw when its body would not be shorter) and Xpress+Huffman (a chunk whose estimate passes its limit is written again as
literals with the package-merge code) have such a switch. Plain Xpress has none, so it is not here.
"""
import hashlib
import random

import numpy as np
import pytest

import thresholds as T

pytestmark = pytest.mark.gpu
BUF_ERROR = -5
XH_FB_BLOCKS = 256                                           # csrc/launch.hip: the grid of the fallback kernel


@pytest.fixture(scope="module")
def fx(oracle):
    """per codec: [(case, input, oracle's bytes)], each checked against the live probe and the recorded reference digest"""
    out = {"xh": [], "lznt1": [], "lznt1_sa": []}
    for c in T.load()["cases"]:
        data = T.build(c)
        d, rec, _ = T.probe(oracle, c, data)
        assert d == c["want"] and rec == c["record"], (c["id"], d, rec)
        st, exp = T.oracle_compress(oracle, c, data)
        assert st == 0 and hashlib.sha256(exp).hexdigest() == c["ref_sha256"], c["id"]
        out[c["codec"]].append((c, data, exp))
    sides = [T.switched(c, c["want"]) for c, _, _ in out["xh"]]
    assert any(sides) and not all(sides)
    for k in out:                                            # both sides of the boundary interleaved in the batch
        a = [x for x in out[k] if T.switched(x[0], x[0]["want"])]
        b = [x for x in out[k] if not T.switched(x[0], x[0]["want"])]
        mixed = []
        while a or b:
            if a:
                mixed.append(a.pop())
            if b:
                mixed.append(b.pop())
        out[k] = mixed
    return out


def _check(m, ctx, fmt, items, what, decode=True):
    got, st = m.compress_units(fmt, [d for _, d, _ in items], ctx=ctx)
    for (c, data, exp), g, s in zip(items, got, st):
        assert s == 0 and g == exp, "%s %s: GPU bytes differ from the oracle's (delta %+d)" % (what, c["id"], c["want"])
        assert hashlib.sha256(g).hexdigest() == c["ref_sha256"], (what, c["id"])
    if decode:                                               # fallback chunks and raw chunks at the boundary through the decoders
        back, st2 = m.decompress_units(fmt, got, [len(d) for _, d, _ in items], ctx=ctx)
        for (c, data, exp), b, s in zip(items, back, st2):
            assert s == 0 and (b or b"") == data, "%s %s: round trip" % (what, c["id"])


@pytest.mark.parametrize("codec", ["lznt1", "xh"])
def test_decision_thresholds(oracle, gpu_ctx, fx, codec):
    """all cases of a codec in one batch through the batch plan; for Xpress+Huffman also batches in which every chunk falls back, none does,
    and more chunks fall back than the fallback kernel has blocks"""
    import ms_compress_amd as m
    fmt = T.CODECS[codec]
    _check(m, gpu_ctx, fmt, fx[codec], "batch")
    if codec != "xh":
        return
    single = [x for x in fx["xh"] if x[0]["length"] <= T.XH_CHUNK]
    yes = [x for x in single if T.switched(x[0], x[0]["want"])]
    no = [x for x in single if not T.switched(x[0], x[0]["want"])]
    assert len(yes) >= 8 and len(no) >= 8
    _check(m, gpu_ctx, fmt, yes, "all fall back")
    _check(m, gpu_ctx, fmt, no, "none falls back")
    many = []
    for k in range(XH_FB_BLOCKS + 40):                       # the kernel's `it += gridDim.x` loop turns
        c = {"id": "random-%d" % k, "codec": "xh", "seed": 7000 + k, "length": T.XH_CHUNK, "plants": [], "chunk": 0}
        data = T.build(c)
        d, rec, _ = T.probe(oracle, c, data)
        exp = oracle.oracle_compress(fmt, data)[1]
        many.append((dict(c, want=d, ref_sha256=hashlib.sha256(exp).hexdigest()), data, exp))
    assert sum(1 for c, _, _ in many if c["want"] >= 1) > XH_FB_BLOCKS
    _check(m, gpu_ctx, fmt, many + yes[:4] + no[:4], "more fallback chunks than blocks", decode=False)


@pytest.mark.parametrize("mode", [1, 2])
def test_lznt1_chunk_kernels(gpu_ctx, fx, mode):
    import ms_compress_amd as m
    gpu_ctx.lib.mscomp_amd_debug_set_lznt1(mode)
    try:
        _check(m, gpu_ctx, 2, fx["lznt1"], "chunk kernel %d" % mode, decode=False)
    finally:
        gpu_ctx.lib.mscomp_amd_debug_set_lznt1(0)


def test_lznt1_suffix_array_flavour(fx):
    import ms_compress_amd as m
    ctx = m.Context()
    try:
        ctx.set_lznt1_sa_dict(True)
        _check(m, ctx, 2, fx["lznt1_sa"], "suffix-array flavour")
    finally:
        ctx.close()


@pytest.mark.parametrize("finder", [1, 2])
def test_xpress_huff_finders(gpu_ctx, fx, finder):
    """extra and the counts reach xh_huff_kernel by two routes"""
    import ms_compress_amd as m
    gpu_ctx.lib.mscomp_amd_debug_set_finder(finder)
    try:
        _check(m, gpu_ctx, 4, fx["xh"], "finder %d" % finder, decode=False)
    finally:
        gpu_ctx.lib.mscomp_amd_debug_set_finder(1)


@pytest.mark.parametrize("codec", ["lznt1", "xh", "lznt1_sa"])
def test_one_shot_call(fx, codec):
    """the drop-in one-shot call (ms_compress, host pointers)"""
    import ms_compress_amd as m
    lib = m.load_library()
    lib.mscomp_amd_set_lznt1_sa_dict(1 if codec == "lznt1_sa" else 0)
    try:
        for c, data, exp in fx[codec]:
            assert m.compress(T.CODECS[codec], data) == exp, c["id"]
    finally:
        lib.mscomp_amd_set_lznt1_sa_dict(0)


@pytest.mark.parametrize("codec", ["lznt1", "xh"])
def test_compress_dev_plan(gpu_ctx, fx, codec):
    """a compress plan with device tables: the size of a chunk that flipped is consumed on the device"""
    import torch
    import ms_compress_amd as m
    fmt = T.CODECS[codec]
    items = fx[codec]
    lens = [len(d) for _, d, _ in items]
    in_off, in_total = m.pack_offsets(lens)
    caps = [m.max_compressed_size(fmt, n) + 2 for n in lens]
    out_off, out_total = m.pack_offsets(caps)
    blob = np.zeros(in_total + 16, np.uint8)
    for (_, d, _), o in zip(items, in_off):
        blob[int(o): int(o) + len(d)] = np.frombuffer(d, np.uint8)
    n = len(items)
    dt = lambda a: torch.from_numpy(np.asarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()
    with torch.cuda.stream(gpu_ctx.stream):
        d_in = torch.from_numpy(blob).cuda()
        d_out = torch.zeros(out_total + 16, dtype=torch.uint8, device="cuda")
        d_len = torch.zeros(n, dtype=torch.int64, device="cuda")
        d_st = torch.full((n,), 77, dtype=torch.int32, device="cuda")
        plan = m.CompressDevPlan(gpu_ctx, fmt, n, in_total + 16, max(lens))
        plan.execute(d_in, dt(in_off), dt(lens), d_out, dt(out_off), dt(caps), d_len, d_st)
        gpu_ctx.stream.synchronize()
    torch.cuda.synchronize()
    h_out, h_len, h_st = d_out.cpu().numpy(), d_len.cpu().numpy(), d_st.cpu().numpy()
    plan.close()
    for i, (c, data, exp) in enumerate(items):
        o = int(out_off[i])
        assert h_st[i] == 0 and bytes(h_out[o: o + int(h_len[i])]) == exp, c["id"]


@pytest.mark.parametrize("codec", ["lznt1", "xh"])
def test_capacities_at_the_boundary(oracle, gpu_ctx, fx, codec):
    """cap = size and cap = size - 1 for the cases either side of the switch: a chunk that flips changes the size the capacity is checked against"""
    import ms_compress_amd as m
    fmt = T.CODECS[codec]
    near = (0, 1, 2) if codec == "xh" else (-1, 0)
    units, caps, want = [], [], []
    for c, data, exp in fx[codec]:
        if c["want"] in near:
            for name, cap in (("size", len(exp)), ("size-1", len(exp) - 1)):
                st, out = T.oracle_compress(oracle, c, data, cap)
                assert st == c["ref_cap_status"][name]
                units.append(data); caps.append(cap); want.append((c["id"], name, st, out))
    assert len(units) >= 24
    got, sts = m.compress_units(fmt, units, ctx=gpu_ctx, capacities=caps)
    for (cid, name, st, out), g, s in zip(want, got, sts):
        assert s == st and (st != 0 or g == out), (cid, name, s, st)
    assert {w[2] for w in want} == {0, BUF_ERROR}


def test_huffman_slow_builder_stage(oracle, gpu_ctx, fx):
    """mscomp_amd_debug_huff_lengths_slow (the fallback kernel's own package-merge: counts on the symbols 0..0x100 only, its pool is sized for
    257 leaves) against orc_huff_lengths_slow, which tests/test_oracle_vs_ref.py pins to the reference's CreateCodesSlow; Kraft equality as a
    check that does not lean on the oracle"""
    hs = [list(h) for h in T.seeded_histograms()]
    n_seeded = len(hs)
    for c, data, exp in fx["xh"]:                            # the histogram of every fallback chunk of the fixture
        for k, r in enumerate(oracle.xpress_huff_decisions(data)):
            if r["fell_back"]:
                h = np.bincount(np.frombuffer(data[k * T.XH_CHUNK: k * T.XH_CHUNK + r["n"]], np.uint8), minlength=512)
                h[0x100] = r["last"]
                hs.append(h.tolist())
    assert len(hs) > n_seeded + 20
    rnd = random.Random(3)
    for _ in range(40):                                      # counts of 1..3 over 100..257 symbols: ties everywhere
        k = rnd.randint(100, 257)
        c = [rnd.randint(1, 3) for _ in range(k)] + [0] * (257 - k)
        rnd.shuffle(c)
        hs.append(c + [0] * 255)
    allc = np.ascontiguousarray(hs, dtype=np.uint32)
    assert allc.shape[1] == 512 and not allc[:, 0x101:].any()
    lens = np.full((len(allc), 512), 0xEE, dtype=np.uint8)
    assert gpu_ctx.lib.mscomp_amd_debug_huff_lengths_slow(gpu_ctx._h, allc.ctypes.data, len(allc), lens.ctypes.data) == 0
    lib = oracle.load_oracle()
    digests = T.load()["huff_slow_sha256_16"]
    deep = 0
    for i in range(len(allc)):
        want = np.zeros(512, dtype=np.uint8)
        lib.orc_huff_lengths_slow(allc[i].ctypes.data, want.ctypes.data)
        if not np.array_equal(lens[i], want):
            s = int(np.nonzero(lens[i] != want)[0][0])
            raise AssertionError("histogram %d: symbol %d got length %d, CreateCodesSlow gives %d" % (i, s, lens[i][s], want[s]))
        if i < n_seeded:
            assert hashlib.sha256(lens[i].tobytes()).hexdigest()[:16] == digests[i], i
        if (allc[i] > 0).sum() >= 2:
            assert sum(2 ** (15 - int(x)) for x in lens[i] if x) == 2 ** 15, i
        deep += int(want.max() == 15)
    assert deep >= 8                                         # the length limit did the work
    bad = allc[:1].copy()
    bad[0, 0x150] = 1                                        # a symbol the pool has no room for is refused, not run
    assert gpu_ctx.lib.mscomp_amd_debug_huff_lengths_slow(gpu_ctx._h, bad.ctypes.data, 1, lens.ctypes.data) == -2
