"""GPU: the block transcoder (mscomp_amd_transcoder_*) against tests/transcode_model.py -- packed bytes, tables, checksums, statuses and
counts --, at the smallest shapes that reach each rule of the header; the new container is decoded again with its new checksums. The
source containers are the model's (the oracle's bytes), so every comparison is with the reference's stream."""
import numpy as np
import pytest

import blocks_model as M
import thresholds as T
import transcode_model as X
from blocks_rig import NewContainer, d64, d8, i32, mixed, rand, text

pytestmark = pytest.mark.gpu
LZNT1, XPRESS, XHUFF = 2, 3, 4


def threshold_chunks(count):
    """LZNT1 chunks of 4096 bytes whose image is 4096 or 4097 bytes although the encoder did not fall back: the boundary chunks of the
    entries of tests/golden/thresholds.json whose body is one or two bytes shorter than the chunk"""
    out = [T.build(c)[c["chunk"] * 4096: c["chunk"] * 4096 + 4096] for c in T.load()["cases"]
           if c["codec"] == "lznt1" and c["want"] in (-1, -2) and c["record"]["n"] == 4096]
    assert len(out) >= count
    return out[:count]


class Source:
    """a container as mscomp_amd_blocks_compress and mscomp_amd_blocks_crc write it, from the model"""

    def __init__(self, oracle, fmt, B, bufs, with_crc=True):
        self.fmt, self.B, self.bufs, self.lens = fmt, B, list(bufs), [len(b) for b in bufs]
        self.packed, self.first, self.off, self.crc = X.fresh(oracle, fmt, self.bufs, B, with_crc)
        self.nbt = len(self.off) - 1


class Case:
    """the arguments of one call: a source, the new format and block size, and the bounds -- by default the ones that refuse nothing"""

    def __init__(self, src, f2, B2, nbn=None, gmax=None, cap=None, packed=None, first=None, lens=None, with_crc=True):
        G = max(src.B, B2)
        self.src, self.f2, self.B2 = src, f2, B2
        self.lens = src.lens if lens is None else lens
        self.first = src.first if first is None else first
        self.packed = src.packed if packed is None else packed
        self.n = len(self.lens)
        self.nbn = sum((x + B2 - 1) // B2 for x in src.lens) if nbn is None else nbn
        self.gmax = sum((x + G - 1) // G for x in src.lens) if gmax is None else gmax
        self.cap = sum(src.lens) if cap is None else cap
        self.crc = src.crc if with_crc else None

    def model(self, oracle):
        s = self.src
        return X.transcode(oracle, s.fmt, s.B, self.f2, self.B2, self.packed, len(self.packed), self.first, s.off, self.lens, self.crc, s.nbt, self.nbn,
                           self.gmax, self.cap)


class Run(Case):
    """one transcoder and its device arrays; go() executes it and fetches everything it wrote"""

    def __init__(self, ctx, src, f2, B2, **kw):
        import torch
        import ms_compress_amd as m
        Case.__init__(self, src, f2, B2, **kw)
        self.ctx = ctx
        self.dev = dev = torch.device("cuda", ctx.device)
        with torch.cuda.device(ctx.device), torch.cuda.stream(ctx.stream):
            self.tc = m.BlockTranscoder(ctx, src.fmt, src.B, f2, B2, self.n, src.nbt, self.nbn, self.gmax)
            self.d_packed, self.d_first, self.d_off, self.d_len = d8(self.packed, dev), d64(self.first, dev), d64(src.off, dev), d64(self.lens, dev)
            self.d_crc = None if self.crc is None else i32(np.concatenate([self.crc, np.zeros(1, np.uint32)]), dev)
            self.out = NewContainer(dev, self.n, self.nbn, sum(src.lens), crc=self.crc is not None, lens=False, fill=-77)

    def launch(self):
        d_new, d_nfirst, d_noff, d_ncrc, _, d_st = self.out.tensors()
        self.tc.transcode(self.d_packed, self.d_first, self.d_off, self.d_len, d_new, d_nfirst, d_noff, d_st, d_block_crc=self.d_crc,
                          d_new_block_crc=d_ncrc, packed_len=len(self.packed), new_cap=self.cap)

    def poison(self):
        self.out.fill()

    def fetch(self):
        """everything the call wrote, whole (NewContainer.pull): the status and checksum arrays have one entry at least"""
        self.ctx.stream.synchronize()
        return self.out.pull()

    def go(self):
        import torch
        with torch.cuda.device(self.ctx.device), torch.cuda.stream(self.ctx.stream):
            self.poison()
            self.launch()
            got = self.fetch()
            got["counts"] = self.tc.counts()
        return got

    def close(self):
        self.tc.close()


def same(got, want):
    """everything the call wrote against the model's tuple, sentinels and the whole image included (NewContainer.compare)"""
    packed, first, off, crc, status, counts = want
    NewContainer.compare(got, dict(packed=packed, first=first, off=off, crc=crc, status=status), "transcoded", len(status), len(off) - 1,
                         crc=crc is not None, fills=(-77, -77, -77))
    assert got["counts"] == counts


def check(ctx, oracle, src, f2, B2, with_crc=True, **kw):
    """run, compare with the model and -- where every resource is accepted -- with a fresh compression, and decode the result again"""
    import ms_compress_amd as m
    run = Run(ctx, src, f2, B2, with_crc=with_crc, **kw)
    got, want = run.go(), run.model(oracle)
    run.close()
    same(got, want)
    got["status"] = got["status"][: run.n]                          # (without resources the one entry still holds its fill: compared above)
    if run.n and got["status"] == [0] * run.n and not kw:
        packed, first, off, crc = X.fresh(oracle, f2, src.bufs, B2, with_crc)
        nb = int(first[-1])
        assert bytes(got["image"][: len(packed)]) == packed and (got["first"] == first).all() and (got["off"][: nb + 1] == off).all()
        assert crc is None or (got["crc"][:nb] == crc).all()
        back, st = m.blocks_decompress(f2, got["image"][: len(packed)], got["first"], got["off"][: nb + 1], src.lens, B2, ctx=ctx,
                                       block_crc=None if crc is None else got["crc"][:nb])
        assert st == [0] * run.n and back == src.bufs
    return got


@pytest.mark.parametrize("B2", [8192, 65536])
def test_join_text_is_carried(gpu_ctx, oracle, B2):
    src = Source(oracle, LZNT1, 4096, [text(1, 3 * B2), text(2, B2 + 4096 + 700), text(3, 4096), b""])
    for with_crc in (False, True):
        got = check(gpu_ctx, oracle, src, LZNT1, B2, with_crc)
        nb_new = sum((n + B2 - 1) // B2 for n in src.lens)
        assert got["counts"] == (nb_new, 0, 0)


@pytest.mark.parametrize("with_crc", [False, True], ids=["plain", "crc"])
def test_join_mixed_is_worked(gpu_ctx, oracle, with_crc):
    """4 KiB blocks by turns random and text: every 8 KiB block has a raw-stored member; beside them carried text and a short raw tail"""
    src = Source(oracle, LZNT1, 4096, [mixed(4, 5 * 4096 + 7), text(5, 2 * 8192), mixed(6, 8 * 4096, period=4), text(7, 8192 + 5)])
    got = check(gpu_ctx, oracle, src, LZNT1, 8192, with_crc)
    assert got["counts"][0] > 0 and got["counts"][1] > 0 and got["counts"][2] > 0
    got = check(gpu_ctx, oracle, src, LZNT1, 32768, with_crc)
    assert got["counts"][1] > 0 and got["counts"][2] > 0


def test_join_random_is_encoded(gpu_ctx, oracle):
    src = Source(oracle, LZNT1, 4096, [rand(8, 3 * 8192 + 1), rand(9, 4096)])
    got = check(gpu_ctx, oracle, src, LZNT1, 8192)
    assert got["counts"] == (0, 0, 5)


@pytest.mark.parametrize("sizes", [(65536, 4096), (524288, 32768)], ids=["64k-4k", "512k-32k"])
def test_split(gpu_ctx, oracle, sizes):
    B1, B2 = sizes
    # text: carried, nothing decoded without checksums; with them every compressed-stored source block is decoded
    src = Source(oracle, LZNT1, B1, [text(10, B1 + 3 * B2 + 11), text(11, B2 - 1)])
    nb_new = sum((n + B2 - 1) // B2 for n in src.lens)
    got = check(gpu_ctx, oracle, src, LZNT1, B2, False)
    assert got["counts"] == (nb_new - 1, 1, 0)                     # (the tail of 11 bytes does not shrink: its source block is decoded once)
    got = check(gpu_ctx, oracle, src, LZNT1, B2, True)
    assert got["counts"] == (nb_new - 1, 3, 0)
    # threshold chunks and random chunks inside compressed-stored blocks: decoded once, stored raw, nothing encoded
    chunks = threshold_chunks(2)
    body = b"".join(chunks[i % 2] if i % 3 == 0 else text(20 + i, 4096) for i in range(B1 // 4096))
    src = Source(oracle, LZNT1, B1, [body, mixed(12, B1, B2, period=4)])
    assert all(int(src.off[j + 1] - src.off[j]) < B1 for j in range(2))
    got = check(gpu_ctx, oracle, src, LZNT1, B2, False)
    assert got["counts"][1:] == (2 if B2 == 4096 else 1, 0) and 0 < got["counts"][0] < 2 * (B1 // B2)   # (at 32 KiB a lone raw chunk still leaves a block that shrinks)
    check(gpu_ctx, oracle, src, LZNT1, B2, True)
    # a raw-stored source block: encoded where it lies, nothing decoded
    src = Source(oracle, LZNT1, B1, [rand(13, B1)])
    assert int(src.off[1]) == B1
    for with_crc in (False, True):
        got = check(gpu_ctx, oracle, src, LZNT1, B2, with_crc)
        assert got["counts"] == (0, 0, B1 // B2)


@pytest.mark.parametrize("pair", [(LZNT1, 4096, XHUFF, 32768), (XPRESS, 65536, LZNT1, 4096), (XPRESS, 32768, XPRESS, 65536)], ids=lambda p: "%d-%d-to-%d-%d" % p)
def test_cross_format(gpu_ctx, oracle, pair):
    f1, B1, f2, B2 = pair
    G = max(B1, B2)
    src = Source(oracle, f1, B1, [text(16, G + 4096 + 9), mixed(17, G, 4096), rand(18, 5000), b"", text(19, 1)])
    for with_crc in (False, True):
        got = check(gpu_ctx, oracle, src, f2, B2, with_crc)
        nb_new = sum((n + B2 - 1) // B2 for n in src.lens)
        assert got["counts"][0] == 0 and got["counts"][2] == nb_new and 0 < got["counts"][1] <= src.nbt


def test_rules(gpu_ctx, oracle):
    bufs = [text(21, 4 * 4096), rand(22, 2 * 4096), text(23, 8192), mixed(24, 4 * 4096)]
    src = Source(oracle, LZNT1, 4096, bufs)
    # rule 0: a decreasing table
    bad = src.first.copy(); bad[1] = src.first[2] + 1
    got = check(gpu_ctx, oracle, src, LZNT1, 8192, first=bad)
    assert got["status"] == [M.ARG] * 4 and not got["first"].any() and not got["off"].any() and got["counts"] == (0, 0, 0)
    # rule 1: a wrong block count for one resource
    got = check(gpu_ctx, oracle, src, LZNT1, 8192, lens=[src.lens[0] + 4096] + src.lens[1:], nbn=7)
    assert got["status"] == [M.DATA, 0, 0, 0] and list(got["first"]) == [0, 0, 1, 2, 4]
    # rule 2: n_blocks_new one short
    got = check(gpu_ctx, oracle, src, LZNT1, 8192, nbn=5)
    assert got["status"] == [0, 0, 0, M.ARG] and list(got["first"]) == [0, 2, 3, 4, 4]
    # rule 4: groups_max one short -- the last worked resource alone is refused, and has no blocks
    got = check(gpu_ctx, oracle, src, LZNT1, 8192, gmax=2)
    assert got["status"] == [0, 0, 0, M.ARG] and list(got["first"]) == [0, 2, 3, 4, 4] and got["counts"] == (3, 0, 1)
    # rule 6: new_cap one byte short
    full = check(gpu_ctx, oracle, src, LZNT1, 8192, gmax=3)
    assert full["status"] == [0] * 4
    got = check(gpu_ctx, oracle, src, LZNT1, 8192, cap=int(full["off"][6]) - 1)
    assert got["status"] == [0, 0, 0, M.BUF] and (got["off"] == full["off"]).all()


def test_chunk_header_that_does_not_tile(gpu_ctx, oracle):
    src = Source(oracle, LZNT1, 65536, [text(25, 65536), text(26, 65536 + 8192), text(27, 4096 * 3)])
    o = int(src.off[1])                                           # the first chunk header of resource 1's first block: one byte longer
    packed = bytearray(src.packed)
    h = (packed[o] | packed[o + 1] << 8) + 1
    packed[o], packed[o + 1] = h & 255, h >> 8
    got = check(gpu_ctx, oracle, src, LZNT1, 4096, packed=bytes(packed))
    assert got["status"] == [0, M.DATA, 0] and list(got["first"]) == [0, 16, 16, 19]
    packed = bytearray(src.packed)                                # the last image of the block runs past the stored bytes
    packed[o] ^= 0x40
    got = check(gpu_ctx, oracle, src, LZNT1, 4096, packed=bytes(packed), with_crc=False)
    assert got["status"] == [0, M.DATA, 0]


def test_flipped_byte_worked_and_carried(gpu_ctx, oracle):
    """with checksums a damaged member of a worked block fails its resource; the same damage in a carried block is carried along"""
    src = Source(oracle, LZNT1, 4096, [mixed(28, 4 * 4096), text(29, 4 * 4096)])
    for row, want in ((1, [M.DATA, 0]), (5, [0, 0])):
        assert int(src.off[row + 1] - src.off[row]) < 4096
        packed = bytearray(src.packed)
        packed[int(src.off[row + 1]) - 1] ^= 0x01                 # a literal of the block's last token group
        got = check(gpu_ctx, oracle, src, LZNT1, 8192, packed=bytes(packed))
        assert got["status"] == want
    assert got["counts"] == (2, 2, 2)                             # (the damaged block is among the carried ones)


def test_inside_a_capture_and_repeats(oracle):
    """the first execution inside a caller's capture, replayed three times; then plain executions of the same object, with another
    capacity in between (its graph is captured again)"""
    import torch
    import ms_compress_amd as m
    s = torch.cuda.Stream()
    ctx = m.Context(stream=s)
    src = Source(oracle, LZNT1, 4096, [mixed(30, 6 * 4096 + 3), text(31, 4 * 4096), rand(32, 100)])
    with torch.cuda.stream(s):
        run = Run(ctx, src, LZNT1, 8192)
        want = run.model(oracle)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        run.launch()
    for _ in range(3):
        with torch.cuda.stream(s):
            run.poison()
            g.replay()
            got = run.fetch()
            got["counts"] = run.tc.counts()
        same(got, want)
    del g
    for cap in (run.cap, run.cap, run.cap, int(want[2][3]), run.cap):
        run.cap = cap
        same(run.go(), run.model(oracle))
    run.close()
    ctx.close()


def test_empty_resources_and_no_resources(gpu_ctx, oracle):
    src = Source(oracle, LZNT1, 4096, [b"", b"", text(33, 10), b""])
    got = check(gpu_ctx, oracle, src, LZNT1, 65536)
    assert list(got["first"]) == [0, 0, 0, 1, 1] and got["counts"] == (0, 0, 1)
    src = Source(oracle, LZNT1, 4096, [b"", b""])
    got = check(gpu_ctx, oracle, src, XHUFF, 4096)
    assert list(got["first"]) == [0, 0, 0] and got["counts"] == (0, 0, 0)
    src = Source(oracle, XPRESS, 65536, [])
    got = check(gpu_ctx, oracle, src, LZNT1, 4096)
    assert list(got["first"]) == [0] and list(got["off"]) == [0] and got["status"] == []


def test_host_convenience(gpu_ctx, oracle):
    import ms_compress_amd as m
    bufs = [text(34, 3 * 8192), mixed(35, 2 * 8192 + 1), b""]
    src = Source(oracle, LZNT1, 4096, bufs)
    for crc in (None, src.crc):
        new_packed, nfirst, noff, ncrc, status, counts = m.blocks_transcode((LZNT1, src.packed, src.first, src.off, src.lens, crc), 4096, 8192, ctx=gpu_ctx)
        packed, first, off, want_crc = X.fresh(oracle, LZNT1, bufs, 8192, crc is not None)
        assert status == [0, 0, 0] and bytes(new_packed) == packed and (nfirst == first).all() and (noff == off).all()
        assert (ncrc is None) if crc is None else (ncrc == want_crc).all()
        assert counts[0] == 3
