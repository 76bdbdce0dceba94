"""CPU: the model of the block sync (tests/sync_model.py) held to zlib and to brute force -- the rolling identity at every offset, the
forged collision, thinning against a greedy walk over all raw candidates, the cap -- and the header's consequence in the model for every
case tests/test_gpu_sync.py runs on the device, over stores the oracle's encoders make."""
import zlib

import numpy as np
import pytest

import blocks_model as M
import read_model as R
import sync_model as Y

SHAPES = (("lznt1", 4096), ("xpress", 4096), ("xpress_huff", 4096), ("xpress", 65536))
FMTS = {"lznt1": 2, "xpress": 3, "xpress_huff": 4}


def oracle_store(oracle, fmt, bufs, B):
    """the container the oracle's encoder makes of ``bufs``, as a model source with its checksums"""
    total = sum(len(b) for b in bufs)
    packed, first, off, st = M.model_compress(oracle, fmt, bufs, B, total, total)
    assert not st.any()
    nbt = len(off) - 1
    return (packed, len(packed), first, off, [len(b) for b in bufs], R.block_crcs(bufs, B, nbt), len(bufs), nbt)


def test_rolling_identity_is_zlib_at_every_offset():
    B = 4096
    buf = Y.rnd(1, 3 * B + 17)
    w = Y.window_crcs(buf, B)
    assert len(w) == 2 * B + 18
    assert all(int(w[p]) == zlib.crc32(buf[p: p + B]) for p in range(len(w)))
    R_ = Y.prefixes(buf)
    assert len(R_) == len(buf) + 1 and int(R_[0]) == 0 and int(R_[-1]) == zlib.crc32(buf) ^ zlib.crc32(bytes(len(buf)))
    B = 65536
    buf = Y.rnd(2, 3 * B + 17)
    w = Y.window_crcs(buf, B)
    for p in [0, len(w) - 1] + [int(x) for x in np.random.RandomState(3).randint(0, len(w), 198)]:
        assert int(w[p]) == zlib.crc32(buf[p: p + B]), p
    assert len(Y.window_crcs(buf[: B - 1], B)) == 0 and len(Y.window_crcs(buf[:B], B)) == 1


def test_forge_collides_and_differs():
    for seed, n in ((4, 4096), (5, 65536), (6, 5)):
        blk = Y.rnd(seed, n)
        f = Y.forge(blk)
        assert len(f) == n and f != blk and f[0] != blk[0] and f[1:-4] == blk[1:-4]
        assert zlib.crc32(f) == zlib.crc32(blk)


def test_thinning_is_the_greedy_walk():
    B = 4096
    zeros = [(p, 7) for p in range(4 * B + 1)]                    # 5 B zeros against a zero block: every position a candidate
    assert Y.thin(zeros, B) == Y.greedy(zeros, B) == [(i * B, 7) for i in range(5)]
    two = [(p, 1 + (p // 3) % 2) for p in range(100)]             # two rows by turns, three positions each: every run starts again
    assert Y.thin(two, B) == [(p, 1 + (p // 3) % 2) for p in range(0, 100, 3)]
    apart = [(p, 3) for p in range(10, 20)] + [(p, 3) for p in range(21, 30)] + [(p, 4) for p in range(30, 2 * B + 40)]
    assert Y.thin(apart, B) == [(10, 3), (21, 3), (30, 4), (30 + B, 4), (30 + 2 * B, 4)]


@pytest.mark.parametrize("fmt,B", SHAPES)
def test_consequence_holds_in_the_model(oracle, fmt, B):
    f = FMTS[fmt]
    store = oracle_store(oracle, f, Y.store_buffers(B), B)
    for name, units in Y.cases(B).items():
        total = sum(len(u) for u in units)
        offs = np.cumsum([0] + [len(u) + 3 for u in units[:-1]]) + 1
        mo = Y.model_sync(oracle, f, store, units, offs, B, total, 1 << 20)
        assert mo["res_status"] == [0, 0, 0] and mo["status"] == [0] * len(units)
        Y.holds_consequence(oracle, f, store, units, mo, B)
        assert mo["count"][1] == mo["count"][2] and mo["count"][4] == len(mo["req"]) and mo["count"][6] == total - B * mo["count"][4], name
        if name == "zeros":
            assert [p for p, _, _ in mo["hits"][0]] == [i * B for i in range(5)] and {(r, k) for _, r, k in mo["hits"][0]} == {(1, 0)}
            assert Y.model_sync(oracle, f, store, units[:1], offs, B, total, 1 << 20)["count"][:2] == [4 * B + 1, 5]
        if name == "forged":
            assert mo["count"][2] == 2 and mo["count"][3] == 1 and mo["hits"][0] == [(33 + B + 5, 2, 0)]
        if name == "edits":
            assert mo["count"][4] >= 6
            k = mo["count"][1] - 1                                 # the cap keeps a prefix, and the recipe stays valid
            capped = Y.model_sync(oracle, f, store, units, offs, B, total, k)
            assert capped["kept"] == mo["kept"][:k] and capped["count"][1] == mo["count"][1] and capped["count"][2] == k
            Y.holds_consequence(oracle, f, store, units, capped, B)
        if name == "short":
            assert mo["hits"] == [[(0, 0, 2)], []] and mo["literals"] == [[(B, 17)], [(0, B + 17)]]
