"""CPU: the model of the block digests (tests/digest_model.py) held to the known answers of include/mscomp_amd.h's tree parameters, and
model_sync_digest held to sync_model.model_sync: on a healthy store both answer alike but for count[7], over every case
tests/test_gpu_digest.py runs on the device."""
import numpy as np
import pytest

import digest_model as G
import sync_model as Y
from test_sync_model import FMTS, oracle_store


def pat(n):
    return bytes((i * 7 + 3) & 255 for i in range(n))


KNOWN = (
    (b"abc", "ceb2aabffbd66b44624407bed68134d4"),
    (bytes(64), "cf3711f8377d87482f1dd2d4a916d866"),
    (pat(1024), "b063e986ff3e45626db77cd913998cc3"),
    (pat(1025), "304edd0b6f826958b2549029af88dc8c"),
    (pat(4096), "71548664a6a59ffd4eaef72369e28caf"),
    (pat(65536), "73daf8242c5136c47b7e4bb9dc620c3a"),
    (pat(524288), "97ebdfed9bf0364de0e4a61d24ede476"),
)


def test_known_answers():
    for data, want in KNOWN:
        assert G.block_digest(data).hex() == want, len(data)
        assert G.words(G.block_digest(data)).tobytes().hex() == want          # four little-endian words: the same 16 bytes


def test_model_digests_numbering_and_refusal():
    B = 4096
    bufs = [pat(B + 1), b"", pat(3), pat(2 * B)]
    dig, st = G.model_digests(bufs, B, 3 * B + 4)
    assert dig.shape == (4 + 3, 4) and list(st) == [0, 0, 0, 0]
    want = [G.block_digest(x) for x in (bufs[0][:B], bufs[0][B:], bufs[2], bufs[3][:B], bufs[3][B:])]
    assert [dig[j].tobytes() for j in range(5)] == want and not dig[5:].any()
    dig, st = G.model_digests(bufs, B, 3 * B + 3)                                  # the last resource goes over: no blocks
    assert list(st) == [0, 0, 0, G.ARG] and [dig[j].tobytes() for j in range(3)] == want[:3] and not dig[3:].any()


def test_model_check():
    B = 4096
    bufs = [pat(B + 17), pat(5)]
    dig, _ = G.model_digests(bufs, B, B + 22)
    out = bytearray(b"\xA5" * 3 + bufs[0] + b"\xA5" * 2 + bufs[1])
    args = ([3, 3 + B + 17 + 2], [len(b) for b in bufs], [0, 2, 3])
    assert G.model_check(out, *args, dig, [0, 0], [B + 17, 5], B, B + 22) == ([0, 0], [B + 17, 5])
    out[3 + B + 1] ^= 1
    assert G.model_check(out, *args, dig, [0, 0], [B + 17, 5], B, B + 22) == ([G.DATA, 0], [0, 5])
    assert G.model_check(out, *args, dig, [0, 0], [B, 5], B, B + 22, ranges=[(0, 1), (0, 9)]) == ([0, 0], [B, 5])   # the flipped block is out of range
    assert G.model_check(out, *args, dig, [G.DATA, 0], [7, 5], B, B + 22) == ([G.DATA, 0], [7, 5])                  # not OK on entry: left alone


@pytest.mark.parametrize("B", [4096])
def test_sync_by_digest_is_sync_on_a_healthy_store(oracle, B):
    f = FMTS["xpress"]
    bufs = Y.store_buffers(B)
    store = oracle_store(oracle, f, bufs, B)
    dig = G.store_digests(bufs, B, store[7])
    for name, units in Y.cases(B).items():
        total = sum(len(u) for u in units)
        offs = np.cumsum([0] + [len(u) + 3 for u in units[:-1]]) + 1
        a = Y.model_sync(oracle, f, store, units, offs, B, total, 1 << 20)
        b = G.model_sync_digest(store, dig, units, offs, B, total, 1 << 20)
        assert b["count"][7] == b["count"][2] == len(b["kept"])
        assert {k: v for k, v in a.items() if k != "count"} == {k: v for k, v in b.items() if k != "count"}, name
        assert a["count"][:7] == b["count"][:7], name
        if name == "forged":                                                       # same CRC-32, other bytes: kept, and refuted by the digest
            assert b["count"][2] == 2 and b["count"][3] == 1 and b["hits"][0] == [(33 + B + 5, 2, 0)]
    # never reads the store's bytes
    blind = (None,) + store[1:]
    units = Y.cases(B)["edits"]
    assert G.model_sync_digest(blind, dig, units, [0] * 3, B, 1 << 30, 1 << 20) == G.model_sync_digest(store, dig, units, [0] * 3, B, 1 << 30, 1 << 20)
    # a stale digest word: that row's candidates are refuted and its bytes come out as literals
    stale = dig.copy()
    stale[0, 2] ^= 1
    mo = G.model_sync_digest(store, stale, [bufs[0]], [0], B, 1 << 30, 1 << 20)
    assert mo["hits"] == [[(B, 0, 1), (2 * B, 0, 2)]] and mo["literals"] == [[(0, B), (3 * B, 17)]] and mo["count"][2] - mo["count"][3] == 1
