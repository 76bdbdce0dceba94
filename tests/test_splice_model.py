"""CPU: the splice model (tests/splice_model.py). The GPU tests compare mscomp_amd_splicer_splice with this model byte for byte, so the model
is pinned here by the header's consequence: on healthy containers that the container model wrote, with every pick accepted, the spliced
container is what the container model and zlib's crc32 give for the picked data in pick order. Each rule has a case that reaches it."""
import numpy as np
import pytest

import blocks_model as M
import read_model as R
import splice_model as S
import write_model as W
from splice_model import ORDER2, source, pick_lists, expect

FMTS = {"lznt1": 2, "xpress": 3, "xpress_huff": 4}
MIXED, TEXT, ZEROS5, RANDOM1 = 5, 7, 6, 3                       # rows of R.RECIPES


@pytest.fixture(scope="module")
def api():
    import ms_compress_amd                                       # noqa: F401  the model describes this library's splicer: no library, no test
    from ms_compress_amd import api
    assert "mscomp_amd_splicer_splice" in api.EXPORTS
    return api


@pytest.mark.parametrize("B", (4096, 65536))
@pytest.mark.parametrize("fmt", list(FMTS))
def test_spliced_container_is_the_compressed_picked_data(api, oracle, fmt, B):
    f = FMTS[fmt]
    bufs0, src0 = source(oracle, f, B)
    bufs1, src1 = source(oracle, f, B, ORDER2)
    assert [bufs1[ORDER2.index(k)] for k in range(len(bufs0))] == bufs0
    for v, picks in enumerate(pick_lists(len(bufs0))):
        data = S.picked([bufs0, bufs1], picks)
        nbt = sum((len(b) + B - 1) // B for b in data) + 3
        for crc in ((True, False) if v == 0 else (True,)):
            got = S.model_splice([src0, src1], picks, B, nbt, 1 << 40, with_crc=crc)
            packed, first, off, bcrc = expect(oracle, f, B, data, nbt)
            assert got["status"] == [0] * len(picks) and got["new_len"] == [len(b) for b in data], v
            assert got["packed"] == packed and (got["first"] == first).all() and (got["off"] == off).all()
            assert (got["crc"] == bcrc).all() if crc else got["crc"] is None
    same = S.model_splice([src0], pick_lists(len(bufs0))[0], B, src0[7], 1 << 40)       # the identity is the source container
    assert same["packed"] == src0[0] and (same["first"] == src0[2]).all() and (same["off"] == src0[3]).all() and (same["crc"] == src0[5]).all()


def test_every_rule_is_reached(api, oracle):
    f, B = 3, 4096
    bufs, src = source(oracle, f, B)
    packed, plen, first, off, lens, crc, n, snbt = src
    nb = int(first[-1])
    reached = set()

    def run(picks, sources=None, nbt=nb, cap=1 << 40):
        got = S.model_splice(sources or [src], picks, B, nbt, cap)
        reached.update(got["reached"])
        return got
    # rule 1, each cause: no such source, no such resource, a falling table, an entry beyond the source's table; the others are untouched
    falling = first.copy(); falling[3] = falling[4] + np.uint64(1)
    beyond = first.copy(); beyond[n] = np.uint64(snbt + 1)
    for picks, sources, bad in (([(0, 1), (1, 0), (0, 4)], None, 1), ([(0, 1), (0, n), (0, 4)], None, 1), ([(0, 1), (0, 1 << 63), (0, 4)], None, 1),
                                ([(0, 1), (0, 3), (0, 4)], [src[:2] + (falling,) + src[3:]], 1), ([(0, 1), (0, n - 1), (0, 4)], [src[:2] + (beyond,) + src[3:]], 1)):
        got = run(picks, sources)
        assert got["status"] == [M.ARG if p == bad else 0 for p in range(3)] and got["new_len"] == [lens[1], 0, lens[4]]
        assert int(got["first"][2]) == int(got["first"][1]) == 1 and got["packed"] == M.model_compress(oracle, f, [bufs[1], bufs[4]], B, 1 << 20, 1 << 20)[0]
    # rule 2: a length that asks for one block more than the table has
    odd = list(lens); odd[MIXED] += B
    got = run([(0, MIXED), (0, TEXT)], [src[:4] + (odd,) + src[5:]])
    assert got["status"] == [M.DATA, 0] and got["new_len"] == [0, lens[TEXT]] and list(got["first"]) == [0, 0, 4]
    # rule 3 crossed mid-list: counts 4, 5, 4, 1, 0 against a table of 8 rows -- the second pick crosses it, a later pick with one block is
    # refused though it would fit beside the first, a later empty pick is accepted
    got = run([(0, MIXED), (0, ZEROS5), (0, TEXT), (0, 1), (0, 0)], nbt=8)
    assert got["status"] == [0, M.ARG, M.ARG, M.ARG, 0] and got["new_len"] == [lens[MIXED], 0, 0, 0, 0] and list(got["first"]) == [0, 4, 4, 4, 4, 4]
    assert len(got["off"]) == 9 and (got["off"][4:] == got["off"][4]).all() and not got["crc"][4:].any()
    got = run([(0, MIXED), (0, TEXT)], nbt=8)                                          # exactly full
    assert got["status"] == [0, 0] and int(got["first"][-1]) == 8
    # rule 5: an unreadable entry -- decreasing, or beyond packed_len -- is an empty row; its neighbours are carried
    j = int(first[MIXED])
    falling = off.copy(); falling[j + 2] = falling[j + 1] - np.uint64(1)
    past = off.copy(); past[j + 4:] = np.uint64(plen + 1)
    for bad in (falling, past):
        got = run([(0, MIXED)], [src[:3] + (bad,) + src[4:]])
        assert got["status"] == [0] and int(got["first"][1]) == 4 and 5 in got["reached"]
        assert any(int(got["off"][k + 1]) == int(got["off"][k]) for k in range(4))
    # rule 7: new_cap falls inside the second block of the second pick: that pick gets MSCOMP_BUF_ERROR, the tables hold the full layout
    full = run([(0, TEXT), (0, MIXED), (0, 1)])
    g = int(full["first"][1])
    got = run([(0, TEXT), (0, MIXED), (0, 1)], cap=int(full["off"][g + 2]) - 1)
    assert got["status"] == [0, M.BUF, M.BUF] and (got["off"] == full["off"]).all() and got["packed"] == full["packed"][: int(full["off"][g + 1])]
    got = run([(0, TEXT), (0, 0)], cap=0)
    assert got["status"] == [M.BUF, 0] and got["packed"] == b""
    assert reached == set(range(1, 8)), sorted(set(range(1, 8)) - reached)
