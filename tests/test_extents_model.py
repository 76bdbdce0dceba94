"""CPU: the extents model (tests/extents_model.py). The GPU tests compare mscomp_amd_splicer_splice_extents with this model byte for byte,
so the model is pinned here by the header's consequence: on healthy containers that the container model wrote, with every resource
accepted, the new container is what the container model and zlib's crc32 give for the concatenated extent data. Each rule has a case
that reaches it."""
import numpy as np
import pytest

import blocks_model as M
import extents_model as X
import read_model as R
from extents_model import buffers, healthy_lists, in1, source, ONE, BP1, MIXED, ZEROS5, TEXT, MIXED5, X3B, X3B5
from splice_model import expect

FMTS = {"lznt1": 2, "xpress": 3, "xpress_huff": 4}


@pytest.fixture(scope="module")
def api():
    import ms_compress_amd                                       # noqa: F401  the model describes this library's splicer: no library, no test
    from ms_compress_amd import api
    assert "mscomp_amd_splicer_splice_extents" in api.EXPORTS
    return api


@pytest.mark.parametrize("B", (4096, 65536))
@pytest.mark.parametrize("fmt", list(FMTS))
def test_extent_container_is_the_compressed_extent_data(api, oracle, fmt, B):
    f = FMTS[fmt]
    bufs0 = buffers(B)
    bufs1 = bufs0[::-1]
    srcs = [source(oracle, f, B, bufs0), source(oracle, f, B, bufs1)]
    for name, resources in healthy_lists(len(bufs0)).items():
        data = X.extent_data([bufs0, bufs1], resources, B)
        ext_first, ext = X.flat(resources)
        nbt = len(data) + sum(len(b) for b in data) // B       # the rows of the container that compress makes for this data
        for crc in ((True, False) if name == "identity" else (True,)):
            got = X.model_splice_extents(srcs, ext_first, ext, B, len(ext), nbt, 1 << 40, with_crc=crc)
            packed, first, off, bcrc = expect(oracle, f, B, data, nbt)
            assert got["status"] == [0] * len(data) and got["new_len"] == [len(b) for b in data], name
            assert got["packed"] == packed and (got["first"] == first).all() and (got["off"] == off).all(), name
            assert (got["crc"] == bcrc).all() if crc else got["crc"] is None
    ext_first, ext = X.flat(healthy_lists(len(bufs0))["identity"])                     # the identity is the source container
    same = X.model_splice_extents(srcs[:1], ext_first, ext, B, len(ext), srcs[0][7], 1 << 40)
    assert same["packed"] == srcs[0][0] and (same["first"] == srcs[0][2]).all() and (same["off"] == srcs[0][3]).all() and (same["crc"] == srcs[0][5]).all()
    assert len(bufs0[X3B]) == 3 * B and len(bufs0[X3B5]) == 3 * B + 5 and len(bufs0[BP1]) == B + 1


def test_every_rule_is_reached(api, oracle):
    f, B = 3, 4096
    bufs = buffers(B)
    src = source(oracle, f, B, bufs)
    packed, plen, first, off, lens, crc, n, snbt = src
    reached = set()
    healthy = [(0, TEXT, 1, 2)]                                 # beside every refused resource: two blocks that must come through

    def run(resources, sources=None, nbt=64, cap=1 << 40, ext_first=None, n_ext=None):
        ef, ext = X.flat(resources)
        got = X.model_splice_extents(sources or [src], ext_first or ef, ext, B, len(ext) if n_ext is None else n_ext, nbt, cap)
        reached.update(got["reached"])
        return got
    two = M.model_compress(oracle, f, [bufs[TEXT][B: 3 * B]], B, 1 << 20, 1 << 20)[0]
    # rule 0: a falling d_ext_first, and one that ends beyond n_ext -- everything zero
    for kw in ({"ext_first": [0, 2, 1, 3]}, {"n_ext": 2}):
        got = run([[(0, 1, 0, None)], healthy, [(0, 0, 0, None)]], **kw)
        assert got["status"] == [M.ARG] * 3 and got["new_len"] == [0] * 3 and not got["first"].any() and not got["off"].any() and not got["crc"].any()
        assert got["packed"] == b"" and got["reached"] == {0}
    # rules 1-3, each cause, the refused extent between two good ones of its resource; the healthy resource beside it is untouched
    falling = first.copy(); falling[3] = falling[4] + np.uint64(1)
    beyond = first.copy(); beyond[n] = np.uint64(snbt + 1)
    odd = list(lens); odd[MIXED] += B
    nm = 4                                                     # blocks of MIXED (3 B + 17)
    for bad, sources, st, rule in (((1, 0, 0, None), None, M.ARG, 1), ((0, n, 0, None), None, M.ARG, 1), ((0, 1 << 63, 0, 1), None, M.ARG, 1),
                                   ((0, 3, 0, None), [src[:2] + (falling,) + src[3:]], M.ARG, 1), ((0, n - 1, 0, None), [src[:2] + (beyond,) + src[3:]], M.ARG, 1),
                                   ((0, MIXED, 0, 1), [src[:4] + (odd,) + src[5:]], M.DATA, 2),
                                   ((0, MIXED, nm + 1, None), None, M.ARG, 3), ((0, MIXED, nm + 1, 0), None, M.ARG, 3), ((0, MIXED, 1, nm), None, M.ARG, 3),
                                   ((0, MIXED, 0, M.M64 - 1), None, M.ARG, 3)):
        got = run([[(0, X3B, 0, 1), bad, (0, X3B, 1, 1)], healthy], sources)
        assert got["status"] == [st, 0] and got["new_len"] == [0, 2 * B] and list(got["first"]) == [0, 0, 2] and got["packed"] == two, bad
        assert {rule, 5, 7} <= got["reached"]
    # the lowest-indexed refused extent gives the status: a wrong block count in front of a wrong range, and the other way round
    got = run([[(0, MIXED, 0, 1), (0, TEXT, 9, 1)]], [src[:4] + (odd,) + src[5:]])
    assert got["status"] == [M.DATA]
    got = run([[(0, TEXT, 9, 1), (0, MIXED, 0, 1)]], [src[:4] + (odd,) + src[5:]])
    assert got["status"] == [M.ARG]
    # rule 4: a B + 1 resource in front of another extent is refused, as the last extent -- empty ones may follow -- it is accepted
    got = run([[(0, BP1, 0, None), (0, X3B, 0, 1)], healthy, [(0, X3B, 0, 1), (0, BP1, 0, None), (0, X3B, 3, None)], [(0, BP1, 1, 1), (0, ONE, 0, 1)]])
    assert got["status"] == [M.ARG, 0, 0, M.ARG] and got["new_len"] == [0, 2 * B, 2 * B + 1, 0] and 4 in got["reached"]
    got = run([[(0, BP1, 0, None), (0, TEXT, 9, 1)]])           # ends short in front of a refused extent only: that one gives the status
    assert got["status"] == [M.ARG] and 3 in got["reached"] and 4 not in got["reached"]
    # rule 6 crossed in the middle: counts 2, 4, 2, 1, 0 against 5 rows; then a table filled to its last row
    got = run([healthy, [(0, MIXED, 0, None)], healthy, [(0, ONE, 0, None)], [(0, X3B, 0, 0)]], nbt=5)
    assert got["status"] == [0, M.ARG, M.ARG, M.ARG, 0] and list(got["first"]) == [0, 2, 2, 2, 2, 2] and 6 in got["reached"]
    assert len(got["off"]) == 6 and (got["off"][2:] == got["off"][2]).all() and not got["crc"][2:].any() and got["packed"] == two
    got = run([healthy, [(0, X3B, 0, None)]], nbt=5)
    assert got["status"] == [0, 0] and int(got["first"][-1]) == 5
    # rule 8: an unreadable entry is an empty row, its neighbours are carried
    j = int(first[TEXT])
    hurt = off.copy(); hurt[j + 2] = hurt[j + 1] - np.uint64(1)
    got = run([healthy], [src[:3] + (hurt,) + src[4:]])
    assert got["status"] == [0] and got["new_len"] == [2 * B] and int(got["off"][1]) == int(got["off"][0]) and int(got["off"][2]) > int(got["off"][1])
    # rule 9: new_cap one byte short of the last block: MSCOMP_BUF_ERROR, the tables hold the full layout
    full = run([healthy, [(0, X3B5, 2, None)], [(0, ONE, 0, None)]])
    got = run([healthy, [(0, X3B5, 2, None)], [(0, ONE, 0, None)]], cap=int(full["off"][4]) - 1)
    assert got["status"] == [0, M.BUF, M.BUF] and (got["off"] == full["off"]).all() and got["packed"] == full["packed"][: int(full["off"][3])]
    assert reached == set(range(10)), sorted(set(range(10)) - reached)
