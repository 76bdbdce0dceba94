"""CPU: the resize model (tests/resize_model.py). The GPU tests compare mscomp_amd_writer_resize with this model byte for byte, so the model is
pinned here by the header's consequence: on a healthy container that the container model wrote, with every resource accepted, the resized
container is what the container model and zlib's crc32 give for the data cut or zero-padded by plain slicing. Each rule has a case that
reaches it, and that coverage is asserted. The block-CRC combination of mscomp_amd_res_crc_dev is pinned to zlib.crc32 of whole resources."""
import zlib

import numpy as np
import pytest

import blocks_model as M
import read_model as R
import resize_model as Z
import write_model as W
from resize_model import SPARE, WANTS, mixes

FMTS = {"lznt1": 2, "xpress": 3, "xpress_huff": 4}
MIXED, TEXT, ZEROS5, RANDOM1 = 5, 7, 6, 3                       # rows of R.RECIPES


@pytest.fixture(scope="module")
def api():
    import ms_compress_amd                                       # noqa: F401  the model describes this library's writer: no library, no test
    from ms_compress_amd import api
    assert "mscomp_amd_writer_resize" in api.EXPORTS and "mscomp_amd_res_crc_dev" in api.EXPORTS
    return api


def table(oracle, f, B):
    """W.container with a table of nb + SPARE rows: (bufs, packed, first, off, nbt, crc)"""
    bufs, packed, first, off, _, _ = W.container(oracle, f, B)
    nb = int(first[-1])
    nbt = nb + SPARE
    off = np.concatenate([off[: nb + 1], np.full(SPARE, off[nb], dtype=np.uint64)])
    return bufs, packed, first, off, nbt, R.block_crcs(bufs, B, nbt)


def _run(oracle, f, B, want, blocks_max=1 << 30, new_cap=1 << 40, crc=True, packed=None, first=None, off=None, nbt=None, lens=None):
    bufs, pk, fi, of, nt, bcrc = table(oracle, f, B)
    pk = pk if packed is None else packed
    return Z.model_resize(oracle, f, pk, len(pk), fi if first is None else first, of if off is None else off,
                          [len(b) for b in bufs] if lens is None else lens, B, nt if nbt is None else nbt, want, blocks_max, new_cap, bcrc if crc else None)


@pytest.mark.parametrize("B", (4096, 65536))
@pytest.mark.parametrize("fmt", list(FMTS))
def test_resized_container_is_the_compressed_resized_data(api, oracle, fmt, B):
    f = FMTS[fmt]
    bufs, packed, first, off, nbt, bcrc = table(oracle, f, B)
    lens = [len(b) for b in bufs]
    for v, want in enumerate(mixes(lens, B)):
        for crc in ((True, False) if v == 0 else (True,)):
            got = _run(oracle, f, B, want, crc=crc)
            assert got["res_status"] == [0] * len(bufs) and got["new_len"] == want, v
            new = Z.resized(bufs, want)
            assert [len(b) for b in new] == want
            total = sum(want)
            want_packed, want_first, want_off, st = M.model_compress(oracle, f, new, B, total, total)
            nb = int(want_first[-1])
            assert not st.any() and nb <= nbt
            assert got["packed"] == want_packed and (got["first"] == want_first).all()
            assert (got["off"][: nb + 1] == want_off[: nb + 1]).all() and (got["off"][nb:] == want_off[nb]).all()
            if crc:
                assert (got["crc"] == R.block_crcs(new, B, nbt)).all()
            else:
                assert got["crc"] is None
            cost = [Z.geometry(L, x, (L + B - 1) // B, B) for L, x in zip(lens, want) if L != x]
            assert got["counts"] == (sum(c for _, _, c in cost), sum(1 for _, ch, _ in cost if ch), sum(c for _, _, c in cost))


def test_every_rule_is_reached(api, oracle):
    f, B = 2, 4096
    bufs, packed, first, off, nbt, bcrc = table(oracle, f, B)
    n, lens = len(bufs), [len(b) for b in bufs]
    nb = int(first[-1])
    reached = set()

    def run(want, **kw):
        got = _run(oracle, f, B, want, **kw)
        reached.update(got["reached"])
        return got
    same = list(lens)
    got = run(same)                                               # rule 2 everywhere: the container is copied
    assert got["packed"] == packed and (got["first"] == first).all() and (got["off"] == off).all() and (got["crc"] == bcrc).all()
    assert got["counts"] == (0, 0, 0) and got["reached"] == {2, 7, 9}
    # rule 0, both forms: zeros and MSCOMP_ARG_ERROR only
    beyond = first.copy(); beyond[n] = np.uint64(nbt + 1)
    falling = first.copy(); falling[3] = falling[4] + np.uint64(1)
    for bad in (beyond, falling):
        got = run([L + 1 for L in lens], first=bad)
        assert got["res_status"] == [M.ARG] * n and got["new_len"] == [0] * n and got["packed"] == b"" and got["counts"] == (0, 0, 0)
        assert not got["first"].any() and not got["off"].any() and not got["crc"].any() and got["reached"] == {0}
    # rule 1: a wrong block count is carried as it is -- with its wrong count -- and the others resize around it
    odd = list(lens); odd[MIXED] += B                             # (a length that asks for one block more than the table has)
    want = list(lens); want[MIXED] = 5; want[TEXT] = lens[TEXT] + B
    got = run(want, lens=odd)
    assert got["res_status"] == [M.DATA if r == MIXED else 0 for r in range(n)] and got["new_len"][MIXED] == odd[MIXED]
    assert int(got["first"][MIXED + 1] - got["first"][MIXED]) == 4 and int(got["first"][TEXT + 1] - got["first"][TEXT]) == 5
    assert {1, 5} <= got["reached"]
    # rule 3: costs 1, 2 (a changed block and a fresh one), 3, 1 and a free cut; a budget of 3 is crossed by the third changing resource, and
    # everything that changes behind it is refused too, the free cut included: the sum includes refused ones
    want = list(lens); want[2] = lens[2] - 1; want[4] = 2 * B + 1; want[MIXED] = lens[MIXED] + 3 * B - 17; want[TEXT] = lens[TEXT] - 1; want[9] = 2 * B
    for bmax, st in ((7, {}), (6, {TEXT: M.ARG, 9: M.ARG}), (3, {MIXED: M.ARG, TEXT: M.ARG, 9: M.ARG}), (0, {2: M.ARG, 4: M.ARG, MIXED: M.ARG, TEXT: M.ARG, 9: M.ARG})):
        got = run(want, blocks_max=bmax)
        assert got["res_status"] == [st.get(r, 0) for r in range(n)], bmax
        kept = [lens[r] if r in st else want[r] for r in range(n)]
        assert got["new_len"] == kept
        total = sum(kept)
        assert got["packed"] == M.model_compress(oracle, f, Z.resized(bufs, kept), B, total, total)[0]
    assert 3 in reached
    # rule 4: a flipped byte in the raw block a cut falls into shows with checksums only; the resource is carried verbatim, its neighbours resize
    j = int(first[MIXED])
    assert int(off[j + 1] - off[j]) == B
    hurt = bytearray(packed); hurt[int(off[j]) + 7] ^= 0x55
    want = list(lens); want[MIXED] = 100; want[MIXED + 1] = 0; want[MIXED - 1] = 3 * B
    assert run(want, packed=bytes(hurt), crc=False)["res_status"] == [0] * n
    got = run(want, packed=bytes(hurt))
    assert got["res_status"] == [M.DATA if r == MIXED else 0 for r in range(n)] and got["new_len"][MIXED] == lens[MIXED] and got["counts"] == (3, 2, 2)
    g = int(got["first"][MIXED])
    assert g == j + 1 and int(got["first"][MIXED + 1]) == g + 4 and (got["crc"][g: g + 4] == bcrc[j: j + 4]).all()
    assert got["packed"][int(got["off"][g]): int(got["off"][g + 4])] == bytes(hurt)[int(off[j]): int(off[j + 4])]
    assert {4, 5} <= got["reached"]
    # rule 7: an unreadable clean entry becomes an empty one
    bad = off.copy(); bad[j + 3] = bad[j + 2] - np.uint64(1)
    want = list(lens); want[TEXT] = 9
    got = run(want, off=bad)
    assert got["res_status"] == [0] * n and int(got["off"][j + 3] - got["off"][j + 2]) == 0
    # rule 8 on the final counts: growing by SPARE + 1 rows is refused as a whole; with a cut that frees one row it fits -- unless the cut's
    # changed block is unreadable, so that the cut is carried and counts with its old rows
    want = list(lens); want[ZEROS5] = lens[ZEROS5] + (SPARE + 1) * B
    got = run(want)
    assert got["reached"] >= {8} and got["res_status"] == [M.ARG] * n and not got["off"].any() and got["counts"] == (0, 0, 0)
    want[MIXED] = lens[MIXED] - 18
    assert run(want)["res_status"] == [0] * n
    hurt = bytearray(packed); hurt[int(off[j + 2]) + 7] ^= 0x55    # block 2 of MIXED, raw: the block the cut falls into
    got = run(want, packed=bytes(hurt))
    assert got["reached"] >= {4, 8} and got["res_status"] == [M.ARG] * n
    # rule 10: capacity cuts inside the first dirty block and, with another cap, inside a carried block; MSCOMP_BUF_ERROR replaces the status
    want = list(lens); want[2] = lens[2] - 100
    full = run(want)
    d = int(full["first"][2])
    got = run(want, new_cap=int(full["off"][d + 1]) - 1)
    assert got["res_status"] == [0, 0] + [M.BUF] * 9 + [0] and (got["off"] == full["off"]).all() and got["packed"] == full["packed"][: int(full["off"][d])]
    full = run(want, lens=odd)
    assert full["res_status"][MIXED] == M.DATA
    g = int(full["first"][MIXED])
    got = run(want, lens=odd, new_cap=int(full["off"][g + 2]) - 1)
    assert got["res_status"][MIXED] == M.BUF and got["res_status"][:MIXED] == [0] * MIXED and 10 in got["reached"]
    assert reached == set(range(11)), sorted(set(range(11)) - reached)


@pytest.mark.parametrize("B", (4096, 65536))
def test_block_crc_combination_is_zlib_crc32_of_the_resource(api, B):
    bufs = R.buffers(B)
    lens = [len(b) for b in bufs]
    assert {0, 1, B - 1, B, B + 1, 3 * B + 17, 5 * B} <= set(lens)
    first = np.cumsum([0] + [(L + B - 1) // B for L in lens]).astype(np.uint64)
    nbt = int(first[-1]) + SPARE
    bcrc = R.block_crcs(bufs, B, nbt)
    got, st = Z.model_res_crc(first, lens, bcrc, B, nbt)
    assert st == [0] * len(bufs) and [int(x) for x in got] == [zlib.crc32(b) for b in bufs]
    bad = first.copy(); bad[MIXED + 1] -= np.uint64(1)            # a wrong count here, and in the next resource
    got, st = Z.model_res_crc(bad, lens, bcrc, B, nbt)
    assert st[MIXED] == st[MIXED + 1] == M.DATA and got[MIXED] == 0 and st[MIXED + 2] == 0
    bad = first.copy(); bad[-1] = np.uint64(nbt + 1)
    assert Z.model_res_crc(bad, lens, bcrc, B, nbt)[1][-1] == M.ARG
