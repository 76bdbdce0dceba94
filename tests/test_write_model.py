"""CPU: the block-writer model (tests/write_model.py). The GPU tests compare mscomp_amd_writer_* with this model byte for byte, so the model is
pinned here by the header's rule 10: on a healthy container that the container model wrote, the written container is what the container
model and zlib's crc32 give for the data patched by plain slicing. Each reject rule is asserted once."""
import numpy as np
import pytest

import blocks_model as M
import read_model as R
import write_model as W

FMTS = {"lznt1": 2, "xpress": 3, "xpress_huff": 4}
MIXED, TEXT, RANDOM1 = 5, 7, 3                                  # rows of R.RECIPES: 3 B + 17 mixed / text, one raw block


@pytest.fixture(scope="module")
def api():
    import ms_compress_amd                                       # noqa: F401  the model describes this library's writer: no library, no test
    from ms_compress_amd import api
    assert "mscomp_amd_writer_write" in api.EXPORTS
    return api


def _writes(bufs, B, seed, count):
    rs = np.random.RandomState(seed)
    reqs, srcs = [], []
    for _ in range(count):
        r = int(rs.randint(0, len(bufs)))
        L = len(bufs[r])
        o = int(rs.randint(0, L + 3))
        pick = [0, 1, 7, 64, B - 1, B, B + 1, 2 * B + 5, int(rs.randint(0, 3 * B)), M.M64]
        ln = pick[int(rs.randint(0, len(pick)))]
        want = W.clip((r, o, ln), [len(b) for b in bufs])[1]
        kind = int(rs.randint(0, 3))
        srcs.append(bytes(want) if kind == 0 else rs.bytes(want) if kind == 1 else (b"pwrite " * (want // 7 + 1))[:want])
        reqs.append((r, o, ln))
    return reqs, srcs


def _run(oracle, f, B, reqs, srcs, blocks_max=1 << 30, new_cap=None, crc=True, packed=None, first=None, off=None, packed_len=None, old_crc=None):
    bufs, pk, fi, of, nbt, bcrc = W.container(oracle, f, B)
    pk = pk if packed is None else packed
    total = sum(len(b) for b in bufs)
    return W.model_write(oracle, f, pk, len(pk) if packed_len is None else packed_len, fi if first is None else first, of if off is None else off,
                         [len(b) for b in bufs], B, nbt, reqs, srcs, blocks_max, total if new_cap is None else new_cap,
                         (bcrc if old_crc is None else old_crc) if crc else None)


@pytest.mark.parametrize("B", (4096, 65536))
@pytest.mark.parametrize("fmt", list(FMTS))
def test_written_container_is_the_compressed_patched_data(api, oracle, fmt, B):
    f = FMTS[fmt]
    bufs, packed, first, off, nbt, bcrc = W.container(oracle, f, B)
    total = sum(len(b) for b in bufs)
    reqs, srcs = _writes(bufs, B, 11, 40)
    reqs += [(RANDOM1, 0, B), (TEXT, B, B), (TEXT, 5, 9), (TEXT, 7, 3)]          # zeros over a raw block, random over a text block, an overlap
    srcs += [bytes(B), np.random.RandomState(1).bytes(B), b"AAAAAAAAA", b"bbb"]
    for crc in (True, False):
        got = _run(oracle, f, B, reqs, srcs, crc=crc)
        assert got["status"] == [0] * len(reqs) and got["res_status"] == [0] * len(bufs)
        assert got["written"] == [W.clip(q, [len(b) for b in bufs])[1] for q in reqs]
        new = W.patched(bufs, reqs, srcs)
        assert new[TEXT][5:14] == b"AAbbbAAAA"                                   # the later request wins
        want_packed, want_first, want_off, st = M.model_compress(oracle, f, new, B, total, total)
        assert not st.any() and (want_first == first).all()
        assert got["packed"] == want_packed and (got["off"] == want_off).all()
        if crc:
            assert (got["crc"] == R.block_crcs(new, B, nbt)).all()
        else:
            assert got["crc"] is None
        j = int(first[RANDOM1])
        assert int(off[j + 1] - off[j]) == B and int(got["off"][j + 1] - got["off"][j]) < B       # raw -> compressed: every later offset moves
        units, distinct, dirty = got["counts"]
        assert dirty == distinct <= int(first[-1]) and distinct < units


def test_no_requests_copies_the_container(api, oracle):
    bufs, packed, first, off, nbt, bcrc = W.container(oracle, 3, 4096)
    got = _run(oracle, 3, 4096, [], [])
    assert got["packed"] == packed and (got["off"] == off).all() and (got["crc"] == bcrc).all() and got["counts"] == (0, 0, 0)


def test_reject_rules(api, oracle):
    f, B = 2, 4096
    bufs, packed, first, off, nbt, bcrc = W.container(oracle, f, B)
    n, lens = len(bufs), [len(b) for b in bufs]
    j = int(first[MIXED])                                         # block 0 raw, block 1 compressed
    reqs = [(MIXED, 10, 100), (n, 0, 5), (MIXED, B - 1, 2), (TEXT, 0, 3 * B), (M.M64, 0, 1), (RANDOM1, 4, 4), (0, 0, 9)]
    srcs = [bytes([q + 1]) * W.clip(q_, lens)[1] for q, q_ in enumerate(reqs)]
    ok = _run(oracle, f, B, reqs, srcs)
    assert ok["status"] == [0, M.ARG, 0, 0, M.ARG, 0, 0] and ok["written"] == [100, 0, 2, 3 * B, 0, 4, 0]      # rule 1
    # rule 0: the table as a whole
    bad = first.copy(); bad[n] = np.uint64(nbt + 1)
    got = _run(oracle, f, B, reqs, srcs, first=bad)
    assert got["status"] == [M.ARG] * len(reqs) and got["res_status"] == [M.ARG] * n and got["written"] == [0] * len(reqs)
    assert not got["off"].any() and not got["crc"].any() and got["packed"] == b"" and got["counts"] == (0, 0, 0)
    bad = first.copy(); bad[3] = bad[4] + np.uint64(1)
    assert _run(oracle, f, B, reqs, srcs, first=bad)["status"] == [M.ARG] * len(reqs)
    # rule 2: a wrong block count fails the resource's requests and leaves its blocks clean
    bad = first.copy(); bad[MIXED + 1] -= np.uint64(1)
    got = _run(oracle, f, B, reqs, srcs, first=bad)
    assert got["status"] == [M.DATA, M.ARG, M.DATA, 0, M.ARG, 0, 0]
    assert got["packed"][int(off[j]): int(off[j + 2])] == packed[int(off[j]): int(off[j + 2])] and (got["off"][: j + 3] == off[: j + 3]).all()
    # rule 4: the budget -- covering blocks 1, -, 2, 3, -, 1, 0
    for bmax, want in ((7, [0, M.ARG, 0, 0, M.ARG, 0, 0]), (6, [0, M.ARG, 0, 0, M.ARG, M.ARG, 0]), (3, [0, M.ARG, 0, M.ARG, M.ARG, M.ARG, 0]),
                       (0, [M.ARG] * 6 + [0])):
        got = _run(oracle, f, B, reqs, srcs, blocks_max=bmax)
        assert got["status"] == want, bmax
        new = W.patched(bufs, reqs, srcs, [s == 0 for s in want])
        total = sum(lens)
        assert got["packed"] == M.model_compress(oracle, f, new, B, total, total)[0]
    # rule 5: a damaged block fails exactly the requests that cover it; it is carried verbatim, and a failed request dirties nothing
    hurt = bytearray(packed); hurt[int(off[j]) + 7] ^= 0x55       # a byte of the raw block: seen with checksums only
    assert _run(oracle, f, B, reqs, srcs, packed=bytes(hurt), crc=False)["status"] == ok["status"]
    got = _run(oracle, f, B, reqs, srcs, packed=bytes(hurt))
    assert got["status"] == [M.DATA, M.ARG, M.DATA, 0, M.ARG, 0, 0]
    assert got["packed"][int(off[j]): int(off[j + 2])] == bytes(hurt)[int(off[j]): int(off[j + 2])] and (got["off"][: j + 3] == off[: j + 3]).all() and (got["crc"][j: j + 2] == bcrc[j: j + 2]).all()
    assert got["counts"] == (7, 6, 4)
    # rule 8: a clean block whose entries cannot be read gets the stored length 0
    bad = off.copy(); bad[j + 3] = bad[j + 2] - np.uint64(1)      # block 2 of MIXED ends before it starts (block 3 then starts early: readable)
    got = _run(oracle, f, B, [(TEXT, 0, 4)], [b"abcd"], off=bad)
    assert got["status"] == [0] and int(got["off"][j + 3] - got["off"][j + 2]) == 0
    # rule 9: one byte short
    need = int(ok["off"][-1])
    got = _run(oracle, f, B, reqs, srcs, new_cap=need - 1)
    last = max(r for r in range(n) if lens[r])
    assert got["res_status"] == [M.BUF if r == last else 0 for r in range(n)] and (got["off"] == ok["off"]).all()
    assert got["packed"] == ok["packed"][: int(ok["off"][int(first[-1]) - 1])]
