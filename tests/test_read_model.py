"""CPU: the block-reader model (tests/read_model.py). The GPU tests compare mscomp_amd_reader_* with this model byte for byte, so the model is
pinned here: every MSCOMP_OK answer is the slice of the source buffer, the budget rejects exactly from the first request whose running total
passes blocks_max, and damage reaches exactly the requests that cover the damaged block."""
import numpy as np
import pytest

import blocks_model as M
import read_model as R

FMTS = {"lznt1": 2, "xpress": 3, "xpress_huff": 4}


@pytest.fixture(scope="module")
def api():
    import ms_compress_amd                                       # noqa: F401  the model describes this library's reader: no library, no test
    from ms_compress_amd import api
    assert "mscomp_amd_reader_read" in api.EXPORTS
    return api


def _container(oracle, fmt, B):
    bufs = R.buffers(B)
    total = sum(len(b) for b in bufs)
    packed, first, off, st = M.model_compress(oracle, fmt, bufs, B, total, total)
    assert not st.any()
    return bufs, packed, first, off, len(bufs) + total // B


def _requests(bufs, B, seed, count):
    rs = np.random.RandomState(seed)
    reqs = []
    for _ in range(count):
        r = int(rs.randint(0, len(bufs)))
        L = len(bufs[r])
        o = int(rs.randint(0, L + 3))
        pick = [0, 1, 7, B - 1, B, B + 1, 2 * B + 5, 3 * B, int(rs.randint(0, 6 * B)), M.M64]
        ln = pick[int(rs.randint(0, len(pick)))]
        reqs.append((r, o, ln))
    return reqs


@pytest.mark.parametrize("fmt", list(FMTS))
def test_ok_answers_are_slices_of_the_source(api, oracle, fmt):
    f, B = FMTS[fmt], 4096
    bufs, packed, first, off, nbt = _container(oracle, f, B)
    lens = [len(b) for b in bufs]
    reqs = _requests(bufs, B, 5, 300) + [(len(bufs), 0, 1), (M.M64, 0, 1), (6, 5 * B, 9), (6, 5 * B + 100, 9), (0, 0, M.M64)]
    crc = R.block_crcs(bufs, B, nbt)
    for with_crc in (None, crc):
        outs, st, (units, distinct, decoded) = R.model_read(oracle, f, packed, len(packed), first, off, lens, B, nbt, reqs, [1 << 62] * len(reqs), 1 << 30, with_crc)
        for (r, o, ln), out, s in zip(reqs, outs, st):
            if r >= len(bufs):
                assert s == M.ARG and out is None
            else:
                assert s == M.OK and out == bufs[r][o: o + min(ln, len(bufs[r]))], (r, o, ln)
        assert 0 < decoded < distinct <= int(first[-1]) < units      # raw and compressed blocks were read, and blocks were shared


def test_budget_rejects_from_the_first_request_past_blocks_max(api, oracle):
    f, B = 3, 4096
    bufs, packed, first, off, nbt = _container(oracle, f, B)
    lens = [len(b) for b in bufs]
    # covering blocks per request: 1, 2, 0 (empty), 3, ARG (no such resource: not counted), BUF (not counted), 1, 1 (want 0 behind it: OK at any budget)
    reqs = [(5, 10, 100), (5, B - 1, 2), (0, 0, 50), (9, B, 3 * B), (99, 0, 5), (6, 0, 5 * B), (5, 0, 1), (7, 5, 5), (5, lens[5], 100)]
    caps = [1 << 40] * len(reqs); caps[5] = 5 * B - 1
    want = {0: [M.ARG, M.ARG, 0, M.ARG, M.ARG, M.BUF, M.ARG, M.ARG, 0], 1: [0, M.ARG, 0, M.ARG, M.ARG, M.BUF, M.ARG, M.ARG, 0],
            3: [0, 0, 0, M.ARG, M.ARG, M.BUF, M.ARG, M.ARG, 0], 6: [0, 0, 0, 0, M.ARG, M.BUF, M.ARG, M.ARG, 0],
            7: [0, 0, 0, 0, M.ARG, M.BUF, 0, M.ARG, 0], 8: [0, 0, 0, 0, M.ARG, M.BUF, 0, 0, 0]}
    for bmax, exp in want.items():
        outs, st, counts = R.model_read(oracle, f, packed, len(packed), first, off, lens, B, nbt, reqs, caps, bmax)
        assert st == exp, (bmax, st)
        assert counts[0] == sum(c for c, s in zip([1, 2, 0, 3, 0, 0, 1, 1, 0], st) if s == 0)
        for (r, o, ln), out, s in zip(reqs, outs, st):
            assert (out is None) if s else out == bufs[r][o: o + ln]


def test_damage_reaches_exactly_the_covering_requests(api, oracle):
    f, B = 2, 4096
    bufs, packed, first, off, nbt = _container(oracle, f, B)
    lens = [len(b) for b in bufs]
    target = 5                                                    # "mixed", 3 B + 17: block 0 random (raw), block 1 text (compressed)
    j = int(first[target])
    assert int(off[j + 1] - off[j]) == B and int(off[j + 2] - off[j + 1]) < B
    reqs = [(target, 0, 10), (target, B - 1, 2), (target, B, B), (target, 2 * B, 5), (7, 0, 3 * B), (target, 0, M.M64)]
    caps = [1 << 40] * len(reqs)
    covers = [{0}, {0, 1}, {1}, {2}, set(), {0, 1, 2, 3}]
    for k in (0, 1):                                              # a table entry: s = 0 for block k of the target
        bad = off.copy(); bad[j + k + 1] = bad[j + k]
        st = R.model_read(oracle, f, packed, len(packed), first, bad, lens, B, nbt, reqs, caps, 100)[1]
        assert st == [M.DATA if (k in c or k + 1 in c) else 0 for c in covers]      # (block k + 1 grew beyond its data length with it)
    crc = R.block_crcs(bufs, B, nbt)
    hurt = bytearray(packed); hurt[int(off[j]) + 7] ^= 0x55       # a byte of the raw block
    assert R.model_read(oracle, f, bytes(hurt), len(hurt), first, off, lens, B, nbt, reqs, caps, 100)[1] == [0] * len(reqs)
    st = R.model_read(oracle, f, bytes(hurt), len(hurt), first, off, lens, B, nbt, reqs, caps, 100, crc)[1]
    assert st == [M.DATA if 0 in c else 0 for c in covers]
    bad = first.copy(); bad[target + 1] += np.uint64(1)          # a wrong block count: the resource and its neighbour
    st = R.model_read(oracle, f, packed, len(packed), bad, off, lens, B, nbt, reqs + [(target + 1, 0, 1)], caps + [9], 100)[1]
    assert st == [M.DATA] * 4 + [0, M.DATA, M.DATA]
