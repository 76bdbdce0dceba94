"""Byte alignment in LZNT1's match compares (csrc/lznt1.hip): every compare reads aligned dwords and shifts them with v_alignbyte_b32, which now
gets the byte ADDRESS as its shift (the instruction reads bits [1:0] of it: tests/test_gpu_alignbyte.py), and the eager scan's bucket entries
travel without zero-extension. The units here put a position p and its candidate q at every combination of p mod 4 and q mod 4, with matches
that end at 3, 4, 5, 7, 8, 9, 15, 16, 17, 18, 19 and 20 bytes and at max_len (34 and 18), so that every dword seam of the first stage (bytes
0..7), the second (8..15) and the two tail loops (lz_lcp_wave, lz_lcp_tail) is crossed -- once with the candidate among the four oldest of its
bucket (the eager scan, and the whole-wave extension behind it) and once behind them (the finishing steps). Each chunk ends with a candidate
whose 16 bytes straddle offsets 4095 / 4096 (the reads wrap modulo 4096) and a match that runs to the chunk's end; where q mod 4 is 0 the first
candidate stands at position 0. Six more units end in a short last chunk of 1, 2, 3, 64, 65 and 4095 bytes, whose bucket array keeps leftovers
of the sort behind the entries. Every chunk is placed on the CPU model of the bucket array that tests/lznt1_model.py keeps, the model's
parse must show each match where and as long as the case claims, the oracle's token starts and lengths must equal the model's, and the GPU
tests compare byte for byte with the oracle in both kernel modes through a host-table plan, a device-table plan and the serial-atomics instance."""
import functools

import numpy as np
import pytest

import lznt1_model as M
import lznt1_run as R

LENS = (3, 4, 5, 7, 8, 9, 15, 16, 17, 18, 19, 20, 40)   # 40: beyond max_len 34 of its position
SHORT = (1, 2, 3, 64, 65, 4095)


def _copy(c, q, p, L):
    for i in range(L):                               # (byte by byte: a source that overlaps its target repeats)
        c[p + i] = c[q + i]


def _chunk(pm, qm, seed):
    """(chunk of 4096 bytes, {position: claimed match length}) for positions = pm and candidates = qm modulo 4"""
    ks = M.keys_of_bucket(M.BUCKET, M.NKEYS)
    for s in range(40):
        sd = seed + 104729 * s
        c = M.filler(4096, sd).copy()
        claim = {}
        # the sources from position qm on (position 0 where qm is 0): the eager ones, four old entries of the finishing cases' bucket, those
        at = 0 if qm == 0 else 4 + qm
        src = []
        for path in ("eager", "finish"):
            for i, L in enumerate(LENS + (24,)):                         # (the last one: the match at max_len 18, behind position 2048)
                x = M.filler(L + 1, sd + 31 * i + (7 if path == "eager" else 11)).copy()
                if path == "finish":
                    x[:3] = np.frombuffer(ks[40 + i], np.uint8)          # its own key of the one bucket: agrees with no other on 3 bytes
                at += (qm - at) % 4
                M.place(c, at, x)
                src.append((L, at, x, i == len(LENS)))
                at += L + 3
            if path == "eager":                                          # (behind the eager sources, so that those stay among the four oldest)
                for j in range(4):
                    M.place(c, at, ks[j])
                    at += 5
        assert at < 1000
        lo, hi = 1100, 2100
        for L, q, x, high in src:
            at = hi if high else lo
            at += (pm - at) % 4
            M.place(c, at, x[:L])
            c[at + L] = x[L] ^ 0x55
            claim[at] = min(L, M.max_len(4096, at))
            assert claim[at] == (18 if high else min(L, 34))
            if high:
                hi = at + L + 3
            else:
                lo = at + L + 3
        assert lo < 2040 and hi < 2200
        c[2300:4040] = np.resize(M.filler(24, sd + 5), 1740)            # (so that the chunk is not stored raw)
        q, p = 4080 + qm, 4088 + pm                                      # the candidate's 16 bytes straddle the chunk's end; max_len = n - p
        _copy(c, q, p, 4096 - p)
        claim[p] = 4096 - p
        parse = M.parse(c)
        if all(parse.get(p) == L for p, L in claim.items()):
            fin = [p for p in claim if M.finish(c, p)["finish"]]
            if len(fin) >= len(LENS):                                # (the second half went through finishing steps)
                return c, claim
    raise AssertionError("no chunk for p mod 4 = %d, q mod 4 = %d" % (pm, qm))


@functools.lru_cache(maxsize=None)
def _built():
    """[(name, unit bytes, [claims per chunk or None])]"""
    out = []
    for pm in range(4):
        for qm in range(4):
            c, claim = _chunk(pm, qm, 9000 + 16 * pm + qm)
            out.append(("p mod 4 = %d, q mod 4 = %d" % (pm, qm), c.tobytes(), [claim]))
    first = _chunk(1, 2, 7777)[0]
    for k in SHORT:
        tail = np.resize(M.filler(29, 600 + k), k).astype(np.uint8)     # a period of 29: matches at every alignment
        out.append(("short last chunk of %d bytes" % k, first.tobytes() + tail.tobytes(), [None, None]))
    return out


def _expected(oracle):
    return {name: R.expected(oracle, u) for name, u, _ in _built()}


def test_units_are_what_they_claim():
    built = _built()
    assert len(built) == 16 + len(SHORT)
    for name, u, claims in built[:16]:
        assert len(u) == 4096 and len(claims[0]) == 2 * (len(LENS) + 1) + 1, name
        mods = {(p % 4) for p in claims[0]}
        assert len(mods) == 1, name


def test_the_oracle_parses_the_units_as_the_model_does(oracle):
    for name, u, claims in _built():
        streams = M.chunk_streams(_expected(oracle)[name])
        assert len(streams) == len(claims), name
        for k, (st, claim) in enumerate(zip(streams, claims)):
            chunk = np.frombuffer(u[4096 * k: 4096 * (k + 1)], np.uint8)
            if not st[1] & 0x80:                                         # stored raw: only the shortest chunks may be
                assert len(chunk) <= 3, (name, k)
                continue
            got = M.token_lengths(st)
            assert got == M.parse(chunk), (name, k)
            for p, L in (claim or {}).items():
                assert got.get(p) == L, (name, p, L, got.get(p))
        assert streams[0][1] & 0x80, name


@pytest.mark.gpu
@pytest.mark.parametrize("path", R.PATHS)
@pytest.mark.parametrize("mode", [1, 2])
def test_lznt1_alignments(oracle, gpu_ctx, mode, path):
    built = _built()
    R.check_plan(oracle, gpu_ctx, [u for _, u, _ in built], mode, path, "alignments", names=[name for name, _, _ in built])
