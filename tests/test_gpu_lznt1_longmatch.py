"""-m gpu: LZNT1 long matches (a candidate that matches 16 bytes or more, extended by the whole wave when the greedy walk lands on
its position) against the oracle, in both chunk-kernel modes: repeats that start in every max_len regime (max_len = 2^(12 - k) + 2
by position, and n - p near the end of a chunk) and end just before, at and after max_len, equal-length candidates (the oldest
wins), long-pending positions that also have a fifth candidate, all-zero and periodic chunks, long matches across the segment seams
of the four-wave kernel, ragged last chunks, and pieces of the long-repeat corpus members."""
import numpy as np
import pytest

import lznt1_run as R
from lznt1_model import max_len

pytestmark = pytest.mark.gpu


def _repeat(rng, p0, dist, length, n=4096):
    """a random chunk whose bytes p0 .. p0 + length - 1 repeat those `dist` earlier (an overlapping copy when dist < length)"""
    d = rng.integers(0, 256, n, dtype=np.uint8)
    for i in range(p0, min(n, p0 + length)):
        d[i] = d[i - dist]
    if p0 + length < n:
        d[p0 + length] = d[p0 + length - dist] ^ 0x5A       # the match ends exactly here
    return d


def _units():
    rng = np.random.default_rng(8)
    units = []
    # one start in every max_len regime; lengths around 16 bytes, the 256-byte steps and max_len
    for p0 in (1, 5, 16, 17, 20, 32, 40, 64, 100, 128, 200, 256, 300, 512, 700, 1024, 1500, 2048, 3000, 4000):
        ml = max_len(4096, p0)
        for length in sorted({15, 16, 17, 18, 255, 256, 257, 271, 272, 273, ml - 1, ml, ml + 1, 4096 - p0}):
            if length < 1 or p0 + length > 4096:
                continue
            for dist in (1, 3, 16, 17, 300):
                if dist <= p0:
                    units.append(_repeat(rng, p0, dist, length))
    # equal-length candidates: the same 80 bytes at 100, 300, 500 and 700 (each followed by other bytes) -- the oldest wins
    x = rng.integers(0, 256, 1200, dtype=np.uint8)
    d = rng.integers(0, 256, 4096, dtype=np.uint8)
    for q in (100, 300, 500, 700, 2500):
        d[q:q + 80] = x[:80]
    units.append(d)
    # long-pending and unresolved: four older copies that stop early, a fifth and a sixth (found by the finishing step) that go further
    for lens in ((50, 60, 70, 80, 150, 200), (20, 20, 20, 20, 20, 40), (30, 30, 30, 30, 900, 900), (17, 18, 19, 20, 600, 1000)):
        d = rng.integers(0, 256, 4096, dtype=np.uint8)
        q = 40
        for ln in lens:
            d[q:q + ln] = x[:ln]
            q += ln + 37
        d[3000:3000 + max(lens)] = x[:max(lens)]
        units.append(d)
    # all-zero and periodic chunks (every lane long-pending), whole and ragged
    for period in (1, 2, 3, 4, 5, 7, 8, 16, 17, 31, 64, 255, 256, 257, 1000):
        base = rng.integers(1, 256, period, dtype=np.uint8)
        for n in (4096, 3 * 4096 + 18, 2 * 4096 + 1, 4096 + 300):
            units.append(np.tile(base, n // period + 1)[:n].copy())
    units.append(np.zeros(5 * 4096 + 7, np.uint8))
    # random text with long repeats across the four-wave kernel's seams (windows 21 / 38 / 52 = bytes 1344 / 2432 / 3328)
    for p0 in (1300, 1330, 1343, 1344, 2400, 2431, 3300, 3327, 3328):
        for dist, length in ((700, 200), (64, 2000), (5, 400), (1000, 34)):
            if dist <= p0:
                units.append(_repeat(rng, p0, dist, length))
    # ragged last chunks that end inside a long repeat (the match ends at n - p)
    for r in (1, 3, 4, 17, 18, 19, 100, 1000, 4095):
        d = rng.integers(0, 256, 4096 + r, dtype=np.uint8)
        d[4096 + r // 2:] = d[4096 + r // 2 - 40:4096 + r - 40]      # a copy 40 bytes back up to the end
        units.append(d)
        units.append(np.concatenate([rng.integers(0, 256, 4096, dtype=np.uint8), np.full(r, 7, np.uint8)]))
    return units


def _corpus_pieces():
    from ms_compress_amd import corpus
    return [corpus.by_name(name, 96 * 4096 + 123) for name in ("nci", "osdb", "sao", "x-ray", "mozilla")]


@pytest.mark.parametrize("mode", [1, 2])
def test_lznt1_long_matches(oracle, gpu_ctx, mode):
    R.check_batch(oracle, gpu_ctx, _units() + _corpus_pieces(), mode, 0, "long matches")
