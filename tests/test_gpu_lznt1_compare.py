"""-m gpu: the candidate compares of LZNT1's window parse (csrc/lznt1.hip lz_window) against the oracle, in both chunk-kernel modes.
The parse decides which bucket entries are candidates without a count (an active position is itself an entry of its bucket, the entries in
front of it are its candidates) and compares the first 8 bytes of a candidate first, bytes 8..15 and beyond only when a candidate of the wave
agreed on all 8. The units here put one position of a chunk on each edge of those rules, and matches of the longest length and offset on the
positions where the token split changes; every unit is one or two chunks. The builders check on a model of the bucket array that a unit is
what it says.
What the validity units can show: that the cut at the own entry is not one entry early or late (a lost candidate, or the position matching
itself) and that the finishing loop ends in the step that holds the own entry. An entry wrongly admitted BEHIND the own entry -- the next
buckets', a short chunk's leftover slots, the table behind the array -- belongs to another bucket, agrees on fewer than 3 bytes and is no
match whatever the mask says: those reads are covered for termination and the cut, not for more."""
import functools

import numpy as np
import pytest

import lznt1_model as M
import lznt1_run as R
from lznt1_model import BITS, bucket_model as _model, filler as _filler, keys_of_bucket as _keys, place as _place

pytestmark = pytest.mark.gpu


def _lcp(c, q, p):
    return M.lcp(c, q, p, len(c) - p)


def _repeats(c, lo, p, seed):
    """make the chunk compressible (a chunk that does not shrink is stored raw and shows no decision of the parse): a 24-byte block repeated from lo
    up to the window of position p, which itself holds filler alone"""
    hi = p & ~63
    if hi - lo >= 48:
        c[lo:hi] = np.resize(_filler(24, seed + 5), hi - lo)


def _colliders(c, keys, first, stride):
    """distinct keys of one bucket at first, first + stride, ...: older same-bucket positions that match nothing"""
    for i, k in enumerate(keys):
        _place(c, first + i * stride, k)


# ---- validity without the count -------------------------------------------------------------------------------------

def _validity_unit(n, bucket, r, seed, tail=3):
    """position p = n - tail, a token start, with exactly r older positions in its bucket, all of other keys. With tail = 3 it is the chunk's last
    key position: every entry behind its own in the array is smaller than p (or lies past the array's end)."""
    ks = _keys(bucket, r + 1)
    for s in range(50):
        c = _filler(n, seed + 7919 * s).copy()
        p = n - tail
        _repeats(c, 8 + 6 * r + 8, p, seed + 7919 * s)
        _colliders(c, ks[:r], 8, 6)
        _place(c, p, ks[r])
        arr, slot, rank = _model(c)
        if rank[p] != r:
            continue                                   # (a filler trigram fell into the bucket: next filler)
        if tail == 3:
            assert all(q < p for q in arr[slot[p] + 1: slot[p] + 6])
        return c
    raise AssertionError("no unit for bucket %d, %d older positions" % (bucket, r))


def _validity_units():
    units = []
    last = (1 << BITS) - 1
    for r in range(7):
        units.append(_validity_unit(1500, 2000, r, 100 + r))
        c = _validity_unit(4096, last, r, 200 + r)                       # bucket 4095 is the array's end: the reads run into the packed table
        arr, slot, _ = _model(c)
        assert slot[4093] == len(arr) - 1
        units.append(c)
    # short chunks: the unused bucket slots behind the keys hold what the sort left there
    text = np.frombuffer(b"abcabcabdabcabcab" * 300, dtype=np.uint8)
    for n in (3, 4, 5, 8, 64, 65, 200):
        units.append(_filler(n, 300 + n).copy())
        units.append(text[:n].copy())
        units.append(np.full(n, 0x5A, np.uint8))
        units.append(np.concatenate([text[:4096], text[7:7 + n]]))        # as the last chunk behind a full one
        for r in (0, 3, 6):
            if 8 + 6 * r + 3 <= n - 3:
                units.append(_validity_unit(n, 1234, r, 400 + n + r))
    # finishing-loop boundaries: R older positions of distinct colliding keys, so no step ends early. 4: nothing to finish; 5: one candidate;
    # 67 / 68 / 69 and 131 / 132 / 133: the own entry in the last lane of a step, in lane 0 of a step with no valid lane, in lane 1
    for R in (4, 5, 67, 68, 69, 131, 132, 133):
        units.append(_validity_unit(8 + 6 * R + 740, 777, R, 500 + R))
        units.append(_validity_unit(8 + 6 * R + 740, 777, R, 600 + R, tail=24))
        units.append(_validity_unit(4096, (1 << BITS) - 1, R, 700 + R))
    return units


# ---- stage boundary ---------------------------------------------------------------------------------------------------

def _stage_unit(p, L, slots, seed, bucket=3001, n=None, stride=48):
    """position p (a token start) with candidates that agree with it on exactly L bytes (L >= 3: same key) in the bucket slots given, oldest
    first; the other slots in front of them hold colliding keys. Everything else is filler."""
    n = n if n is not None else p + 64
    nc = max(slots) + 1
    ks = _keys(bucket, nc + 1)
    for s in range(50):
        c = _filler(n, seed + 7919 * s).copy()
        x = np.concatenate([np.frombuffer(ks[nc], dtype=np.uint8), _filler(40, seed + 13 + s)])   # the position's bytes
        _repeats(c, 8 + stride * nc, p, seed + 7919 * s)
        _place(c, p, x[:min(40, n - p)])
        for j in range(nc):
            at = 8 + stride * j
            if j in slots:
                _place(c, at, x[:L])
                c[at + L] = x[L] ^ 0x55                                  # the first byte that differs
            else:
                _place(c, at, ks[j])
        arr, slot, rank = _model(c)
        if rank[p] != nc:
            continue                                   # (a filler trigram fell into the bucket: next filler)
        if all(_lcp(c, 8 + stride * j, p) == L if j in slots else _lcp(c, 8 + stride * j, p) < 3 for j in range(nc)):
            return c
    raise AssertionError("no stage unit p=%d L=%d slots=%s" % (p, L, slots))


def _stage_units():
    units = []
    for p in (1500, 3000):                                 # max_len 34 / 18
        for L in range(3, 19):
            for slot in (0, 1, 2, 3, 6):                   # eager candidates 0..3, a finishing candidate
                units.append(_stage_unit(p, L, (slot,), 1000 + 20 * L + slot))
        # control: candidates in every slot, none reaches 8 bytes
        units.append(_stage_unit(p, 7, (0, 1, 2, 3, 4, 5, 6), 1900))
        units.append(_stage_unit(p, 3, (0, 3, 6), 1901))
        # ties: two candidates of the same length, the older one wins -- both eager, eager and finishing, both finishing
        for L in (7, 8, 9, 16):
            for pair in ((0, 1), (2, 3), (3, 5), (5, 6)):
                units.append(_stage_unit(p, L, pair, 2000 + 10 * L + pair[0]))
    # the chunk's end: position n - m with a candidate that matches to the end (and, behind it, on zeros as far as a compare past the
    # end would look): the limit n - p lies below, at and above 8 bytes
    for n in (700, 3000):
        for m in range(3, 18):
            for slot in (0, 3, 6):
                for s in range(50):
                    c = _stage_unit(n - m, 30, (slot,), 3000 + 20 * m + slot + 7919 * s, n=n + 40, stride=36)[:n].copy()
                    q = 8 + 36 * slot
                    c[q + m:q + 30] = 0
                    if _model(c)[2][n - m] == slot + 1 and _lcp(c, q, n - m) == m:
                        break
                else:
                    raise AssertionError("no end unit n=%d m=%d" % (n, m))
                units.append(c)
    return units


# ---- token split --------------------------------------------------------------------------------------------------------

def _split_units():
    """a match of length max_len at position p with the largest offset its token split allows (p itself: the candidate is position 0), for lane 0 and
    lane 1 of the windows where the split changes and of the four-wave kernel's segment starts: a random block of p bytes, repeated"""
    units = []
    for w in (1, 2, 4, 8, 16, 32, 21, 38, 52):
        for lane in (0, 1):
            p = 64 * w + lane
            units.append(np.resize(_filler(p, 4000 + p), 4096).copy())
            units.append(np.resize(_filler(p, 4100 + p), min(4096, p + p // 4 + 64)).copy())
    for p in (2, 5, 16, 17):                               # window 0: the per-lane form
        units.append(np.resize(_filler(max(p, 3), 4200 + p)[:p], 4096).copy())
        units.append(np.resize(_filler(max(p, 3), 4300 + p)[:p], 300).copy())
    return units


@functools.lru_cache(maxsize=None)
def _units():
    return _validity_units() + _stage_units() + _split_units()


@pytest.mark.parametrize("mode", [1, 2])
def test_lznt1_candidate_compares(oracle, gpu_ctx, mode):
    units = _units()
    for i, u in enumerate(units):
        assert len(u) < 256 or R.expected(oracle, u)[1] & 0x80, "unit %d (len %d): its first chunk is stored raw and tests nothing" % (i, len(u))
    R.check_batch(oracle, gpu_ctx, units, mode, 0, "candidate compares")
