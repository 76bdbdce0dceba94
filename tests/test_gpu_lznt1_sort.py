"""-m gpu: the bucket sort of the four-wave LZNT1 chunk kernel against the oracle, byte for byte, in both chunk-kernel modes and with the
order-independent form of the atomics on and off. The sort ranks a chunk's positions in three parts (positions [0, 960), [960, 2496),
[2496, 4096): one wave each, one count field per part in a bucket's word) and joins the parts' ranks afterwards, so the cases sit where the
parts meet: one key in every position (every field filled to its part's length), keys confined to one part or to a pair of parts, occurrences
on either side of a part boundary, chunk lengths around the boundaries, the first and the last bucket and bucket pairs whose packed ends
straddle a dword, and many concurrent copies of the repetitive cases."""
import random

import numpy as np
import pytest

import cases
import lznt1_run as R
from lznt1_model import BITS, PART_FIRST, keys_with_raw_hash as _keys_with_raw_hash, noise as _noise, place_key as _place, straddling_buckets

pytestmark = pytest.mark.gpu
P1, P2 = PART_FIRST[1:]                              # first position of parts 1 and 2
PARTS = ((0, P1), (P1, P2), (P2, 4096))


def _one_key_everywhere():
    return [bytes([0x61]) * 4096, bytes(4096)] + [bytes([0x5A]) * n for n in (4095, 4094, 4000, 2500, 2497, 1000, 961, 100)] + [bytes([7]) * (2 * 4096 + 1777)]


def _keys_in_parts():
    units = []
    key = b"\x11\x22\x33"
    inside = [[a + 7, a + 200, (a + b) // 2, b - 300, b - 9] for a, b in PARTS]          # five occurrences well inside each part
    for mask in range(1, 8):                                                             # one part, every pair of parts, all three
        pos = [p for i in range(3) if mask >> i & 1 for p in inside[i]]
        units.append(_place(100 + mask, key, pos))
        units.append(_place(110 + mask, key, pos) + _place(120 + mask, key, pos[::-1]))  # (and as two chunks of one unit)
    # occurrences that straddle a part boundary by one position either side: a run of four equal bytes at b - 1 holds the key (x, x, x) at
    # b - 1 and b alone; an older occurrence in front gives both something to find. Then the same with occurrences behind the boundary too.
    for b in (P1, P2):
        for extra in ((), (b + 300, 4000)):
            d = _noise(200 + b + len(extra))
            for p in (50,) + tuple(extra):
                d[p:p + 3] = b"\xEE\xEE\xEE"
            d[b - 1:b + 3] = b"\xEE\xEE\xEE\xEE"
            units.append(bytes(d))
        # the last occurrence wholly in front of the boundary (ends at b - 1), the next one starting at b; and three in a row across it
        units.append(_place(300 + b, key, (b - 3, b)))
        units.append(_place(310 + b, key, (40, b - 3, b, b + 3, 4090)))
        units.append(_place(320 + b, key, (b - 1,)) + _place(321 + b, key, (10, b - 2, b + 1)))
    # a long repeat across each boundary, and across both
    rnd = random.Random(9)
    units += [cases.periodic_with_mutations(n=4096, period=p, seed=70 + p, gap=(150, 900)) for p in (1, 2, 3, 64, 959, 960, 1536)]
    units.append(cases.family("lz", 3 * 4096, rnd))
    return units


def _lengths_at_the_boundaries():
    rnd = random.Random(4)
    ns = list(range(958, 963)) + list(range(2494, 2499)) + [3, 1, 2, 4, 5, 31, 62, 63, 64, 65, 4093, 4094, 4095, 4096]
    units = []
    for n in ns:
        for kind in ("words", "two", "run", "lz"):
            units.append(cases.family(kind, n, rnd))
            units.append(cases.family(kind, 4096 + n, rnd))                              # (as the ragged last chunk of a unit)
    return units


def _first_last_and_straddling_buckets():
    rng = np.random.default_rng(21)
    strad = straddling_buckets(4)
    targets = [0, 1, (1 << BITS) - 1, (1 << BITS) - 2] + strad + [h - 1 for h in strad]
    kb = _keys_with_raw_hash(sorted(set(targets)), 6)
    units = []
    groups = [[0, 1], [0], [1], [(1 << BITS) - 1], [(1 << BITS) - 2, (1 << BITS) - 1], [0, 1, (1 << BITS) - 1]] + [[h - 1, h] for h in strad]
    for g in groups:
        ks = [k for t in g for k in kb[t]]
        seq = b"".join(ks[i] for i in rng.integers(0, len(ks), 1366))[:4096]             # keys of the group in all three parts
        units.append(seq)
        noisy = bytearray(seq)
        for i in rng.integers(0, len(noisy), 300):
            noisy[i] = int(rng.integers(0, 256))
        units.append(bytes(noisy))
        units.append(seq[:P2 + 1])
    return units


def _repetitive():
    return ([bytes([0x61]) * 4096, bytes([0x5A]) * 2497, bytes([0x5A]) * 961, (b"ab" * 2048), (b"abc" * 1366)[:4096]]
            + [cases.periodic_with_mutations(n=8192, period=p, seed=80 + p, gap=(100, 900)) for p in (1, 2, 3, 7, 64, 960)]
            + [cases.few_distances(n=8192, dists=(1, 2, 3, 959, 960, 961), seed=90, run=(40, 900)),
               cases.few_distances(n=8192, dists=(2495, 2496, 1536, 1600, 16), seed=91, run=(100, 1200))])


MODES = pytest.mark.parametrize("mode,serial", [(1, 0), (2, 0), (1, 1), (2, 1)])


@MODES
def test_one_key_in_every_position(oracle, gpu_ctx, mode, serial):
    R.check_batch(oracle, gpu_ctx, _one_key_everywhere(), mode, serial, "one key everywhere")


@MODES
def test_keys_confined_to_parts_and_across_part_boundaries(oracle, gpu_ctx, mode, serial):
    R.check_batch(oracle, gpu_ctx, _keys_in_parts(), mode, serial, "keys in parts")


@MODES
def test_chunk_lengths_around_the_part_boundaries(oracle, gpu_ctx, mode, serial):
    R.check_batch(oracle, gpu_ctx, _lengths_at_the_boundaries(), mode, serial, "lengths at the boundaries")


@MODES
def test_first_last_and_dword_straddling_buckets(oracle, gpu_ctx, mode, serial):
    R.check_batch(oracle, gpu_ctx, _first_last_and_straddling_buckets(), mode, serial, "first / last / straddling buckets")


@MODES
def test_repetitive_cases_many_concurrent_copies(oracle, gpu_ctx, mode, serial):
    """48 concurrent copies per batch, three passes, identical bytes in every copy of every pass (a race between the sorting waves shows up in
    SOME copies of SOME passes)."""
    R.check_batch(oracle, gpu_ctx, _repetitive(), mode, serial, "repetitive", copies=48, passes=3)
