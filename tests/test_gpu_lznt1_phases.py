"""-m gpu: the sort and the emission of the four-wave LZNT1 chunk kernel against the oracle, byte for byte. Chunk-kernel mode 2 with the
order-independent form of the atomics off and on; mode 1 once as the control. Units are one or two chunks.

Sort (lznt1.hip section B): a position is hashed once, the hash rides beside the rank; the chunk's 64 batches of 64 positions are ranked in
three parts, first positions P1 and P2 below, one count field per part. The cases sit where the parts meet and where a field is full.
Emission (sections D0 / D1): a wave copies the match tokens of its 16 windows from the records (speculative or repair area per window) into
LDS and emits from there. The cases: windows without a match, windows with the most matches a window can hold, tokens in the repair area,
the cascade, every fill of the last flag group, the raw / compressed decision at its threshold, ragged last chunks."""
import random

import numpy as np
import pytest

import cases
import lznt1_model as M
import lznt1_run as R
import thresholds
from lznt1_model import MAXM, PART_FIRST, keys_with_raw_hash as _keys_with_raw_hash, noise as _noise, place_key as _place
from lznt1_run import expected as _expected

pytestmark = pytest.mark.gpu
P1, P2 = PART_FIRST[1:]                              # first position of parts 1 and 2
PARTS = ((0, P1), (P1, P2), (P2, 4096))
MODES = pytest.mark.parametrize("mode,serial", [(2, 0), (2, 1), (1, 0)])


# ---------------------------------------------------------------------------------------------------------------------
# sort
# ---------------------------------------------------------------------------------------------------------------------
def _one_key_everywhere():
    """every field filled to its part's length: a full chunk, and chunks cut around every part boundary (a key needs three bytes, so the last
    key of a chunk of n bytes sits at n - 3: lengths b - 1 .. b + 3 put it one position either side of b)"""
    ns = [4096] + [b + d for b in (P1, P2) for d in (-1, 0, 1, 2, 3)]
    units = [bytes([0x61]) * n for n in ns] + [bytes(n) for n in ns[:3]]
    # the same key everywhere, but matches too short to swallow the chunk: a key of three equal bytes broken by a changing byte every fourth
    units += [bytes(b for i in range(n // 4 + 1) for b in (0x5A, 0x5A, 0x5A, i & 0xFF))[:n] for n in ns]
    return units


def _keys_in_parts():
    units = []
    key = b"\x11\x22\x33"
    inside = [[a + 7, a + 200, (a + b) // 2, b - 300, b - 9] for a, b in PARTS]
    for mask in range(1, 8):                                                             # each part, every pair of parts, all three
        pos = [p for i in range(3) if mask >> i & 1 for p in inside[i]]
        units.append(_place(100 + mask, key, pos))
        units.append(_place(110 + mask, key, pos) + _place(120 + mask, key, pos[::-1]))  # (and as two chunks of one unit)
    return units


def _occurrences_at_the_boundaries():
    units = []
    key = b"\x44\x55\x66"
    for b in (P1, P2):
        for occ in ((b - 1,), (b,), (b + 1,), (b - 1, b + 2), (b - 3, b), (b - 3, b, b + 3)):
            units.append(_place(200 + b + len(occ), key, (40,) + occ))                   # an older occurrence in front gives them something to find
            units.append(_place(210 + b + len(occ), key, occ + (4000,)))
        d = _noise(300 + b)
        d[50:53] = b"\xEE\xEE\xEE"
        d[b - 1:b + 3] = b"\xEE\xEE\xEE\xEE"                                             # the key at b - 1 and at b alone, overlapping
        units.append(bytes(d))
    return units


def _hash_0_1_4095():
    rng = np.random.default_rng(31)
    kb = _keys_with_raw_hash([0, 1, 4095], 6)
    units = []
    for g in ([0], [1], [4095], [0, 1], [0, 1, 4095]):
        ks = [k for t in g for k in kb[t]]
        seq = b"".join(ks[i] for i in rng.integers(0, len(ks), 1366))[:4096]             # the group's keys in all three parts
        units += [seq, seq[:P2 + 1], seq[:P1 + 2]]
        noisy = bytearray(seq)
        for i in rng.integers(0, len(noisy), 300):
            noisy[i] = int(rng.integers(0, 256))
        units.append(bytes(noisy))
    return units


def _chunk_lengths():
    rnd = random.Random(6)
    units = []
    for n in (1, 2, 3, 4, 63, 64, 65, 4095, 4096):
        for kind in ("words", "two", "run", "lz"):
            units.append(cases.family(kind, n, rnd))
    return units


# ---------------------------------------------------------------------------------------------------------------------
# emission
# ---------------------------------------------------------------------------------------------------------------------
def _trigram_chunk(shift=0, n=4096):
    """64 trigrams (A_i, B_i, C_i), each followed by a byte that no trigram starts with: four windows without any match. Behind them the
    trigrams back to back in changing orders: every match is exactly three bytes long (the byte behind a trigram differs from every earlier
    occurrence's), so a window of 64 positions holds 22 or 21 match starts. `shift` literal bytes in front move the starts against the windows."""
    tri = [bytes([0x80 + i, 0xC0 + i, 0x40 + i]) for i in range(64)]
    out = bytearray(bytes(range(shift)))                                                 # (values below 0x40: no trigram byte)
    for i in range(64):
        out += tri[i] + bytes([i & 0x3F])
    for stride in (1, 5, 7, 11, 13, 17, 19, 23, 25, 29, 31, 35, 37, 41, 43, 47, 49, 53, 55, 59, 61):
        for i in range(64):
            out += tri[(i * stride) % 64]
    return bytes(out[:n])


def _match_counts_per_window(comp, n):
    """from the oracle's bytes of ONE compressed chunk: (tokens, list of match starts per window of 64 positions)"""
    _, _, raw, tokens = next(M.walk_stream(comp))
    assert not raw, "chunk stored raw"
    assert tokens[-1][0] + (tokens[-1][1] or 1) == n, (tokens[-1], n)
    per = [0] * ((n + 63) // 64)
    for pos, length in tokens:
        per[pos // 64] += length > 0
    return len(tokens), per


def _windows_without_and_full_of_matches(oracle):
    units = [_trigram_chunk(s) for s in (0, 1, 2)] + [_trigram_chunk(0, n) for n in (4095, 1024 + 65, 2048 + 1)]
    T, per = _match_counts_per_window(_expected(oracle, units[0]), 4096)
    assert per[:4] == [0, 0, 0, 0] and max(per) == MAXM and all(c in (MAXM - 1, MAXM) for c in per[4:]), per
    assert all(max(per[16 * j:16 * j + 16]) == MAXM for j in range(4)), "a full window in every wave's 16 windows"
    # a compressible chunk with stretches of noise: windows without a match between windows with some
    d = bytearray(cases.family("lz", 4096, random.Random(12)))
    for a in (64, 1024 - 32, 2048, 3072 + 17, 4096 - 130):
        d[a:a + 130] = _noise(a, 130)
    units.append(bytes(d))
    return units


def _repair_area():
    """seams that do not re-synchronise at once: the repairing wave's tokens land in the second record area"""
    return ([cases.periodic_with_mutations(n=8192, period=p, seed=80 + p, gap=(100, 900)) for p in (1, 2, 3, 7, 64, 960)]
            + [cases.few_distances(n=8192, dists=(1, 2, 3, 959, 960, 961), seed=90, run=(40, 900)),
               cases.few_distances(n=8192, dists=(2495, 2496, 1536, 1600, 16), seed=91, run=(100, 1200))])


def _cascade():
    """noise, then one byte repeated to the chunk's end. Behind position 2048 a match is at most 18 bytes long, so the true parse walks the run in
    steps of 18 from where the noise ends; a wave that starts a segment speculatively at a window boundary walks it in steps of 18 from there.
    Unless the two starts agree modulo 18 they never meet: the repair runs through the whole segment behind the seam, and the segment after
    that is walked again by wave 0 (the cascade). Several noise lengths, so that no choice of segment boundaries agrees with all of them."""
    units = []
    for k in (2100, 2101, 2107, 2113):
        units.append(bytes(_noise(k, k)) + bytes([0x61]) * (4096 - k))
        units.append(bytes(_noise(k + 1, k)) + (b"xy" * 2048)[:4096 - k])
    return units


def _last_flag_group(oracle):
    """k different literals, then a run: the token count moves by one with k, so eight consecutive k give every fill of the last flag group"""
    units = [bytes(range(0x80, 0x80 + k)) + bytes([0x33]) * 300 + bytes(range(0x10, 0x15)) for k in range(1, 17)]
    fills = {_match_counts_per_window(_expected(oracle, u), len(u))[0] % 8 for u in units}
    assert {0, 1, 7} <= fills, fills
    return units


def _thresholds():
    """a chunk that compresses to exactly n - 1 bytes and one that goes raw at n (tests/golden/thresholds.json, rebuilt from their recipes)"""
    want = {"lznt1-4096-only-d-1-s45004", "lznt1-4096-only-d-1-s45003", "lznt1-4096-only-d+0-s45002", "lznt1-4096-only-d+1-s45007",
            "lznt1-4095-only-d-1-s44006", "lznt1-4095-only-d+0-s44001"}
    rs = [r for r in thresholds.load()["cases"] if r["id"] in want]
    assert len(rs) == len(want)
    return [thresholds.build(r) for r in rs]


def _ragged_last_chunks():
    rnd = random.Random(15)
    full = [cases.family("lz", 4096, rnd), _trigram_chunk(0), bytes(_noise(77))]
    return [f + cases.family(kind, t, rnd) for f in full for t in (1, 2, 65) for kind in ("run", "lz")]


# ---------------------------------------------------------------------------------------------------------------------
@MODES
def test_sort_one_key_in_every_position(oracle, gpu_ctx, mode, serial):
    R.check_batch(oracle, gpu_ctx, _one_key_everywhere(), mode, serial, "one key everywhere")


@MODES
def test_sort_keys_confined_to_parts_and_pairs_of_parts(oracle, gpu_ctx, mode, serial):
    R.check_batch(oracle, gpu_ctx, _keys_in_parts(), mode, serial, "keys in parts")


@MODES
def test_sort_occurrences_at_the_part_boundaries(oracle, gpu_ctx, mode, serial):
    R.check_batch(oracle, gpu_ctx, _occurrences_at_the_boundaries(), mode, serial, "occurrences at the boundaries")


@MODES
def test_sort_keys_with_raw_hash_0_1_and_4095(oracle, gpu_ctx, mode, serial):
    R.check_batch(oracle, gpu_ctx, _hash_0_1_4095(), mode, serial, "raw hash 0 / 1 / 4095")


@MODES
def test_sort_chunk_lengths(oracle, gpu_ctx, mode, serial):
    R.check_batch(oracle, gpu_ctx, _chunk_lengths(), mode, serial, "chunk lengths")


@MODES
def test_emit_windows_without_a_match_and_with_the_most_matches(oracle, gpu_ctx, mode, serial):
    R.check_batch(oracle, gpu_ctx, _windows_without_and_full_of_matches(oracle), mode, serial, "no match / 22 matches")


@MODES
def test_emit_tokens_from_the_repair_area(oracle, gpu_ctx, mode, serial):
    R.check_batch(oracle, gpu_ctx, _repair_area(), mode, serial, "repair area")


@MODES
def test_emit_after_a_cascade(oracle, gpu_ctx, mode, serial):
    R.check_batch(oracle, gpu_ctx, _cascade(), mode, serial, "cascade")


@MODES
def test_emit_every_fill_of_the_last_flag_group(oracle, gpu_ctx, mode, serial):
    R.check_batch(oracle, gpu_ctx, _last_flag_group(oracle), mode, serial, "last flag group")


@MODES
def test_emit_at_the_raw_threshold(oracle, gpu_ctx, mode, serial):
    units = _thresholds()
    sizes = sorted(len(_expected(oracle, u)) - len(u) for u in units)
    assert sizes[0] == 1 and sizes[-1] == 2, sizes            # 2-byte header + (n - 1) bytes, and the raw chunk's 2 + n
    R.check_batch(oracle, gpu_ctx, units, mode, serial, "n - 1 / raw")


@MODES
def test_emit_ragged_last_chunks(oracle, gpu_ctx, mode, serial):
    R.check_batch(oracle, gpu_ctx, _ragged_last_chunks(), mode, serial, "ragged last chunks")


@MODES
def test_repetitive_cases_64_concurrent_copies(oracle, gpu_ctx, mode, serial):
    """64 copies per batch, three passes, identical bytes in every copy of every pass (a race between the waves of a block -- sorting, or
    staging tokens while another wave still writes -- shows up in SOME copies of SOME passes)"""
    units = _repair_area() + _cascade()[:4] + [_trigram_chunk(1), bytes([0x61]) * 4096, (b"abc" * 1366)[:4096]]
    R.check_batch(oracle, gpu_ctx, units, mode, serial, "repetitive", copies=64, passes=3)
