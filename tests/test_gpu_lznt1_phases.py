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
import thresholds

pytestmark = pytest.mark.gpu
LZNT1 = 2
BITS = 12
P1, P2 = 15 * 64, 39 * 64                            # first position of parts 1 and 2 (lznt1.hip LZ4_P1, LZ4_P2: batches of 64 positions)
PARTS = ((0, P1), (P1, P2), (P2, 4096))
MAXM = 22                                            # matches that can start in one window (lznt1.hip LZ4_MAXM)
MODES = pytest.mark.parametrize("mode,serial", [(2, 0), (2, 1), (1, 0)])


def _noise(seed, n=4096):
    return bytearray(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes())


def _place(seed, key, positions, n=4096):
    d = _noise(seed, n)
    for p in positions:
        d[p:p + 3] = key
    return bytes(d[:n])


_ORACLE_OUT = {}


def _expected(oracle, u):
    """the oracle's bytes of a unit, computed once per unit and shared by every test and mode"""
    if u not in _ORACLE_OUT:
        es, exp = oracle.oracle_compress(LZNT1, u)
        assert es == 0
        _ORACLE_OUT[u] = exp
    return _ORACLE_OUT[u]


def _check(oracle, gpu_ctx, units, mode, serial, what):
    import ms_compress_amd as m
    lib = gpu_ctx.lib
    lib.mscomp_amd_debug_set_lznt1(mode)
    lib.mscomp_amd_debug_set_serial_atomics(serial)
    try:
        got, st = m.compress_units(LZNT1, units, ctx=gpu_ctx)
    finally:
        lib.mscomp_amd_debug_set_lznt1(0)
        lib.mscomp_amd_debug_set_serial_atomics(0)
    for i, (u, g, s) in enumerate(zip(units, got, st)):
        exp = _expected(oracle, u)
        assert s == 0, (what, i, len(u), s)
        assert g == exp, "%s, mode %d, serial %d, unit %d (len %d): GPU bytes differ from the oracle (%d vs %d B)" % (what, mode, serial, i, len(u), len(g), len(exp))


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


def _raw_hash(key24):
    return ((key24 * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - BITS)


_KEYS = {}


def _keys_with_raw_hash(targets, per_bucket):
    """brute force over all 2^24 keys, once: `per_bucket` keys (3 bytes, little-endian) per target value of the hash BEFORE 0 is mapped to 1"""
    if not _KEYS:
        keys = np.arange(1 << 24, dtype=np.uint64)
        h = _raw_hash(keys)
        for t in targets:
            ks = keys[h == t][:per_bucket].astype(np.uint32)
            assert len(ks) == per_bucket
            _KEYS[t] = [bytes([int(k) & 0xFF, (int(k) >> 8) & 0xFF, (int(k) >> 16) & 0xFF]) for k in ks]
    return _KEYS


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
    hdr = comp[0] | (comp[1] << 8)
    assert hdr & 0x8000, "chunk stored raw"
    end = 2 + (hdr & 0xFFF) + 1
    i, pos, T = 2, 0, 0
    per = [0] * ((n + 63) // 64)
    while i < end:
        flags = comp[i]; i += 1
        for b in range(8):
            if i >= end:
                break
            T += 1
            if flags >> b & 1:
                tok = comp[i] | (comp[i + 1] << 8); i += 2
                sh = 12
                while sh > 4 and (1 << (16 - sh)) < pos:
                    sh -= 1
                per[pos // 64] += 1
                pos += (tok & ((1 << sh) - 1)) + 3
            else:
                i += 1; pos += 1
    assert pos == n, (pos, n)
    return T, per


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
    _check(oracle, gpu_ctx, _one_key_everywhere(), mode, serial, "one key everywhere")


@MODES
def test_sort_keys_confined_to_parts_and_pairs_of_parts(oracle, gpu_ctx, mode, serial):
    _check(oracle, gpu_ctx, _keys_in_parts(), mode, serial, "keys in parts")


@MODES
def test_sort_occurrences_at_the_part_boundaries(oracle, gpu_ctx, mode, serial):
    _check(oracle, gpu_ctx, _occurrences_at_the_boundaries(), mode, serial, "occurrences at the boundaries")


@MODES
def test_sort_keys_with_raw_hash_0_1_and_4095(oracle, gpu_ctx, mode, serial):
    _check(oracle, gpu_ctx, _hash_0_1_4095(), mode, serial, "raw hash 0 / 1 / 4095")


@MODES
def test_sort_chunk_lengths(oracle, gpu_ctx, mode, serial):
    _check(oracle, gpu_ctx, _chunk_lengths(), mode, serial, "chunk lengths")


@MODES
def test_emit_windows_without_a_match_and_with_the_most_matches(oracle, gpu_ctx, mode, serial):
    _check(oracle, gpu_ctx, _windows_without_and_full_of_matches(oracle), mode, serial, "no match / 22 matches")


@MODES
def test_emit_tokens_from_the_repair_area(oracle, gpu_ctx, mode, serial):
    _check(oracle, gpu_ctx, _repair_area(), mode, serial, "repair area")


@MODES
def test_emit_after_a_cascade(oracle, gpu_ctx, mode, serial):
    _check(oracle, gpu_ctx, _cascade(), mode, serial, "cascade")


@MODES
def test_emit_every_fill_of_the_last_flag_group(oracle, gpu_ctx, mode, serial):
    _check(oracle, gpu_ctx, _last_flag_group(oracle), mode, serial, "last flag group")


@MODES
def test_emit_at_the_raw_threshold(oracle, gpu_ctx, mode, serial):
    units = _thresholds()
    sizes = sorted(len(_expected(oracle, u)) - len(u) for u in units)
    assert sizes[0] == 1 and sizes[-1] == 2, sizes            # 2-byte header + (n - 1) bytes, and the raw chunk's 2 + n
    _check(oracle, gpu_ctx, units, mode, serial, "n - 1 / raw")


@MODES
def test_emit_ragged_last_chunks(oracle, gpu_ctx, mode, serial):
    _check(oracle, gpu_ctx, _ragged_last_chunks(), mode, serial, "ragged last chunks")


@MODES
def test_repetitive_cases_64_concurrent_copies(oracle, gpu_ctx, mode, serial):
    """64 copies per batch, three passes, identical bytes in every copy of every pass (a race between the waves of a block -- sorting, or
    staging tokens while another wave still writes -- shows up in SOME copies of SOME passes)"""
    import ms_compress_amd as m
    units = _repair_area() + _cascade()[:4] + [_trigram_chunk(1), bytes([0x61]) * 4096, (b"abc" * 1366)[:4096]]
    want = [_expected(oracle, u) for u in units]
    copies = 64
    lib = gpu_ctx.lib
    lib.mscomp_amd_debug_set_lznt1(mode)
    lib.mscomp_amd_debug_set_serial_atomics(serial)
    try:
        for pas in range(3):
            got, st = m.compress_units(LZNT1, [u for u in units for _ in range(copies)], ctx=gpu_ctx)
            assert all(s == 0 for s in st)
            bad = [i for i, g in enumerate(got) if g != want[i // copies]]
            assert not bad, "pass %d, mode %d, serial %d: %d of %d copies differ from the oracle, first: copy %d of unit %d" % (pas, mode, serial, len(bad), len(got), bad[0] % copies, bad[0] // copies)
    finally:
        lib.mscomp_amd_debug_set_lznt1(0)
        lib.mscomp_amd_debug_set_serial_atomics(0)
