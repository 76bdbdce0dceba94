"""-m gpu: the LZNT1 match dictionary (12-bit hash of the 3-byte key; the four-wave kernel keeps the bucket ends as packed
12-bit fields) against the oracle, in both chunk-kernel modes: keys that land in the first and last buckets and on bucket
pairs whose ends straddle a dword of the packed table, one full bucket, no repeated key at all, ragged last chunks and the
seam-stress units of the four-wave kernel."""
import numpy as np
import pytest

import lznt1_run as R
from lznt1_model import BITS, keys_by_bucket as _keys_by_bucket, straddling_buckets as _straddling_buckets

pytestmark = pytest.mark.gpu


def _units():
    rng = np.random.default_rng(12)
    targets = [1, 2, (1 << BITS) - 1] + _straddling_buckets(6)
    kb = _keys_by_bucket(targets, 6)
    assert all(len(v) == 6 for v in kb.values())
    units = []
    # keys of one bucket in a random order (distinct keys collide in the bucket, equal ones match), with and without noise
    for t in targets:
        seq = b"".join(kb[t][i] for i in rng.integers(0, 6, 3000))
        units.append(np.frombuffer(seq, dtype=np.uint8))
        noisy = bytearray(seq)
        for i in rng.integers(0, len(noisy), 400):
            noisy[i] = int(rng.integers(0, 256))
        units.append(np.frombuffer(bytes(noisy), dtype=np.uint8))
    # all target buckets mixed, and pairs of neighbouring buckets (h - 1, h)
    allk = [k for t in targets for k in kb[t]]
    units.append(np.frombuffer(b"".join(allk[i] for i in rng.integers(0, len(allk), 6000)), dtype=np.uint8))
    for h in _straddling_buckets(6)[:3]:
        pair = _keys_by_bucket([h - 1, h], 4)
        ks = pair[h - 1] + pair[h]
        units.append(np.frombuffer(b"".join(ks[i] for i in rng.integers(0, len(ks), 2500)), dtype=np.uint8))
    # one repeated byte: one bucket of 4094 entries per chunk
    units += [np.full(4096, 0x61, np.uint8), np.full(3 * 4096 + 17, 0, np.uint8)]
    # every trigram of the chunk distinct
    for seed in range(100):
        r = np.random.default_rng(1000 + seed).integers(0, 256, 4096, dtype=np.uint8)
        k = r[:-2].astype(np.uint32) | (r[1:-1].astype(np.uint32) << 8) | (r[2:].astype(np.uint32) << 16)
        if len(np.unique(k)) == len(k):
            units.append(r)
            break
    else:
        raise AssertionError("no chunk with distinct trigrams found")
    # ragged last chunks of a compressible unit: n = 1..5 and 4093..4096
    text = np.frombuffer(b"the match dictionary of a chunk, keyed by a hash of three bytes. " * 400, dtype=np.uint8)
    for n in (1, 2, 3, 4, 5, 4093, 4094, 4095, 4096):
        units.append(text[: 2 * 4096 + n].copy())
        units.append(text[:n].copy())
    # seam stress of the four-wave kernel (test_lznt1_chunk_kernels_agree): periodic data that re-synchronises late
    for period in (3, 5, 7):
        base = rng.integers(0, 256, period, dtype=np.uint8)
        units.append(np.tile(base, 20000 // period + 1)[:20000])
    return units


@pytest.mark.parametrize("mode", [1, 2])
def test_lznt1_dictionary_buckets(oracle, gpu_ctx, mode):
    R.check_batch(oracle, gpu_ctx, _units(), mode, 0, "dictionary buckets")
