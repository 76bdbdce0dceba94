"""GPU: the addressing of the four-wave LZNT1 chunk kernel (csrc/lznt1.hip lznt1_chunk4_kernel). The kernel keeps what its sort and parse never
read -- the addresses of the chunk's slot and of its entry in the size index, the chunk and wave numbers -- in the lanes of one vector register
and fetches them when the parse is over; a mistake there leaves the matching alone and sends a chunk's bytes, records or size to the wrong place,
or reads the wrong source, length or unit. So the batches here are about where things are, not what they hold: units that end inside, at and one
byte behind a chunk boundary at odd input offsets (byte-wise staging, ragged `n`, the unit lookup across nine units), a raw chunk between two
compressed ones in one unit, two chunks whose seam repairs write the second record area, and the same chunks at indices other than 0.
Every batch runs through a plan with host tables, a plan with device tables whose bound lies above the real chunk count (the surplus blocks return
at once) and the serial-atomics instance, twice each with identical bytes demanded, and every unit is compared byte for byte with the oracle."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
LZNT1 = 2
GUARD = 0xEE
SEAMS = (21 * 64, 38 * 64, 52 * 64)                  # first position of segments 1 to 3 (lznt1.hip LZ4_B1 / B2 / B3: windows of 64 positions)
PATHS = pytest.mark.parametrize("path", ["host-tables", "device-tables", "serial-atomics"])


def _noise(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _text(n, skip=0):
    from ms_compress_amd import corpus
    return corpus.by_name("mozilla", skip + n + 1000).tobytes()[skip: skip + n]


def _nine_units():
    """(a) lengths around the chunk boundaries, the first three below the shortest match"""
    sizes = (1, 2, 3, 64, 4095, 4096, 4097, 8209, 20480)
    data = _text(sum(sizes))
    out, pos = [], 0
    for s in sizes:
        out.append(data[pos: pos + s])
        pos += s
    return out


def _raw_between():
    """(b) one unit of three chunks: compressible, random (stored raw), compressible"""
    return [_text(4096) + _noise(3, 4096) + _text(4096, 50_000)]


def _seam_unit():
    """(c) two chunks in which every position lies inside a match of one short distance: the speculative parse of a segment starts at its first
    window, the real one arrives there inside a match, and the seam's repair writes its windows' tokens into the second record area"""
    return [cases.periodic_with_mutations(n=8192, period=301, seed=9, gap=(150, 400))]


def _token_starts(stream):
    """per chunk of an LZNT1 stream: the set of positions at which a token of the chunk starts (None for a raw chunk)"""
    out, i = [], 0
    while i + 2 <= len(stream):
        hdr = stream[i] | (stream[i + 1] << 8)
        if hdr == 0:
            break
        end = i + 2 + (hdr & 0xFFF) + 1
        if not hdr & 0x8000:
            out.append(None)
            i = end
            continue
        starts, pos, j = set(), 0, i + 2
        while j < end:
            flags = stream[j]
            j += 1
            for b in range(8):
                if j >= end:
                    break
                starts.add(pos)
                if (flags >> b) & 1:
                    tok = stream[j] | (stream[j + 1] << 8)
                    j += 2
                    shift = 12 if pos <= 16 else 12 - ((pos - 1).bit_length() - 4)
                    pos += (tok & ((1 << shift) - 1)) + 3
                else:
                    j += 1
                    pos += 1
        out.append(starts)
        i = end
    return out


_ORACLE_OUT = {}


def _expected(oracle, u):
    """the oracle's bytes of a unit, computed once per unit and shared by every test and path"""
    if u not in _ORACLE_OUT:
        es, exp = oracle.oracle_compress(LZNT1, u)
        assert es == 0
        _ORACLE_OUT[u] = exp
    return _ORACLE_OUT[u]


def _layout(units):
    """input offsets odd (unit i starts at an odd byte, a gap of 1 or 2 behind the unit before), capacities with guard bytes between them"""
    import ms_compress_amd as m
    in_off, pos = [], 1
    for u in units:
        in_off.append(pos)
        pos += len(u)
        pos += 1 if pos % 2 == 0 else 2
    blob = np.zeros(pos + 32, np.uint8)
    for u, o in zip(units, in_off):
        blob[o: o + len(u)] = np.frombuffer(u, np.uint8)
    caps = [m.max_compressed_size(LZNT1, len(u)) + 2 for u in units]
    out_off, opos = [], 16
    for c in caps:
        out_off.append(opos)
        opos += c + 16
    assert all(o % 2 == 1 for o in in_off)
    return blob, np.array(in_off, np.uint64), np.array([len(u) for u in units], np.uint64), np.array(out_off, np.uint64), np.array(caps, np.uint64), opos


def _dt(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def _run(gpu_ctx, units, path):
    """the batch executed twice by one plan: [(lengths, statuses, output bytes)] * 2"""
    import torch
    import ms_compress_amd as m
    blob, in_off, lens, out_off, caps, out_total = _layout(units)
    n = len(units)
    d_in = torch.from_numpy(blob).cuda()
    d_len = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
    lib = gpu_ctx.lib
    if path == "device-tables":
        # eight chunks more than the batch has: the blocks past the real count run past_real_chunks
        plan = m.CompressDevPlan(gpu_ctx, LZNT1, n, int(lens.sum()) + 8 * 4096, int(lens.max()))
        tabs = [_dt(a) for a in (in_off, lens, out_off, caps)]
    else:
        plan = m.Plan(gpu_ctx, LZNT1, in_off, lens, out_off, caps)
    lib.mscomp_amd_debug_set_lznt1(2)
    lib.mscomp_amd_debug_set_serial_atomics(1 if path == "serial-atomics" else 0)
    res = []
    try:
        for _ in range(2):
            d_out = torch.full((out_total,), GUARD, dtype=torch.uint8, device="cuda")
            d_len.fill_(-1)
            d_st.fill_(77)
            if path == "device-tables":
                plan.execute(d_in, tabs[0], tabs[1], d_out, tabs[2], tabs[3], d_len, d_st)
            else:
                plan.execute(d_in, d_out, d_len, d_st)
            torch.cuda.synchronize()
            res.append((d_len.cpu().numpy().copy(), d_st.cpu().numpy().copy(), d_out.cpu().numpy().copy()))
    finally:
        lib.mscomp_amd_debug_set_lznt1(0)
        lib.mscomp_amd_debug_set_serial_atomics(0)
        plan.close()
    return res, out_off, caps


def _check(oracle, gpu_ctx, units, path, what, first=0):
    """units[first:] against the oracle (the units in front only move the chunk indices), both executions, and nothing written outside a capacity"""
    res, out_off, caps = _run(gpu_ctx, units, path)
    for k, (ln, st, out) in enumerate(res):
        inside = np.zeros(len(out), bool)
        for i, u in enumerate(units):
            o = int(out_off[i])
            inside[o: o + int(caps[i])] = True
            assert st[i] == 0, (what, path, k, i, len(u), st[i])
            if i < first:
                continue
            exp = _expected(oracle, u)
            got = bytes(out[o: o + int(ln[i])])
            assert got == exp, "%s, %s, execution %d, unit %d (len %d): GPU bytes differ from the oracle (%d vs %d B)" % (what, path, k, i, len(u), len(got), len(exp))
        assert (out[~inside] == GUARD).all(), (what, path, k, np.nonzero(out[~inside] != GUARD)[0][:8])
    assert all((a == b).all() for a, b in zip(res[0], res[1])), "%s, %s: two executions of one plan differ" % (what, path)


@PATHS
def test_nine_units_at_odd_offsets(oracle, gpu_ctx, path):
    _check(oracle, gpu_ctx, _nine_units(), path, "nine units")


@PATHS
def test_raw_chunk_between_two_compressed_ones(oracle, gpu_ctx, path):
    units = _raw_between()
    kinds = [s is None for s in _token_starts(_expected(oracle, units[0]))]
    assert kinds == [False, True, False], kinds                            # the unit is what it claims
    _check(oracle, gpu_ctx, units, path, "raw between compressed")


@PATHS
def test_seam_repairs_in_two_chunks(oracle, gpu_ctx, path):
    units = _seam_unit()
    chunks = _token_starts(_expected(oracle, units[0]))
    assert len(chunks) == 2
    for starts in chunks:                                                  # a seam no token starts at is repaired by the segment in front of it
        assert starts is not None and any(s not in starts for s in SEAMS), sorted(starts)[:8]
    _check(oracle, gpu_ctx, units, path, "seam repairs")


@PATHS
def test_same_chunks_alone_and_as_the_tail_of_40(oracle, gpu_ctx, path):
    tail = _raw_between() + _seam_unit()                                   # 3 + 2 chunks
    _check(oracle, gpu_ctx, tail, path, "five chunks alone")
    front = [_text(4096 * 30, 100_000), _text(4096 * 4 + 5, 300_000)]     # 30 + 5 chunks in front: the tail's chunks are 35 to 39
    assert sum((len(u) + 4095) // 4096 for u in front + tail) == 40
    _check(oracle, gpu_ctx, front + tail, path, "five chunks behind 35", first=len(front))
