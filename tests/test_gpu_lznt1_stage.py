"""Section A of the LZNT1 chunk kernels (csrc/lznt1.hip): the chunk is staged into LDS with 16-byte loads where its first byte is 16-byte
aligned and byte by byte elsewhere, and LDS from byte n on is zero. The batch here is laid out by the test (lznt1_run.run_plan's odd offsets do
not reach the even alignments): a unit starts at every src & 15 from 0 to 15, with chunk lengths of 1, 2, 3, 15, 16, 17, 31, 4081, 4095 and 4096
bytes and two-chunk units whose second chunk has 1 and 4095 bytes; the first unit begins at the first byte of the input tensor and the last one
ends at its last byte (the tensor has exactly the batch's bytes: nothing of the test's lies behind it). The bytes in front of and behind every
unit repeat one 16-byte pattern, and every unit ends with the same pattern, of which an earlier copy inside the unit is followed by the pattern's
first bytes: a gap byte that leaked into LDS below n would change a literal (or a byte of a raw chunk), one that leaked into the zeroed tail
would continue the last match. (The kernels cap every compare at max_len <= n - p, so a wrong byte behind n may stay without effect on the
output; what the test can show there, it shows.) Every unit is compared byte for byte with the oracle in both kernel modes through a host-table
plan, a device-table plan and the serial-atomics instance, with guard bytes around every capacity. A staging that loads 16 bytes at any alignment
(tools/dev/not_kept/lznt1_stage16.patch.txt, profiles/HISTORY.md round 21) passes the same file."""
import functools

import numpy as np
import pytest

import lznt1_model as M
import lznt1_run as R

LENS = (1, 2, 3, 15, 16, 17, 31, 4081, 4095, 4096, 4096 + 1, 4096 + 4095)
PATTERN = np.array([0xC3, 0x5A, 0x17, 0xE8, 0x91, 0x2D, 0xF6, 0x4B, 0xA0, 0x7E, 0x39, 0xD4, 0x66, 0x0F, 0xB2, 0x85], np.uint8)


def _chunk(n, seed, last):
    """a chunk of n bytes that ends with the pattern; where there is room, an earlier copy of it is followed by its first 8 bytes. A long last
    chunk has a periodic stretch, so that it is stored compressed and ends with a match; the first chunk of a two-chunk unit and the short
    chunks are stored raw: every staged byte is in the output."""
    c = M.filler(n, seed).copy()
    if n >= 64:
        if last and n >= 4000:
            c[1000:n - 100] = np.resize(M.filler(24, seed + 5), n - 1100)
        M.place(c, 8, np.concatenate([PATTERN, PATTERN[:8]]).tobytes())
        c[n - 16:] = PATTERN
    else:
        c[:] = np.resize(PATTERN, (n + 15) // 16 * 16)[-n:]               # the pattern repeated, cut in front: it ends where the pattern ends
    return c


@functools.lru_cache(maxsize=None)
def _unit(length):
    """the unit of a length: every chunk built by itself (an LZNT1 chunk sees only itself)"""
    return b"".join(_chunk(min(4096, length - o), 77 + length + o, o + 4096 >= length).tobytes() for o in range(0, length, 4096))


@functools.lru_cache(maxsize=None)
def _layout():
    """(input bytes, offsets, units): alignments 0..15 x LENS, gaps of 17 to 32 pattern bytes, the first unit at byte 0, the last one at the end"""
    units, offs, parts, pos = [], [], [], 0
    for a in range(16):
        for length in LENS:
            gap = 0 if not units else 17 + (a - (pos + 17)) % 16
            parts.append(np.resize(PATTERN, gap))
            pos += gap
            assert pos % 16 == a
            u = _unit(length)
            offs.append(pos)
            units.append(u)
            parts.append(np.frombuffer(u, np.uint8))
            pos += length
    blob = np.concatenate(parts)
    assert len(blob) == pos == offs[-1] + len(units[-1]) and offs[0] == 0
    return blob, offs, units


def test_layout_is_what_it_claims():
    blob, offs, units = _layout()
    assert len(units) == 16 * len(LENS)
    assert sorted({(o % 16, len(u)) for o, u in zip(offs, units)}) == [(a, n) for a in range(16) for n in sorted(LENS)]
    assert offs[0] == 0 and offs[-1] + len(units[-1]) == len(blob)
    for i, (o, u) in enumerate(zip(offs, units)):
        assert bytes(blob[o:o + len(u)]) == u
        last = len(u) - (len(u) - 1) // 4096 * 4096                       # bytes of the last chunk
        k = min(16, last)
        assert u[-k:] == PATTERN.tobytes()[-k:]                           # the unit ends with the pattern's end ...
        if i + 1 < len(units):
            gap = blob[o + len(u):offs[i + 1]]
            assert 17 <= len(gap) <= 32 and bytes(gap) == np.resize(PATTERN, len(gap)).tobytes()   # ... and the pattern starts again behind it
        if last >= 64:
            first = len(u) - last
            assert u[first + 8:first + 32] == PATTERN.tobytes() + PATTERN.tobytes()[:8]             # the earlier copy, continued as the gap is


def test_the_last_match_of_a_long_chunk_stops_at_the_chunks_end(oracle):
    """the model's parse: the chunk ends with a match of the pattern against its earlier copy, cut by the chunk's end"""
    for length in (4081, 4095, 4096, 4096 + 4095):
        u = _unit(length)
        streams = M.chunk_streams(R.expected(oracle, u))
        c = np.frombuffer(u, np.uint8)[(length - 1) // 4096 * 4096:]
        n, t = len(c), M.parse(c)
        assert t.get(n - 16) == 16, (length, t.get(n - 16))
        assert streams[-1][1] & 0x80 and M.token_lengths(streams[-1]) == t, length
        assert all(not st[1] & 0x80 for st in streams[:-1]), length          # the first chunk of two: raw
    for length in (1, 2, 3, 15, 16, 17, 4096 + 1):                            # raw: all their bytes are in the output
        assert not M.chunk_streams(R.expected(oracle, _unit(length)))[-1][1] & 0x80, length
    st = M.chunk_streams(R.expected(oracle, _unit(31)))[0]                    # 31 bytes of the pattern: a match 16 bytes back that runs to the end
    assert st[1] & 0x80 and M.token_lengths(st) == M.parse(np.frombuffer(_unit(31), np.uint8)) and M.token_lengths(st)[16] == 15


@pytest.mark.gpu
@pytest.mark.parametrize("path", R.PATHS)
@pytest.mark.parametrize("mode", [1, 2])
def test_lznt1_staging_at_every_alignment(oracle, gpu_ctx, mode, path):
    import torch
    import ms_compress_amd as m
    blob, offs, units = _layout()
    want = [R.expected(oracle, u) for u in units]
    caps = [m.max_compressed_size(R.LZNT1, len(u)) + 2 for u in units]
    out_off, total = [], 16
    for cp in caps:
        out_off.append(total)
        total += cp + 16
    in_off, lens, out_off, caps = (np.array(a, np.uint64) for a in (offs, [len(u) for u in units], out_off, caps))
    inside = np.zeros(total, bool)
    for o, cp in zip(out_off, caps):
        inside[int(o): int(o) + int(cp)] = True
    n = len(units)
    d_in = torch.from_numpy(blob.copy()).cuda()                            # exactly the batch's bytes
    assert d_in.numel() == len(blob) and d_in.data_ptr() % 16 == 0
    d_len = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    d_st = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    d_out = torch.full((total,), R.GUARD, dtype=torch.uint8, device="cuda")
    if path == "device-tables":
        plan = m.CompressDevPlan(gpu_ctx, R.LZNT1, n, int(lens.sum()) + 8 * 4096, int(lens.max()))
        tabs = [R._dt(a) for a in (in_off, lens, out_off, caps)]
    else:
        plan = m.Plan(gpu_ctx, R.LZNT1, in_off, lens, out_off, caps)
    try:
        with R.hooks(gpu_ctx, mode, 1 if path == "serial-atomics" else 0):
            if path == "device-tables":
                plan.execute(d_in, tabs[0], tabs[1], d_out, tabs[2], tabs[3], d_len, d_st)
            else:
                plan.execute(d_in, d_out, d_len, d_st)
            torch.cuda.synchronize()
    finally:
        plan.close()
    ln, st, out = d_len.cpu().numpy(), d_st.cpu().numpy(), d_out.cpu().numpy()
    assert (out[~inside] == R.GUARD).all(), np.nonzero(out[~inside] != R.GUARD)[0][:8]
    assert (d_in.cpu().numpy() == blob).all()
    for i, (u, exp) in enumerate(zip(units, want)):
        assert st[i] == 0, (mode, path, i, offs[i] % 16, len(u), st[i])
        got = bytes(out[int(out_off[i]): int(out_off[i]) + max(int(ln[i]), 0)])
        assert got == exp, "mode %d, %s, unit %d at src & 15 = %d, %d bytes: GPU bytes differ from the oracle (%d vs %d B)" % (
            mode, path, i, offs[i] % 16, len(u), len(got), len(exp))
