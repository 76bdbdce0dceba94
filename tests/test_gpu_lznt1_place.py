"""The placement of the LZNT1 chunk images (csrc/util.hip concat_slots_kernel): a grid that is fixed by the device walks the batch in tiles of
64 consecutive chunks, block b taking the tiles b, b + grid, ...; a wave reads a tile's 64 offsets and sizes at once, finds the unit of its
first chunk by one search, reads a unit's row again only where a chunk reaches the next unit, and moves one image at a time: bytes up to the
destination's next 16-byte boundary, 16-byte stores, bytes behind them. What can go wrong there is an image's length and the alignment of its
place (head and tail without a body, every residue of the destination), what a tile holds (raw images beside images of a few bytes, a tile
that begins inside a unit), the seams of units inside a tile (three and more units in one tile, a unit over two tiles), the chunk count (a
partial tile, exactly one tile, one chunk more), a block's second tile (mscomp_amd_debug_set_place_blocks caps the grid: without the cap it
takes over 130 000 chunks to run) and a unit that does not fit its capacity, which gets MSCOMP_BUF_ERROR and no byte while its neighbours get
theirs. Every case runs through a host-table plan and a device-table plan (whose bound lies eight chunks above the batch), both chunk kernels
and grids of 1, 3 and the device's blocks, byte for byte against the oracle, with guard bytes around every capacity."""
import contextlib
import functools

import numpy as np
import pytest

import lznt1_model as M
import lznt1_run as R

PLANS = ("host-tables", "device-tables")
TILE = 64
BUF_ERROR = -5
EVERY = [pytest.mark.gpu, pytest.mark.parametrize("path", PLANS), pytest.mark.parametrize("mode", [1, 2]), pytest.mark.parametrize("blocks", [1, 3, 0])]


def every(f):
    for mark in EVERY:
        f = mark(f)
    return f


@contextlib.contextmanager
def grid_cap(gpu_ctx, blocks):
    try:
        gpu_ctx.lib.mscomp_amd_debug_set_place_blocks(blocks)
        yield
    finally:
        gpu_ctx.lib.mscomp_amd_debug_set_place_blocks(0)


# ---- the units ---------------------------------------------------------------------------------------------------------------
def _chunk(seed, j, n=M.CHUNK):
    """chunk j of a unit: noise in front, zeros behind, the share of the noise from 0 to the whole chunk: images of a few bytes up to raw ones"""
    k = (seed * 131 + j * 977) % (M.CHUNK + 1)
    c = np.zeros(n, np.uint8)
    c[:min(k, n)] = np.frombuffer(bytes(M.noise(seed * 100003 + j, M.CHUNK)), np.uint8)[:min(k, n)]
    return c


@functools.lru_cache(maxsize=None)
def _unit(chunks, seed, last=M.CHUNK):
    """a unit of `chunks` chunks, the last one of `last` bytes"""
    return b"".join(_chunk(seed, j, last if j + 1 == chunks else M.CHUNK).tobytes() for j in range(chunks))


@functools.lru_cache(maxsize=None)
def _batch(total):
    """`total` chunks in units of at most 30 chunks; the last chunk of the batch has 1000 bytes"""
    units, left = [], total
    while left:
        k = min(left, 30)
        left -= k
        units.append(_unit(k, 40 + len(units), 1000 if left == 0 else M.CHUNK))
    return tuple(units)


@functools.lru_cache(maxsize=None)
def _alternating():
    """one unit of 70 chunks, noise (a raw image of 4 098 bytes) and zeros (a few bytes) by turns"""
    return b"".join(bytes(M.noise(900 + j)) if j % 2 == 0 else bytes(M.CHUNK) for j in range(70))


SEAMS = (1, 2, 20, 40, 1, 63, 64, 65)


@functools.lru_cache(maxsize=None)
def _seams():
    return tuple(_unit(k, 70 + i) for i, k in enumerate(SEAMS))


def _chunks_of(u):
    return (len(u) + M.CHUNK - 1) // M.CHUNK


def _tiles_of_units(units):
    """per unit the first and the last tile it has chunks in"""
    out, c = [], 0
    for u in units:
        k = _chunks_of(u)
        out.append((c // TILE, (c + k - 1) // TILE))
        c += k
    return out


# ---- CPU: the batches are what the cases claim -----------------------------------------------------------------------------
def test_the_alternating_unit_holds_both_extremes(oracle):
    u = _alternating()
    sizes = [len(s) for s in M.chunk_streams(R.expected(oracle, u))]
    assert len(sizes) == 70 and all(s == M.CHUNK + 2 for s in sizes[0::2]) and all(s < 32 for s in sizes[1::2])


def test_the_seam_batch_has_crowded_tiles_and_a_unit_over_two_tiles():
    t = _tiles_of_units(_seams())
    per_tile = {}
    for a, b in t:
        for x in range(a, b + 1):
            per_tile[x] = per_tile.get(x, 0) + 1
    assert max(per_tile.values()) >= 3 and any(a != b for a, b in t)
    assert [_chunks_of(u) for u in _seams()] == list(SEAMS)


def test_the_mixed_chunks_give_images_of_many_lengths(oracle):
    sizes = [len(s) for u in _seams() for s in M.chunk_streams(R.expected(oracle, u))]
    assert min(sizes) < 40 and max(sizes) == M.CHUNK + 2 and len({s % 16 for s in sizes}) == 16


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _run(gpu_ctx, units, mode, path, out_off, caps):
    """lznt1_run.run_plan with the outputs laid out by the caller: (lengths, statuses, output bytes); inputs at odd offsets"""
    import torch
    import ms_compress_amd as m
    in_off, pos = [], 1
    for u in units:
        in_off.append(pos)
        pos += len(u)
        pos += 1 if pos % 2 == 0 else 2
    blob = np.zeros(pos + 32, np.uint8)
    for u, o in zip(units, in_off):
        blob[o: o + len(u)] = np.frombuffer(u, np.uint8)
    total = int(max(o + c for o, c in zip(out_off, caps))) + 16
    in_off, lens, out_off, caps = (np.array(a, np.uint64) for a in (in_off, [len(u) for u in units], out_off, caps))
    n = len(units)
    d_in = torch.from_numpy(blob).cuda()
    d_len = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    d_st = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    d_out = torch.full((total,), R.GUARD, dtype=torch.uint8, device="cuda")
    if path == "device-tables":
        plan = m.CompressDevPlan(gpu_ctx, R.LZNT1, n, int(lens.sum()) + 8 * 4096, int(lens.max()))
        tabs = [R._dt(a) for a in (in_off, lens, out_off, caps)]
    else:
        plan = m.Plan(gpu_ctx, R.LZNT1, in_off, lens, out_off, caps)
    try:
        with R.hooks(gpu_ctx, mode, 0):
            if path == "device-tables":
                plan.execute(d_in, tabs[0], tabs[1], d_out, tabs[2], tabs[3], d_len, d_st)
            else:
                plan.execute(d_in, d_out, d_len, d_st)
            torch.cuda.synchronize()
    finally:
        plan.close()
    out = d_out.cpu().numpy()
    inside = np.zeros(total, bool)
    for o, cp in zip(out_off, caps):
        inside[int(o): int(o) + int(cp)] = True
    assert (out[~inside] == R.GUARD).all(), (mode, path, np.nonzero(out[~inside] != R.GUARD)[0][:8])
    return d_len.cpu().numpy(), d_st.cpu().numpy(), out


@every
def test_images_without_a_body(oracle, gpu_ctx, mode, path, blocks):
    """one-chunk units of 1, 2 and 3 bytes: images of 3 to 5 bytes, a head or a tail and nothing between"""
    units = [bytes(M.noise(7, n)) for n in (1, 2, 3)]
    assert [len(R.expected(oracle, u)) for u in units] == [3, 4, 5]
    with grid_cap(gpu_ctx, blocks):
        R.check_plan(oracle, gpu_ctx, units, mode, path, "images of 3 to 5 bytes")


@every
def test_every_residue_of_the_destination(oracle, gpu_ctx, mode, path, blocks):
    """one-chunk units whose out_off takes every residue modulo 16, once with an image of about a hundred bytes and once with a raw image of 4 098"""
    import ms_compress_amd as m
    units = [bytes(M.noise(300 + i, 100 + 7 * i)) for i in range(16)] + [bytes(M.noise(400 + i)) for i in range(16)]
    caps = [m.max_compressed_size(R.LZNT1, len(u)) + 2 for u in units]
    out_off, pos = [], 16
    for i, cp in enumerate(caps):
        pos += 16 + (i % 16 - (pos + 16)) % 16
        out_off.append(pos)
        pos += cp
    assert [o % 16 for o in out_off] == list(range(16)) * 2 and all(b - (a + c) >= 16 for a, b, c in zip(out_off, out_off[1:], caps))
    with grid_cap(gpu_ctx, blocks):
        ln, st, out = _run(gpu_ctx, units, mode, path, out_off, caps)
    for i, u in enumerate(units):
        exp = R.expected(oracle, u)
        assert st[i] == 0 and bytes(out[out_off[i]: out_off[i] + max(int(ln[i]), 0)]) == exp, (i, out_off[i] % 16, len(u), st[i], ln[i], len(exp))


@every
def test_a_tile_of_raw_and_tiny_images(oracle, gpu_ctx, mode, path, blocks):
    with grid_cap(gpu_ctx, blocks):
        R.check_plan(oracle, gpu_ctx, [_alternating()], mode, path, "70 chunks, noise and zeros by turns")


@every
def test_unit_seams_inside_a_tile(oracle, gpu_ctx, mode, path, blocks):
    with grid_cap(gpu_ctx, blocks):
        R.check_plan(oracle, gpu_ctx, list(_seams()), mode, path, "units of %s chunks" % (SEAMS,))


@every
@pytest.mark.parametrize("total", [1, 63, 64, 65, 200])
def test_chunk_counts(oracle, gpu_ctx, total, mode, path, blocks):
    units = list(_batch(total))
    assert sum(_chunks_of(u) for u in units) == total
    with grid_cap(gpu_ctx, blocks):
        R.check_plan(oracle, gpu_ctx, units, mode, path, "%d chunks" % total)


@every
@pytest.mark.parametrize("front", [64, 5])
def test_a_unit_that_does_not_fit(oracle, gpu_ctx, front, mode, path, blocks):
    """the middle unit's capacity is one byte short: MSCOMP_BUF_ERROR, nothing written to it, its neighbours exact. Its first chunk is the first
    of a tile (64 chunks in front) or lies in mid-tile (5 in front)."""
    import ms_compress_amd as m
    units = [_unit(front, 11), _unit(3, 12), _unit(2, 13, 700)]
    want = [R.expected(oracle, u) for u in units]
    caps = [m.max_compressed_size(R.LZNT1, len(u)) + 2 for u in units]
    caps[1] = len(want[1]) - 1
    out_off, pos = [], 16
    for cp in caps:
        out_off.append(pos)
        pos += cp + 16
    with grid_cap(gpu_ctx, blocks):
        ln, st, out = _run(gpu_ctx, units, mode, path, out_off, caps)
    assert st[1] == BUF_ERROR == m.MSCOMP_BUF_ERROR and ln[1] == 0, (st, ln)
    assert (out[out_off[1] - 16: out_off[1] + caps[1] + 16] == R.GUARD).all()          # its guard bytes, and no byte of its own
    for i in (0, 2):
        assert st[i] == 0 and bytes(out[out_off[i]: out_off[i] + int(ln[i])]) == want[i], (i, st[i], ln[i], len(want[i]))


@every
def test_suffix_array_flavour(oracle, gpu_ctx, mode, path, blocks):
    """the other dictionary's chunk kernel hands its images to the same launcher"""
    lib = gpu_ctx.lib
    u = _alternating()
    es, exp = oracle.oracle_compress_sa(u)
    assert es == 0 and lib.mscomp_amd_get_lznt1_sa_dict() == 0
    lib.mscomp_amd_set_lznt1_sa_dict(1)
    try:
        with grid_cap(gpu_ctx, blocks):
            res, out_off, _ = R.run_plan(gpu_ctx, [u], mode, path)
    finally:
        lib.mscomp_amd_set_lznt1_sa_dict(0)
    ln, st, out = res[0]
    assert st[0] == 0 and bytes(out[int(out_off[0]): int(out_off[0]) + max(int(ln[0]), 0)]) == exp
