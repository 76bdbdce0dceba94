"""GPU: the branches of the parity kernels (csrc/parity.hip) that the one container of 25 rows in tests/test_gpu_parity_rows.py never
reaches, each with inputs made for it (tests/parity_rig.py) and an assertion BEFORE anything runs that the input reaches it:
  - every list of parities the damage pass can come to use -- [2], [0, 2] and [1, 2] make the matrices that are not plain Vandermonde --
    with lost members whose index needs the eighth bit of its byte in the record and wraps gf_exp's n %= 255, in groups of 255 and 254;
  - every position of the lost member within a batch of PA_DEPTH members;
  - the solve pass with more than one column tile per group (B = 16384 and 65536): lost rows that end in the last tile, short lost rows
    in a group of several tiles, plen on a tile seam and 16 bytes either side;
  - both running sums (par_off, and the fix view's offset table) past their first tile of 8192 entries, a capacity that cuts a row
    beyond it, groups and records from more than one workgroup, more items than the grid of the parity and the solve pass has workgroups;
  - every pair (start of a row mod 16, length mod 16).
As in tests/test_gpu_parity_rows.py every output is sentinel-filled with guards behind it and compared whole with tests/parity_model.py,
d_par and d_fix_packed as images over FILL, and FILL lies behind packed_len; beyond the model, every rebuilt row is compared with the
healthy container's stored bytes. The same inputs run through the model alone in tests/test_parity_model.py."""
import numpy as np
import pytest

import parity_model as Y
import parity_rig as G
from blocks_rig import Container, memo, rand, soft, text, FMTS, FILL
from parity_rig import FixOuts, check_build, check_rebuild, lose, rows_back, synthetic

pytestmark = pytest.mark.gpu
F = FMTS["xpress"]


@pytest.fixture(scope="module")
def made(gpu_ctx):
    yield from memo()


def parity(gpu_ctx, made, B, nbt, k, m):
    import ms_compress_amd as mm
    return made("parity", B, nbt, k, m, lambda: mm.BlockParity(gpu_ctx, B, nbt, k, m))


def built(gpu_ctx, made, name, con, k, m):
    """(parity object, healthy parity set at exact capacity, its length) of a container, made once"""
    pr = parity(gpu_ctx, made, con.B, con.nbt, k, m)

    def make():
        mo, pset = check_build(pr, con, slack=0, what=(name, k, m))
        assert mo["status"] == Y.OK and pset.room == int(mo["par_off"][-1])
        return pset, pset.room, mo
    return (pr,) + made("set", name, k, m, make)


# ---- which parities solve a group, at high member indices ----------------------------------------------------------------------------------
def subset_container(gpu_ctx, made):
    return made("subsets", lambda: synthetic(gpu_ctx, F, G.SUB_B, G.subset_table(), 51))


@pytest.mark.parametrize("m", [3, 2])
def test_every_parity_subset_at_high_member_indices(gpu_ctx, made, m):
    lens, cases = G.subset_table(), G.subset_cases(m)
    G.subset_conditions(lens, cases, m)
    h = subset_container(gpu_ctx, made)
    pr, pset, total, mb = built(gpu_ctx, made, "subsets", h, G.SUB_K, m)
    assert mb["head"] == [G.SUB_NB, 2, G.SUB_K, m]
    outs, seen = FixOuts(h.dev, h.nbt, 8 * G.SUB_B), set()
    for usable, lost0, lost1 in cases:
        rows = G.subset_rows(lost0, lost1)
        con, ver = lose(h, rows)
        mo, _ = check_rebuild(pr, con, ver, pset.damaged(par=G.spoil(mb["par_off"], m, 0, usable)), total, outs=outs, what=(m, usable, lost0, lost1))
        want = {0: list(usable[: len(lost0)])}
        if lost1:
            want[1] = list(range(len(lost1)))
        assert mo["status"] == Y.OK and mo["used"] == want and mo["rebuilt"] == sorted(rows) and mo["count"][4] == m - len(usable)
        rows_back(h, outs, mo, rows)
        seen.add(tuple(mo["used"][0]))
    assert seen == (set(G.SUBSETS) if m == 3 else {(0,), (1,), (0, 1)})


def test_one_lost_member_too_many_for_each_subset_size(gpu_ctx, made):
    h = subset_container(gpu_ctx, made)
    pr, pset, total, mb = built(gpu_ctx, made, "subsets", h, G.SUB_K, 3)
    outs = FixOuts(h.dev, h.nbt, 8 * G.SUB_B)
    for usable, lost0, lost1 in G.subset_overflows():
        assert len(lost0) == len(usable) + 1
        con, ver = lose(h, G.subset_rows(lost0, lost1))
        mo, _ = check_rebuild(pr, con, ver, pset.damaged(par=G.spoil(mb["par_off"], 3, 0, usable)), total, outs=outs, what=("too many", usable))
        back = [2 * i + 1 for i in lost1]
        assert mo["status"] == Y.DATA and mo["unrecoverable"] == [0] and mo["rebuilt"] == back and mo["used"] == {1: [0]}
        assert mo["count"][:4] == [len(lost0) + len(lost1), len(lost1), 2, 1]
        rows_back(h, outs, mo, back)


# ---- every member position of small groups -------------------------------------------------------------------------------------------------
def test_every_member_position_of_small_groups(gpu_ctx, made):
    """k = nb = 1 .. 9 at m = 1: the lost member at every place of a batch of PA_DEPTH = 4, in a first batch of 1 .. 4 members"""
    for nb in range(1, 10):
        h = synthetic(gpu_ctx, F, G.SUB_B, G.SMALL_LENS[:nb], 60 + nb)
        pr, pset, total, mb = built(gpu_ctx, made, ("small", nb), h, nb, 1)
        assert mb["head"] == [nb, 1, nb, 1]
        outs = FixOuts(h.dev, h.nbt, h.plen + 64)
        for j in range(nb):
            con, ver = lose(h, [j])
            mo, _ = check_rebuild(pr, con, ver, pset, total, outs=outs, what=("small", nb, j))
            assert mo["status"] == Y.OK and mo["rebuilt"] == [j] and mo["used"] == {0: [0]}
            rows_back(h, outs, mo, [j])


# ---- rebuild across column tiles -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [16384, 65536])
def test_rebuild_of_a_real_container_across_column_tiles(gpu_ctx, made, B):
    """six rows, raw ones among them, B / 4096 column tiles per group: the rows by length, lost alone, by twos and by threes"""
    h = made("real", B, lambda: Container.make(gpu_ctx, F, B, [rand(11, B + 77), soft(12, 2 * B + 1000), text(13, B - 3)]))
    h.d_packed[h.plen:] = FILL
    L = [int(x) for x in G.stored_lens(h.model(False))]
    by_len = sorted(range(6), key=lambda j: L[j])
    assert len(L) == 6 and L[by_len[-1]] == B and len(set(L)) >= 4
    for k, m in ((6, 3), (4, 2)):
        Gn = (6 + k - 1) // k
        same = lambda j: [i for i in by_len if i % Gn == j % Gn and i != j]     # the other members of j's group, by length
        losses = [[by_len[-1]], [by_len[0]], [by_len[-1], same(by_len[-1])[0]], [by_len[0], by_len[-1]]] + ([[by_len[-1], by_len[0], by_len[2]]] if m == 3 else [])
        met = set().union(*(G.tile_situations(B, L, k, m, lost) for lost in losses))
        assert B > 4096 and "a lost row that ends in the last tile, beyond tile 0" in met and "2 lost rows of different lengths" in met, met
        pr, pset, total, _ = built(gpu_ctx, made, ("real", B), h, k, m)
        outs = FixOuts(h.dev, h.nbt, h.plen + 64)
        for lost in losses:
            con, ver = lose(h, lost)
            mo, _ = check_rebuild(pr, con, ver, pset, total, outs=outs, what=("real", B, k, m, lost))
            assert mo["status"] == Y.OK and mo["rebuilt"] == sorted(lost)
            rows_back(h, outs, mo, lost)


@pytest.mark.parametrize("t", [1, 2, 3])
def test_rebuild_with_plen_on_a_tile_seam(gpu_ctx, made, t):
    tables = G.tile_tables()
    G.tile_conditions(tables)
    for plen, lens in tables:
        if (plen + 16) // 4096 != t:
            continue
        h = synthetic(gpu_ctx, F, G.TILE_B, lens, plen)
        outs = FixOuts(h.dev, h.nbt, h.plen + 64)
        for (k, m), losses in G.TILE_LOSSES.items():
            pr = parity(gpu_ctx, made, G.TILE_B, 6, k, m)
            mb, pset = check_build(pr, h, slack=0, what=("seam", plen, k, m))
            assert mb["status"] == Y.OK and mb["par_off"][1] == plen
            for lost in losses:
                con, ver = lose(h, lost)
                mo, _ = check_rebuild(pr, con, ver, pset, pset.room, outs=outs, what=("seam", plen, k, m, lost))
                assert mo["status"] == Y.OK and mo["rebuilt"] == sorted(lost)
                rows_back(h, outs, mo, lost)


# ---- tables past one scan tile -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,m", list(G.BIG_SHAPES))
def test_tables_past_one_scan_tile(gpu_ctx, made, k, m):
    import torch
    lens = G.big_table()
    rows, X, spoil_n = G.big_losses(k, m)
    listed = G.big_conditions(k, m, rows, X)
    grid = 2 * 4 * torch.cuda.get_device_properties(gpu_ctx.device).multi_processor_count   # what the parity and the solve pass launch at most
    Gn = (G.BIG_NB + k - 1) // k
    if (k, m) == (2, 3):
        assert Gn > grid and listed > grid, "neither pass goes round its grid loop"
    h = made("big", lambda: synthetic(gpu_ctx, F, G.BIG_B, lens, 71, nbt=G.BIG_NBT))
    pr, pset, total, mb = built(gpu_ctx, made, "big", h, k, m)
    Q = Y.geometry(G.BIG_NBT, k, m)[1]
    assert len(mb["par_off"]) == Q + 1 and mb["head"] == [G.BIG_NB, Gn, k, m]
    if Q > G.SCAN_TILE:                                           # a capacity that cuts a parity row beyond the running sum's first tile
        q = next(q for q in range(G.SCAN_TILE + 808, Q) if mb["par_off"][q + 1] > mb["par_off"][q])
        cut, _ = check_build(pr, h, pset=G.ParitySet(h.dev, h.nbt, k, m, total), par_cap=mb["par_off"][q + 1] - 16, what=("big, cut", k, m))
        assert cut["status"] == Y.BUF and cut["par_off"] == mb["par_off"] and cut["pieces"] == mb["pieces"][:q], "the rows before the cut are still written"
        assert cut["par_crc"][:q] == mb["par_crc"][:q] and not any(cut["par_crc"][q:])
    con, ver = lose(h, rows)
    bad = pset.damaged(par=G.spoil(mb["par_off"], m, X, range(m - spoil_n)))
    mo, outs = check_rebuild(pr, con, ver, bad, total, slack=0, what=("big", k, m))
    back = [j for j in rows if j % Gn != X]
    assert mo["status"] == Y.DATA and mo["unrecoverable"] == [X] and mo["rebuilt"] == back and len(mo["used"]) == listed
    assert mo["count"][2:5] == [listed + 1, 1, spoil_n] and outs.room == mo["fix_off"][-1] == sum(int(lens[j]) for j in back)
    rows_back(h, outs, mo, back)
    j = next(j for j in back if j > G.SCAN_TILE + 808 and lens[j])   # fix_cap cuts a rebuilt row beyond the running sum's first tile
    cut, _ = check_rebuild(pr, con, ver, bad, total, outs=outs, fix_cap=mo["fix_off"][j + 1] - 1, what=("big, fix_cap", k, m))
    assert cut["status"] == Y.BUF and cut["fix_off"] == mo["fix_off"] and cut["count"] == mo["count"]
    assert [i for i in back if cut["fix_verdict"][i] == Y.GOOD] == [i for i in back if i < j]
    rows_back(h, outs, cut, [i for i in back if i < j])


# ---- alignment matrix ----------------------------------------------------------------------------------------------------------------------
def test_every_start_and_length_residue(gpu_ctx, made):
    lens, start = G.align_table()
    rows = G.align_losses(lens, start)
    h = synthetic(gpu_ctx, F, G.ALIGN_B, lens, 81)
    assert np.array_equal(np.asarray(h.off[: G.ALIGN_NB], dtype=np.int64) % 16, start)
    k, m = G.ALIGN_SHAPE
    pr, pset, total, mb = built(gpu_ctx, made, "align", h, k, m)
    con, ver = lose(h, rows)
    mo, outs = check_rebuild(pr, con, ver, pset, total, slack=0, what="align")
    assert mo["status"] == Y.OK and mo["rebuilt"] == rows and mo["count"][:4] == [24, 24, 16, 0]
    rows_back(h, outs, mo, rows)
