"""CPU: the parity model (tests/parity_model.py), which the GPU tests compare mscomp_amd_parity_build and _rebuild with array for array.
The field and the code are pinned here -- the packed "times alpha" of the kernels against the table product, Horner against the defining
sum -- and so is the reason for the cap of three parity rows: every erasure pattern of up to three rows is solvable with ANY parities of
{0, 1, 2}, exhaustively at k = 255, and a fourth parity alpha^(3 i) is not. Then round trips on small containers of tests/blocks_model.py, and the synthetic tables of
tests/test_gpu_parity_edges.py (tests/parity_rig.py) with the assertions that they reach the branches they are named for."""
import itertools

import numpy as np
import pytest

import extents_model as X
import parity_model as Y
import parity_rig as G
import read_model as R
import repair_model as P

B = 4096
FMT = 3


@pytest.fixture(scope="module")
def api():
    import ms_compress_amd                                       # noqa: F401  the model describes this library's calls: no library, no test
    from ms_compress_amd import api
    assert "mscomp_amd_parity_build" in api.EXPORTS and "mscomp_amd_parity_rebuild" in api.EXPORTS
    assert (api.MSCOMP_AMD_PARITY_K_MAX, api.MSCOMP_AMD_PARITY_M_MAX) == (Y.K_MAX, Y.M_MAX)
    return api


@pytest.fixture(scope="module")
def src(oracle):
    s = X.source(oracle, FMT, B, R.buffers(B))
    nb = int(s[2][-1])
    lens = np.diff(np.asarray(s[3][: nb + 1], dtype=np.int64))
    assert nb == 28 and (lens == B).sum() >= 5 and (lens < 64).sum() >= 5 and len(set((np.asarray(s[3][:nb]) % 16).tolist())) >= 8
    return s


def test_packed_times_alpha_is_the_table_product(api):
    for lane in range(4):
        for v in range(256):
            others = 0x00A55A3C & ~(0xFF << (8 * lane))
            got = Y.x2_packed(v << (8 * lane) | others)
            assert (got >> (8 * lane)) & 0xFF == int(Y.mul(2, v)), (lane, v)
            for o in range(4):                                     # and the other lanes are the products of their own bytes
                if o != lane:
                    assert (got >> (8 * o)) & 0xFF == int(Y.mul(2, (others >> (8 * o)) & 0xFF))
    assert int(Y.EXP[8]) == 0x1D and sorted(int(x) for x in Y.EXP[:255]) == list(range(1, 256))   # 0x11D, and alpha generates the field


def test_horner_is_the_defining_sum(api):
    rs = np.random.RandomState(5)
    for k in (1, 2, 7, 20):
        rows = [rs.randint(0, 256, 48).astype(np.uint8) for _ in range(k)]
        for m in (1, 2, 3):
            assert np.array_equal(Y.horner(rows, m), Y.defining(rows, m)), (k, m)


def _det2(x, y, p, q):
    """the determinant of [[x^p, y^p], [x^q, y^q]] for arrays of points"""
    pw = lambda v, e: Y.EXP[(Y.LOG[v] * e) % 255]
    return Y.mul(pw(x, p), pw(y, q)) ^ Y.mul(pw(x, q), pw(y, p))


def test_every_erasure_pattern_is_solvable_with_three_parities(api):
    """exhaustively at k = 255: every single row with every parity, every pair of rows with every pair of parities, every triple of rows"""
    pts = Y.EXP[:255]
    assert len(set(pts.tolist())) == 255 and (pts != 0).all()
    for p in range(3):
        assert (Y.EXP[(np.arange(255) * p) % 255] != 0).all()
    i, j = np.triu_indices(255, 1)
    for p, q in ((0, 1), (0, 2), (1, 2)):
        assert (_det2(pts[i], pts[j], p, q) != 0).all(), (p, q)
    t = np.array(list(itertools.combinations(range(255), 3)), dtype=np.int64)
    a, b, c = pts[t[:, 0]], pts[t[:, 1]], pts[t[:, 2]]
    sq = lambda v: Y.mul(v, v)
    # the 3 x 3 determinant of rows (1, 1, 1), (a, b, c), (a^2, b^2, c^2), expanded along the first row
    det = (Y.mul(b, sq(c)) ^ Y.mul(c, sq(b))) ^ (Y.mul(a, sq(c)) ^ Y.mul(c, sq(a))) ^ (Y.mul(a, sq(b)) ^ Y.mul(b, sq(a)))
    assert len(t) == 255 * 254 * 253 // 6 and (det != 0).all()


def test_a_fourth_parity_has_a_singular_pair(api):
    """the cap is a fact: with alpha^(3 i) beside alpha^0, two rows 85 apart have the same cube"""
    pts = Y.EXP[:255]
    i, j = np.triu_indices(255, 1)
    bad = np.nonzero(_det2(pts[i], pts[j], 0, 3) == 0)[0]
    assert bad.size > 0 and (int(i[bad[0]]), int(j[bad[0]])) == (0, 85)
    assert Y.invert([[1, 1], [Y.coef(3, 0), Y.coef(3, 85)]]) is None and Y.invert([[1, 1], [Y.coef(2, 0), Y.coef(2, 85)]]) is not None


def _erased(s, rows):
    """the source with a byte of each row flipped, and the verdicts that say so"""
    packed = bytearray(s[0])
    nbt = int(s[7])
    ver = [Y.GOOD] * int(s[2][-1]) + [Y.SKIPPED] * (nbt - int(s[2][-1]))
    for j in rows:
        if int(s[3][j + 1]) > int(s[3][j]):
            packed[int(s[3][j])] ^= 0xFF
        ver[j] = 3
    return (bytes(packed),) + tuple(s[1:]), ver


def _stored(s, j):
    return bytes(s[0][int(s[3][j]): int(s[3][j + 1])])


@pytest.mark.parametrize("k,m", [(1, 1), (3, 1), (4, 2), (5, 3), (255, 3)])
def test_every_erasure_pattern_of_a_group_comes_back(api, src, k, m):
    nb, nbt = int(src[2][-1]), int(src[7])
    mb = Y.model_build(src, B, k, m, 1 << 40)
    G = (nb + k - 1) // k
    assert mb["status"] == Y.OK and mb["head"] == [nb, G, k, m] and all(o % 16 == 0 for o in mb["par_off"])
    groups = range(G) if k < 255 else [0]
    for g in groups:
        members = list(range(g, nb, G))
        pats = [c for e in range(1, m + 1) for c in itertools.combinations(members, e)]
        if len(pats) > 40:
            pats = pats[:: len(pats) // 40]
        for rows in pats:
            dam, ver = _erased(src, rows)
            mo = Y.model_rebuild(dam, ver, mb["set"], B, k, m, 1 << 40)
            assert mo["status"] == Y.OK and mo["rebuilt"] == sorted(rows) and mo["count"][:4] == [len(rows), len(rows), 1, 0]
            fix = Y.fix_source(src, mo)
            for j in range(nbt):
                want = _stored(src, j) if j in rows else b""
                assert _stored(fix, j) == want and mo["fix_verdict"][j] == (Y.GOOD if j in rows else Y.SKIPPED)


def test_one_row_too_many_loses_its_group_alone(api, src):
    k, m = 4, 2
    nb = int(src[2][-1])
    G = (nb + k - 1) // k
    mb = Y.model_build(src, B, k, m, 1 << 40)
    gone = [2, 2 + G, 2 + 2 * G, 3, 4 + G]                       # three of group 2, one each of groups 3 and 4
    dam, ver = _erased(src, gone)
    mo = Y.model_rebuild(dam, ver, mb["set"], B, k, m, 1 << 40)
    assert mo["status"] == Y.DATA and mo["unrecoverable"] == [2] and mo["rebuilt"] == [3, 4 + G] and mo["count"] == [5, 2, 3, 1, 0, mo["count"][5]]
    fix = Y.fix_source(src, mo)
    assert _stored(fix, 3) == _stored(src, 3) and _stored(fix, 4 + G) == _stored(src, 4 + G) and _stored(fix, 2) == b""


def test_a_damaged_parity_row_shifts_the_choice(api, src):
    k, m = 4, 2
    nb = int(src[2][-1])
    G = (nb + k - 1) // k
    mb = Y.model_build(src, B, k, m, 1 << 40)
    pset = dict(mb["set"])
    par = bytearray(pset["par"])
    par[int(pset["par_off"][2 * m + 0]) + 3] ^= 0x10               # parity 0 of group 2
    pset["par"] = bytes(par)
    dam, ver = _erased(src, [2 + G])
    mo = Y.model_rebuild(dam, ver, pset, B, k, m, 1 << 40)
    assert mo["status"] == Y.OK and mo["used"] == {2: [1]} and mo["count"][4] == 1 and _stored(Y.fix_source(src, mo), 2 + G) == _stored(src, 2 + G)
    dam, ver = _erased(src, [2, 2 + G])
    mo = Y.model_rebuild(dam, ver, pset, B, k, m, 1 << 40)
    assert mo["status"] == Y.DATA and mo["unrecoverable"] == [2] and mo["rebuilt"] == []
    other = Y.model_build(src, B, 5, m, 1 << 40)["set"]
    assert Y.model_rebuild(src, ver, other, B, k, m, 1 << 40)["status"] == Y.DATA            # a header of another shape
    assert Y.model_rebuild(src, ver, mb["set"], B, k, m, 1 << 40, nbt=int(src[7]) + 1)["status"] == Y.ARG


def test_capacities(api, src):
    k, m = 4, 2
    full = Y.model_build(src, B, k, m, 1 << 40)
    total = full["par_off"][-1]
    short = Y.model_build(src, B, k, m, total - 16)
    assert Y.model_build(src, B, k, m, total)["status"] == Y.OK and short["status"] == Y.BUF and short["par_off"] == full["par_off"]
    assert short["pieces"] == full["pieces"][:-1] and short["par_crc"][: len(full["pieces"]) - 1] == full["par_crc"][: len(full["pieces"]) - 1]
    assert short["par_crc"][len(full["pieces"]) - 1] == 0
    dam, ver = _erased(src, [5, 9])
    mo = Y.model_rebuild(dam, ver, full["set"], B, k, m, 1 << 40)
    need = mo["fix_off"][-1]
    cut = Y.model_rebuild(dam, ver, full["set"], B, k, m, need - 1)
    assert cut["status"] == Y.BUF and cut["fix_off"] == mo["fix_off"] and cut["fix_verdict"][5] == Y.GOOD and cut["fix_verdict"][9] == Y.SKIPPED


def test_fix_view_and_repair_give_the_healthy_container(api, oracle, src):
    """the header's consequence over the models: salvage, rebuild, repair over {primary, fix view}, splice by extents"""
    k, m = 4, 2
    nb, n = int(src[2][-1]), int(src[6])
    mb = Y.model_build(src, B, k, m, 1 << 40)
    packed = bytearray(src[0])
    for j in (3, 6, 12, 25):                                      # raw and compressed rows of four groups
        packed[int(src[3][j]) + min(5, int(src[3][j + 1] - src[3][j]) - 1)] ^= 0xFF
    off = np.array(src[3], dtype=np.uint64)
    off[16] = off[15]                                             # an offset entry: rows 15 and 16, two groups
    dam = (bytes(packed), src[1], src[2], off) + tuple(src[4:])
    total = sum(src[4])
    ver = P.model_salvage(oracle, FMT, dam, B, total, src[4])["verdict"]
    assert sorted(int(j) for j in np.nonzero(ver[:nb] != Y.GOOD)[0]) == [3, 6, 12, 15, 16, 25]
    mo = Y.model_rebuild(dam, ver, mb["set"], B, k, m, 1 << 40)
    assert mo["status"] == Y.OK and mo["rebuilt"] == [3, 6, 12, 15, 16, 25]
    fix = Y.fix_source(dam, mo)
    ver_fix = P.model_salvage(oracle, FMT, fix, B, total, src[4], only=ver)["verdict"]
    assert [int(x) for x in ver_fix[:nb]] == [Y.GOOD if j in mo["rebuilt"] else Y.SKIPPED for j in range(nb)]
    for second in (ver_fix, mo["fix_verdict"]):
        mr = P.model_repair([dam, fix], [ver, second], B, n, nb)
        assert not any(mr["status"]) and mr["count"][:2] == [6, 0]
        P.holds_consequence([dam, fix], mr, B, src)


# ---- the inputs of tests/test_gpu_parity_edges.py (tests/parity_rig.py) through the model alone: build, erase, rebuild, rows back ----------
def _round_trip(s, mb, rows, k, m, Bs, pset=None, want_used=None, lost_group=None):
    """rebuild of ``rows`` lost from the synthetic source s; every row of a recoverable group comes back with its stored bytes"""
    dam, ver = G.lose_host(s, rows)
    mo = Y.model_rebuild(dam, ver, pset or mb["set"], Bs, k, m, 1 << 40)
    nb = int(s[2][-1])
    Gn = (nb + k - 1) // k
    back = [j for j in rows if j % Gn != lost_group]
    assert mo["rebuilt"] == sorted(back) and mo["unrecoverable"] == ([] if lost_group is None else [lost_group])
    assert mo["status"] == (Y.OK if lost_group is None else Y.DATA)
    fix = Y.fix_source(s, mo)
    for j in back:
        assert _stored(fix, j) == _stored(s, j), j
    if want_used is not None:
        assert mo["used"] == want_used, (mo["used"], want_used)
    return mo


def test_edges_every_parity_subset_at_high_member_indices(api):
    lens = G.subset_table()
    s = G.synthetic_host(G.SUB_B, lens, 51)
    for m in (3, 2):
        cases = G.subset_cases(m)
        G.subset_conditions(lens, cases, m)
        mb = Y.model_build(s, G.SUB_B, G.SUB_K, m, 1 << 40)
        assert mb["head"] == [G.SUB_NB, 2, G.SUB_K, m] and mb["par_off"][m] == m * 4096
        seen = set()
        for usable, lost0, lost1 in cases:
            pset = G.spoiled(mb["set"], G.spoil(mb["par_off"], m, 0, usable))
            used = {0: list(usable[: len(lost0)])}
            if lost1:
                used[1] = list(range(len(lost1)))
            mo = _round_trip(s, mb, G.subset_rows(lost0, lost1), G.SUB_K, m, G.SUB_B, pset, used)
            assert mo["count"][4] == m - len(usable)
            seen.add(tuple(mo["used"][0]))
        assert seen == (set(G.SUBSETS) if m == 3 else {(0,), (1,), (0, 1)})
    mb = Y.model_build(s, G.SUB_B, G.SUB_K, 3, 1 << 40)
    for usable, lost0, lost1 in G.subset_overflows():
        assert len(lost0) == len(usable) + 1
        _round_trip(s, mb, G.subset_rows(lost0, lost1), G.SUB_K, 3, G.SUB_B, G.spoiled(mb["set"], G.spoil(mb["par_off"], 3, 0, usable)), {1: [0]}, lost_group=0)


def test_edges_every_member_position_of_small_groups(api):
    for nb in range(1, 10):
        s = G.synthetic_host(B, G.SMALL_LENS[:nb], 60 + nb)
        mb = Y.model_build(s, B, nb, 1, 1 << 40)
        assert mb["head"] == [nb, 1, nb, 1]
        for j in range(nb):
            _round_trip(s, mb, [j], nb, 1, B, want_used={0: [0]})


def test_edges_rebuild_across_column_tiles(api):
    tables = G.tile_tables()
    G.tile_conditions(tables)
    for plen, lens in tables:
        s = G.synthetic_host(G.TILE_B, lens, plen)
        for (k, m), losses in G.TILE_LOSSES.items():
            mb = Y.model_build(s, G.TILE_B, k, m, 1 << 40)
            assert mb["par_off"][1] == plen
            for rows in losses:
                _round_trip(s, mb, rows, k, m, G.TILE_B)


@pytest.mark.parametrize("k,m", list(G.BIG_SHAPES))
def test_edges_tables_past_one_scan_tile(api, k, m):
    lens = G.big_table()
    s = G.synthetic_host(G.BIG_B, lens, 71, nbt=G.BIG_NBT)
    rows, X, spoil_n = G.big_losses(k, m)
    listed = G.big_conditions(k, m, rows, X)
    mb = Y.model_build(s, G.BIG_B, k, m, 1 << 40)
    assert len(mb["par_off"]) == Y.geometry(G.BIG_NBT, k, m)[1] + 1 and mb["row_len"][G.BIG_NB:] == [0] * 3
    pset = G.spoiled(mb["set"], G.spoil(mb["par_off"], m, X, range(m - spoil_n)))
    mo = _round_trip(s, mb, rows, k, m, G.BIG_B, pset, lost_group=X)
    assert len(mo["used"]) == listed and mo["count"][2:5] == [listed + 1, 1, spoil_n] and mo["fix_off"][-1] == sum(int(lens[j]) for j in mo["rebuilt"])


def test_edges_alignment_matrix(api):
    lens, start = G.align_table()
    s = G.synthetic_host(G.ALIGN_B, lens, 81)
    assert np.array_equal(np.asarray(s[3][: G.ALIGN_NB], dtype=np.int64) % 16, start)
    k, m = G.ALIGN_SHAPE
    mb = Y.model_build(s, G.ALIGN_B, k, m, 1 << 40)
    _round_trip(s, mb, G.align_losses(lens, start), k, m, G.ALIGN_B)
