"""What the GPU tests of the parity object (tests/test_gpu_parity_rows.py, tests/test_gpu_parity_edges.py) add to tests/blocks_rig.py and
tests/repair_rig.py: one build and one rebuild with sentinel-filled, guarded outputs compared with tests/parity_model.py array for array
and image for image; synthetic tables of stored rows (parity reads stored bytes only: no encoder, no oracle) with the rows to lose; and
the inputs of the edge tests, each with the assertions that it reaches the branch it is named for -- host code, which
tests/test_parity_model.py runs through the model alone. torch is imported inside the functions that need it. Not collected as a test."""
import numpy as np

import parity_model as Y
from blocks_rig import Container, d64, i32, rand, same_image, CAP_GUARD, ENTRY_GUARD, FILL, SENT, SENT32, ST_FILL

FILL32 = FILL * 0x01010101


def _full(dev, n, v, t):
    import torch
    return torch.full((n + ENTRY_GUARD,), v, dtype=t, device=dev)


def _u64(t):
    return [int(x) for x in t.cpu().numpy().view(np.uint64)]


def _u32(t):
    return [int(x) for x in t.cpu().numpy().view(np.uint32)]


def _whole(got, want, guard, what):
    """an output array against the model's: its entries and nothing but sentinels behind them, or all sentinels where the call writes nothing"""
    want = [] if want is None else [int(x) for x in want]
    assert got == want + [guard] * (len(got) - len(want)), (what, got, want)


class ParitySet:
    """the outputs of a build for a table of nbt rows: d_par of ``room`` bytes of FILL with CAP_GUARD more behind them, and the five arrays"""

    def __init__(self, dev, nbt, k, m, room):
        import torch
        self.dev, self.nbt, self.k, self.m, self.room = dev, nbt, k, m, room
        self.Q = Y.geometry(nbt, k, m)[1]
        self.d_par = torch.full((room + CAP_GUARD,), FILL, dtype=torch.uint8, device=dev)
        self.d_off, self.d_head = _full(dev, self.Q + 1, SENT, torch.int64), _full(dev, 4, SENT, torch.int64)
        self.d_crc, self.d_rl, self.d_st = _full(dev, self.Q, SENT32, torch.int32), _full(dev, nbt, SENT32, torch.int32), _full(dev, 1, ST_FILL, torch.int32)

    def reset(self):
        self.d_par.fill_(FILL); self.d_off.fill_(SENT); self.d_head.fill_(SENT); self.d_crc.fill_(SENT32); self.d_rl.fill_(SENT32); self.d_st.fill_(ST_FILL)

    def build(self, pr, view, par_cap=None):
        pr.build(view, self.d_par, self.d_off, self.d_crc, self.d_rl, self.d_head, self.d_st, par_cap=self.room if par_cap is None else par_cap)

    def against(self, mo, what):
        _whole(_u64(self.d_off), mo["par_off"], SENT, (what, "par_off"))
        _whole(_u32(self.d_crc), mo["par_crc"], SENT32, (what, "par_crc"))
        _whole(_u32(self.d_rl), mo["row_len"], SENT32, (what, "row_len"))
        _whole(_u64(self.d_head), mo["head"], SENT, (what, "par_head"))
        _whole([int(x) for x in self.d_st.cpu().numpy()], [mo["status"]], ST_FILL, (what, "status"))
        same_image(self.d_par.cpu().numpy(), mo["pieces"], FILL, (what, "d_par"))

    def damaged(self, par=(), crc=()):
        """a copy whose parity bytes at ``par`` and CRC words at ``crc`` are flipped, with the host set that says the same"""
        import copy
        c = copy.copy(self)
        c.d_par, c.d_crc = self.d_par.clone(), self.d_crc.clone()
        for at in par:
            c.d_par[at] ^= 0x40
        for q in crc:
            c.d_crc[q] ^= 0x1001
        return c

    def host(self, par_len):
        """the set as the model reads it"""
        return {"par": bytes(self.d_par.cpu().numpy()[:par_len]), "par_off": np.array(_u64(self.d_off)[: self.Q + 1], dtype=np.uint64),
                "par_crc": np.array(_u32(self.d_crc)[: self.Q], dtype=np.uint32), "row_len": np.array(_u32(self.d_rl)[: self.nbt], dtype=np.uint32),
                "head": np.array(_u64(self.d_head)[:4], dtype=np.uint64)}


def check_build(pr, con, pset=None, par_cap=None, nbt=None, what="build", slack=None):
    """one BlockParity.build over the Container ``con`` compared with the model; returns (model, ParitySet). The set made here has the
    room of bound(), or with ``slack`` that of the model's total + slack: a large table does not allocate and compare Q B bytes."""
    build = lambda cap: Y.model_build(con.model(False, nbt=nbt), con.B, pr.k, pr.m, cap, nbt=pr.n_blocks_table)
    mo = None
    if pset is None:
        if slack is not None:
            mo = build(1 << 62)                                   # (everything fits: what any capacity from the total up gives)
        room = pr.bound()[1] if slack is None else (int(mo["par_off"][-1]) if mo["par_off"] else 0) + slack
        pset = ParitySet(con.dev, pr.n_blocks_table, pr.k, pr.m, room)
    pset.reset()
    pset.build(pr, con.view(False, nbt=nbt), par_cap)
    con.ctx.stream.synchronize()
    if mo is None or par_cap is not None:
        mo = build(pset.room if par_cap is None else par_cap)
    pset.against(mo, what)
    return mo, pset


class FixOuts:
    """the outputs of a rebuild: d_fix of ``room`` bytes of FILL with CAP_GUARD more behind them, and the four arrays"""

    def __init__(self, dev, nbt, room):
        import torch
        self.dev, self.nbt, self.room = dev, nbt, room
        self.d_fix = torch.full((room + CAP_GUARD,), FILL, dtype=torch.uint8, device=dev)
        self.d_off, self.d_count = _full(dev, nbt + 1, SENT, torch.int64), _full(dev, 6, SENT, torch.int64)
        self.d_ver, self.d_st = _full(dev, nbt, SENT32, torch.int32), _full(dev, 1, ST_FILL, torch.int32)

    def reset(self):
        self.d_fix.fill_(FILL); self.d_off.fill_(SENT); self.d_count.fill_(SENT); self.d_ver.fill_(SENT32); self.d_st.fill_(ST_FILL)

    def rebuild(self, pr, view, d_verdict, pset, par_len, fix_cap=None):
        pr.rebuild(view, d_verdict, pset.d_par, pset.d_off, pset.d_crc, pset.d_rl, pset.d_head, self.d_fix, self.d_off, self.d_ver, self.d_count, self.d_st,
                   par_len=par_len, fix_cap=self.room if fix_cap is None else fix_cap)

    def against(self, mo, what):
        _whole(_u64(self.d_off), mo["fix_off"], SENT, (what, "fix_off"))
        _whole(_u32(self.d_ver), mo["fix_verdict"], SENT32, (what, "fix_verdict"))
        _whole(_u64(self.d_count), mo["count"], SENT, (what, "count"))
        _whole([int(x) for x in self.d_st.cpu().numpy()], [mo["status"]], ST_FILL, (what, "status"))
        same_image(self.d_fix.cpu().numpy(), mo["pieces"], FILL, (what, "d_fix"))


def check_rebuild(pr, con, verdict, pset, par_len, outs=None, fix_cap=None, nbt=None, d_verdict=None, what="rebuild", slack=None):
    """one BlockParity.rebuild over the (damaged) Container ``con``, its verdicts and the ParitySet compared with the model; returns
    (model, FixOuts). The outputs made here have room for every stored byte, or with ``slack`` for the model's total + slack."""
    rebuild = lambda cap: Y.model_rebuild(con.model(False, nbt=nbt), verdict, pset.host(par_len), con.B, pr.k, pr.m, cap, nbt=pr.n_blocks_table, par_len=par_len)
    mo = None
    if outs is None:
        if slack is not None:
            mo = rebuild(1 << 62)
        outs = FixOuts(con.dev, pr.n_blocks_table, con.plen + 64 if slack is None else (int(mo["fix_off"][-1]) if mo["fix_off"] else 0) + slack)
    outs.reset()
    d_verdict = i32(np.asarray(verdict, dtype=np.uint32), con.dev) if d_verdict is None else d_verdict
    outs.rebuild(pr, con.view(False, nbt=nbt), d_verdict, pset, par_len, fix_cap)
    con.ctx.stream.synchronize()
    if mo is None or fix_cap is not None:
        mo = rebuild(outs.room if fix_cap is None else fix_cap)
    outs.against(mo, what)
    return mo, outs


def rows_back(h, outs, mo, rows):
    """beyond the model: every row of ``rows`` lies in d_fix, at the offsets the call wrote, with the healthy container's stored bytes"""
    got, off = outs.d_fix.cpu().numpy(), _u64(outs.d_off)
    for j in rows:
        want = h.packed[int(h.off[j]): int(h.off[j + 1])]
        assert mo["fix_verdict"][j] == Y.GOOD and off[j + 1] - off[j] == len(want) and bytes(got[off[j]: off[j + 1]]) == want, ("row", j)


def fix_container(con, outs, mo):
    """the sparse mirror as a Container beside ``con``: the fix's stored bytes and offsets, the primary's first, lens and crc"""
    c = con.edited(off=np.array(mo["fix_off"], dtype=np.uint64))
    c.d_packed, c.d_boff = outs.d_fix, outs.d_off
    c.plen = c.cap = int(mo["fix_off"][-1])
    image = bytearray(c.plen)
    for at, b in mo["pieces"]:
        image[at: at + len(b)] = b
    c.packed = bytes(image)
    return c


# ---- synthetic tables: stored rows of any length at any residue, and rows lost from them ------------------------------------------------
CRC_VERDICT = 3                                                 # repair_model.CRC: what salvage says of a row whose checksum fails


def synthetic_host(B, lens, seed, nbt=None, lead=3):
    """a source as the models take one: random stored bytes, ONE resource of len(lens) rows with these stored lengths, the first at
    offset ``lead`` and each behind the last, the table padded to ``nbt`` rows (the entries behind the last row repeat its end)"""
    nb = len(lens)
    nbt = nb if nbt is None else nbt
    assert nbt >= nb and (not nb or 0 <= min(lens) and max(lens) <= B)
    off = np.zeros(nbt + 1, dtype=np.uint64)
    off[: nb + 1] = lead + np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))])
    off[nb + 1:] = off[nb]
    packed = rand(seed, int(off[nb]))
    return (packed, len(packed), np.array([0, nb], dtype=np.uint64), off, [nb * B], None, 1, nbt)


def synthetic(ctx, fmt, B, lens, seed, nbt=None, lead=3):
    """synthetic_host as a Container on the device, FILL behind packed_len; no encoder and no oracle: parity reads stored bytes only"""
    packed, _, first, off, res, _, _, nbt = synthetic_host(B, lens, seed, nbt, lead)
    con = Container.from_host(ctx, fmt, B, packed, first, off, res, np.zeros(nbt, dtype=np.uint32))
    con.d_packed[con.plen:] = FILL
    return con


def lose_host(src, rows):
    """(the source with one byte flipped in every row of ``rows`` that has bytes, the verdicts: CRC for every row named -- a row of no
    bytes too --, GOOD for the others, SKIPPED behind the last row)"""
    packed, nb, nbt = bytearray(src[0]), int(src[2][-1]), int(src[7])
    ver = np.array([Y.GOOD] * nb + [Y.SKIPPED] * (nbt - nb), dtype=np.uint32)
    for j in rows:
        a, b = int(src[3][j]), int(src[3][j + 1])
        if b > a:
            packed[a + j % (b - a)] ^= 0xFF
        ver[j] = CRC_VERDICT
    return (bytes(packed),) + tuple(src[1:]), ver


def lose(con, rows):
    """lose_host for a Container"""
    src, ver = lose_host(con.model(False), rows)
    return con.edited(packed=src[0][: con.plen]), ver


def spoil(par_off, m, g, usable):
    """a byte of every parity row of group g that is not in ``usable`` (for ParitySet.damaged(par=...) or spoiled())"""
    assert par_off[g * m + 1] - par_off[g * m] >= 16, "a group without a stored byte has no parity byte to flip"
    return [int(par_off[g * m + p]) + 7 for p in range(m) if p not in usable]


def spoiled(pset, at):
    """a model's parity set with these bytes flipped as ParitySet.damaged flips them"""
    par = bytearray(pset["par"])
    for a in at:
        par[a] ^= 0x40
    return dict(pset, par=bytes(par))


def stored_lens(src):
    nb = int(src[2][-1])
    return np.diff(np.asarray(src[3][: nb + 1], dtype=np.int64))


# ---- the inputs of tests/test_gpu_parity_edges.py, with the assertions that they reach what they are named for -------------------------
# (1) every parity subset at high member indices: 509 rows at k = 255 are two groups, of 255 and of 254 members; row 2 i + g is member i
# of group g
SUBSETS = [(0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)]
HIGH = (0, 85, 127, 128, 170, 200, 253, 254)
SUB_B, SUB_K, SUB_NB = 4096, 255, 509


def subset_table():
    lens = np.random.RandomState(41).choice([4096, 4095, 3000, 64, 17, 16, 15, 1, 0], SUB_NB)
    lens[0], lens[2 * 85], lens[2 * 128], lens[2 * 254] = 4096, 3000, 0, 17   # members 0, 85, 128 (a row of no bytes) and 254 of group 0
    assert set(lens.tolist()) == {4096, 4095, 3000, 64, 17, 16, 15, 1, 0} and lens[0::2].max() == lens[1::2].max() == 4096
    assert (len(lens[0::2]), len(lens[1::2])) == (255, 254), "unequal groups: member 254 exists in group 0 alone"
    return lens


def subset_cases(m):
    """[(parities of group 0 left usable, members of group 0 lost, members of group 1 lost)]: every subset of the m parities that the
    damage pass can come to use, with e = 1 .. its size members lost; group 1 keeps all its parities"""
    singles, n, out = [128, 0, 254, 85, 127, 170, 200, 253], 0, []
    if m == 2:                                                                 # {1} alone and {0, 1}
        out = [((1,), [254]), ((1,), [128]), ((0, 1), [170]), ((0, 1), [0, 85]), ((0, 1), [128, 254])]
    for s in SUBSETS if m == 3 else ():
        out.append((s, [singles[n % 8]]))
        n += 1
        if len(s) >= 2:
            out.append((s, [0, 85]))
        if s in ((0, 2), (1, 2)):                                              # the two matrices that are not plain Vandermonde: a second pair
            out.append((s, [128, 254] if s == (0, 2) else [127, 253]))
        if len(s) == 3:
            out.append((s, [0, 128, 254]))
    other = ([253], [], [0, 127], [200])
    return [(s, lost, other[i % 4]) for i, (s, lost) in enumerate(out)]


def subset_overflows():
    """one lost member too many for a usable set of each size; group 1 loses member 253 and gets it back"""
    return [((2,), [0, 85], [253]), ((0, 2), [0, 128, 254], [253]), ((0, 1, 2), [0, 85, 170, 254], [253])]


def subset_rows(lost0, lost1):
    return [2 * i for i in lost0] + [2 * i + 1 for i in lost1]


def subset_conditions(lens, cases, m):
    """before anything runs: what the cases make the damage pass use is every subset, a lost member index needs the eighth bit of its byte
    and wraps gf_exp's n %= 255 (2 * 128), the pair (0, 85) and the triple (0, 128, 254) occur, and a lost row has no bytes"""
    used = {s[: len(lost)] for s, lost, _ in cases}
    assert used == ({s for s in SUBSETS} if m == 3 else {(1,), (0,), (0, 1)}), used
    assert all(len(lost) <= len(s) and set(lost) <= set(HIGH) for s, lost, _ in cases)
    assert any(max(lost) >= 128 and 2 in s[: len(lost)] for s, lost, _ in cases) or m < 3, "no product p i that wraps"
    assert any(lost == [0, 85] for _, lost, _ in cases) and (m < 3 or any(lost == [0, 128, 254] for _, lost, _ in cases))
    assert any(lens[2 * i] == 0 for _, lost, _ in cases for i in lost)
    assert any(254 in lost for _, lost, _ in cases) and any(253 in other for _, _, other in cases), "the last member of either group"


# (2) every member position of a small group: k = nb = 1 .. 9 at m = 1
SMALL_LENS = [100, 4096, 17, 0, 33, 16, 1, 250, 64]


# (3) rebuild across column tiles (a tile is 4096 bytes of the group's column): six rows at B = 65536 whose longest puts plen on a tile
# seam and 16 bytes either side of it. At (6, 3) one group; at (4, 2) group 0 = rows 0, 2, 4 and group 1 = rows 1, 3, 5, both of them long
TILE_B = 65536
TILE_LOSSES = {(6, 3): [[0], [2], [4], [0, 2], [0, 3, 4], [5, 1, 3]], (4, 2): [[0], [2], [0, 4], [1, 3], [3, 5, 4]]}


def tile_tables():
    """[(plen, lens)] for plen = 4096 t - 16, 4096 t and 4096 t + 16, t = 1 .. 3"""
    return [(plen, [plen - 3, 100, 17, plen - 16, 5101 if plen > 5200 else 4000, 1]) for t in (1, 2, 3) for plen in (4096 * t - 16, 4096 * t, 4096 * t + 16)]


def tile_situations(B, lens, k, m, lost):
    """the situations of the solve pass that losing ``lost`` from rows of these lengths meets, by name"""
    nb, out = len(lens), set()
    G = (nb + k - 1) // k
    tile = lambda n: (n - 1) // 4096
    for g in range(G):
        mine = [j for j in lost if j % G == g]
        plen = (max(lens[j] for j in range(g, nb, G)) + 15) // 16 * 16
        for j in mine:
            if B > 4096 and lens[j] and tile(lens[j]) >= 1 and tile(lens[j]) == tile(plen):
                out.add("a lost row that ends in the last tile, beyond tile 0")
            if B > 4096 and 0 < lens[j] < 4096 and tile(plen) >= 2:
                out.add("a lost row under one tile in a group of three tiles or more")
            if B > 4096 and lens[j] % 16 and tile(lens[j]) == 1:
                out.add("a lost row of a length that is no multiple of 16 and ends in tile 1")
        if len(mine) in (2, 3) and len({lens[j] for j in mine}) == len(mine):
            out.add("%d lost rows of different lengths" % len(mine))
        assert len(mine) <= m
    return out


TILE_SITUATIONS = {"a lost row that ends in the last tile, beyond tile 0", "a lost row under one tile in a group of three tiles or more",
                   "a lost row of a length that is no multiple of 16 and ends in tile 1", "2 lost rows of different lengths", "3 lost rows of different lengths"}


def tile_conditions(tables):
    """before anything runs: every seam and every situation occurs, at both shapes"""
    assert sorted(p for p, _ in tables) == sorted(4096 * t + d for t in (1, 2, 3) for d in (-16, 0, 16))
    for (k, m), losses in TILE_LOSSES.items():
        met = set()
        for plen, lens in tables:
            assert (max(lens) + 15) // 16 * 16 == plen
            for lost in losses:
                met |= tile_situations(TILE_B, lens, k, m, lost)
        assert met >= TILE_SITUATIONS - ({"3 lost rows of different lengths"} if m < 3 else set()), ((k, m), TILE_SITUATIONS - met)


# (4) a table past one tile of the running sum (8192 entries) and past one workgroup of the passes that take a lane per group (256)
SCAN_TILE = 8192
BIG_B, BIG_NB, BIG_NBT = 4096, 20000, 20003
BIG_SHAPES = {(2, 3): 4, (7, 1): 7, (255, 2): 1}                # (k, m): every how many groups one loses a member
BIG_FIXED = [0, 8191, 8192, 8193, 16383, 16384, BIG_NB - 1]    # either side of the running sum's seams, the first row and the last


def big_table():
    lens = np.random.RandomState(43).choice([0, 1, 5, 15, 16, 17, 31, 33, 48, 100], BIG_NB)
    lens[8192], lens[16383] = 33, 17
    return lens


def big_losses(k, m):
    """(rows to lose, the group that loses one row too many, how many of its parity rows are spoiled for that): BIG_FIXED, a member in
    every BIG_SHAPES[k, m]-th group, and the group in the middle of the table -- with min(its members, m + 1) rows lost, and where it has
    no more members than parities (k = 2 under m = 3) parity rows spoiled until one too few is usable"""
    nb, step = BIG_NB, BIG_SHAPES[k, m]
    G = (nb + k - 1) // k
    members = lambda g: (nb - g + G - 1) // G
    X = G // 2 + 1
    lost = {}
    for j in BIG_FIXED:
        assert j % G != X and len(lost.setdefault(j % G, set())) < m
        lost[j % G].add(j // G)
    for g in range(0, G, step):
        if g != X and g not in lost:
            lost[g] = {(7 * g) % members(g)}
    cnt = members(X)
    e = min(cnt, m + 1)
    lost[X] = set(list(dict.fromkeys([0, cnt - 1, cnt // 2, 1]))[:e])
    assert len(lost[X]) == e
    rows = sorted(i * G + g for g, mem in lost.items() for i in mem)
    return rows, X, (m - (e - 1) if e <= m else 0)


def big_conditions(k, m, rows, X):
    """before anything runs: both running sums pass their first tile, the rows either side of a tile seam are lost, and the damaged groups
    come from more than one workgroup of the damage pass where the table has that many groups"""
    G = (BIG_NB + k - 1) // k
    gmax, Q = Y.geometry(BIG_NBT, k, m)
    groups = {j % G for j in rows}
    assert BIG_NBT > 2 * SCAN_TILE and set(BIG_FIXED) <= set(rows) and X in groups
    if (k, m) == (2, 3):
        assert G == 10000 and Q > 3 * SCAN_TILE
    assert len(groups) >= min(300, G)
    assert len({g // 256 for g in groups}) >= min(2, (G + 255) // 256), "records from one workgroup only"
    return len(groups) - 1                                       # the groups listed for the solve pass


# (5) every pair (start of the row mod 16, length mod 16)
ALIGN_B, ALIGN_NB, ALIGN_SHAPE = 4096, 2000, (4, 2)


def align_table():
    lens = np.random.RandomState(40).randint(16, 81, ALIGN_NB)
    start = (3 + np.concatenate([[0], np.cumsum(lens)[:-1]])) % 16
    assert len(set(zip(start.tolist(), (lens % 16).tolist()))) == 256, "not every pair of residues"
    return lens, start


def align_losses(lens, start):
    """a lost row for every start residue r, of the length residue (7 r + 3) % 16, each in a group of its own; for an even r a second member
    of its group is lost with it"""
    k, m = ALIGN_SHAPE
    G = (ALIGN_NB + k - 1) // k
    rows, groups = [], set()
    for r in range(16):
        j = next(j for j in range(ALIGN_NB) if start[j] == r and lens[j] % 16 == (7 * r + 3) % 16 and j % G not in groups)
        groups.add(j % G)
        rows += [j] if r % 2 else [j, (j + G) % ALIGN_NB]
    assert len(set(rows)) == 24 and {int(start[j]) for j in rows} == set(range(16)) and {int(lens[j]) % 16 for j in rows} == set(range(16))
    return sorted(rows)
