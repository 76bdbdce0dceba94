"""What the far-offset tests share (test_far_rig.py on the CPU, test_gpu_far_plans.py and test_gpu_far_blocks.py on the GPU): every offset
a caller hands the library is 64 bits wide, and these tests hand it offsets that need more than 31 and more than 32 bits. A far offset
needs a large address range, not large data: one arena of 4 GiB + 64 MiB is allocated once per process and never filled as a whole; a case
claims a few small windows of it (Window), writes only those, and reads only those back.

BASES are the three places a case's first buffer starts at: 2051 bytes below 2^31, 2053 bytes below 2^32 (the first buffer of every case
is at least 4 KiB long, so it starts below the boundary and ends above it) and 4099 bytes above 2^32. All are odd. An offset cut to 32 or
31 bits lands at the window's alias (base mod 2^32, base mod 2^31), which the case owns too: the alias of an output window holds a canary
that must survive the call, the alias of an input window a decoy -- other input of the same lengths, so that a cut read gives wrong bytes
or a wrong status, both of which the comparisons with the oracle see. Every window has EDGE guard bytes on either side.

Input and output of a call live in the one arena, as disjoint windows, and the arena is passed as both d_in and d_out (no entry point
refuses equal base pointers; none is told a buffer's size). The arena's claims keep the windows, guards and aliases of a case pairwise
disjoint and inside the arena: Window's constructor asserts it.

The two sides of a case cannot both sit at the three bases: a window at "4g" has its 31-bit alias where a window at "2g" lies, and
reaches up to where one at "above" begins. So the side opposite "4g" lies 32 MiB further up ("above+", also odd and wholly above 2^32),
and the pairs of places a case uses are fixed here (PAIR, and MOVED for the second execution of a plan with device tables): every base
is an input place and an output place of some execution.
HostArena is a sparse stand-in with the same methods, so that the arithmetic is pinned without a device. torch is imported inside the
functions that need it. Not collected as a test."""
import contextlib

import numpy as np

import plans_rig as PR

ARENA_BYTES = (1 << 32) + (1 << 26)
BASES = {"2g": (1 << 31) - 2051, "4g": (1 << 32) - 2053, "above": (1 << 32) + 4099}
BOUNDARY = {"2g": 1 << 31, "4g": 1 << 32}                        # what the first buffer at this base straddles
PLACES = dict(BASES, **{"above+": BASES["above"] + (1 << 25)})   # "above+": where the other side of a case at "4g" goes (see PAIR)
PAIR = {"2g": ("2g", "above"), "4g": ("4g", "above+"), "above": ("above", "2g")}           # (input place, output place) of the case of a base
MOVED = {"2g": ("above+", "4g"), "4g": ("above", "2g"), "above": ("above+", "4g")}         # ... of a dev plan's second execution
EDGE = 64                                                        # guard bytes on either side of a window and of its aliases
GUARD, CANARY = PR.GUARD, 0xC3                                   # what a window and the alias of an output window hold before a call
FIRST_MIN = 4096                                                 # the least length of a case's first buffer on either side
_arenas = {}


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


class _Claims:
    """the spans of the arena that the windows of the running case own"""

    def _init_claims(self, size):
        self.size, self.claims = size, []

    def claim(self, spans):
        """all of ``spans`` (lo, hi, what) or none of them: each inside the arena and disjoint from every other span claimed"""
        held = list(self.claims)
        for lo, hi, what in spans:
            assert 0 <= lo <= hi <= self.size, ("outside the arena", what, lo, hi)
            for a, b, w in held:
                assert hi <= a or b <= lo, ("windows overlap", what, (lo, hi), w, (a, b))
            held.append((lo, hi, what))
        self.claims[:] = held

    @contextlib.contextmanager
    def case(self):
        """the windows claimed inside are given back at its end; those claimed before stay (a module's far containers)"""
        mark = len(self.claims)
        try:
            yield self
        finally:
            del self.claims[mark:]

    def fill(self, lo, hi, v):
        self.write(lo, np.full(hi - lo, v, dtype=np.uint8))


class HostArena(_Claims):
    """the arena without a device: the bytes written, kept by 64 KiB page; a byte never written reads as 0"""
    PAGE = 1 << 16
    t = None                                                     # (no tensor: a far container on it has no d_packed)

    def __init__(self, size=ARENA_BYTES):
        self._init_claims(size)
        self.pages = {}

    def _each(self, at, n):
        while n:
            p, o = divmod(at, self.PAGE)
            k = min(n, self.PAGE - o)
            yield p, o, k
            at, n = at + k, n - k

    def write(self, at, data):
        data, done = u8(data), 0
        assert 0 <= at and at + len(data) <= self.size
        for p, o, k in self._each(at, len(data)):
            self.pages.setdefault(p, np.zeros(self.PAGE, dtype=np.uint8))[o: o + k] = data[done: done + k]
            done += k

    def read(self, at, n):
        assert 0 <= at and at + n <= self.size
        parts = [self.pages[p][o: o + k] if p in self.pages else np.zeros(k, dtype=np.uint8) for p, o, k in self._each(at, n)]
        return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


class DevArena(_Claims):
    """the arena in device memory: ``t`` is the tensor a call takes as d_in, d_out or d_packed"""

    def __init__(self, t):
        self._init_claims(t.numel())
        self.t = t

    def fill(self, lo, hi, v):
        self.t[lo:hi].fill_(v)

    def write(self, at, data):
        import torch
        data = u8(data)
        assert 0 <= at and at + len(data) <= self.size
        if len(data):
            self.t[at: at + len(data)].copy_(torch.from_numpy(data.copy()))

    def read(self, at, n):
        assert 0 <= at and at + n <= self.size
        return self.t[at: at + n].cpu().numpy()


def arena(ctx):
    """the one arena of this process on the context's device, uninitialised. Only this allocation may skip."""
    import pytest
    import torch
    if ctx.device not in _arenas:
        dev = torch.device("cuda", ctx.device)
        try:
            _arenas[ctx.device] = DevArena(torch.empty(ARENA_BYTES, dtype=torch.uint8, device=dev))
        except torch.cuda.OutOfMemoryError:
            free, total = torch.cuda.mem_get_info(dev)
            pytest.skip("no room for the far arena of %d bytes: %d of %d bytes free" % (ARENA_BYTES, free, total))
    return _arenas[ctx.device]


def alias_bases(base):
    """where an offset of ``base`` lands when it is cut to 32 and to 31 bits, where that is another place"""
    return [b for b in dict.fromkeys((base % (1 << 32), base % (1 << 31))) if b != base]


def straddles(name, at, n):
    """the n bytes at ``at`` begin below the boundary of base ``name`` and end above it"""
    return at < BOUNDARY[name] < at + n


class Window:
    """``room`` bytes of the arena at ``base`` with EDGE guard bytes around them, and the same range at every alias of base: all filled
    here -- the window with GUARD, an alias with CANARY -- and all claimed, so that two windows of a case can never meet."""

    def __init__(self, arena, base, room, what="window"):
        self.a, self.base, self.room, self.what = arena, int(base), int(room), what
        self.lo, self.hi = self.base - EDGE, self.base + self.room + EDGE
        self.aliases = alias_bases(self.base)
        arena.claim([(self.lo, self.hi, what)] + [(b - EDGE, b + self.room + EDGE, what + " alias") for b in self.aliases])
        arena.fill(self.lo, self.hi, GUARD)
        self.shadow = {}
        for b in self.aliases:
            arena.fill(b - EDGE, b + self.room + EDGE, CANARY)
            self.shadow[b] = np.full(self.room + 2 * EDGE, CANARY, dtype=np.uint8)

    def refill(self):
        """guard bytes over the window again (between two executions); the aliases keep what they hold"""
        self.a.fill(self.lo, self.hi, GUARD)

    def put(self, at, data):
        """data at byte ``at`` of the window"""
        assert 0 <= at and at + len(data) <= self.room
        self.a.write(self.base + at, data)

    def put_alias(self, at, data):
        """data (a decoy) at byte ``at`` of every alias"""
        data = u8(data)
        assert 0 <= at and at + len(data) <= self.room
        for b in self.aliases:
            self.a.write(b + at, data)
            self.shadow[b][EDGE + at: EDGE + at + len(data)] = data

    def get(self, at=0, n=None):
        n = self.room - at if n is None else n
        assert 0 <= at and at + n <= self.room
        return self.a.read(self.base + at, n)

    def image(self):
        """the window with its guards, [base - EDGE, base + room + EDGE): byte x of the window is image()[EDGE + x]"""
        return self.a.read(self.lo, self.hi - self.lo)

    def guards_intact(self, used=()):
        """everything of the window and its edges outside the (at, n) ranges of ``used`` still holds GUARD"""
        keep = np.ones(self.hi - self.lo, dtype=bool)
        for at, n in used:
            keep[EDGE + int(at): EDGE + int(at) + int(n)] = False
        img = self.image()
        bad = np.nonzero(img[keep] != GUARD)[0]
        assert bad.size == 0, (self.what, "written outside its ranges", int(np.nonzero(keep)[0][bad[0]]) - EDGE)
        return True

    def aliases_intact(self):
        """every alias, edges included, holds what was put there: the canary, or the decoy"""
        for b in self.aliases:
            got = self.a.read(b - EDGE, self.room + 2 * EDGE)
            bad = np.nonzero(got != self.shadow[b])[0]
            assert bad.size == 0, (self.what, "alias at", b, "touched at byte", int(bad[0]) - EDGE)
        return True


class FarBytes:
    """what a model takes as ``packed`` for a container whose stored bytes lie at ``base``: as long as base + the data, a slice inside
    [base, base + len(data)) gives the bytes, and any other read raises -- a model that read in front of the container would fail"""

    def __init__(self, base, data):
        self.base, self.data = int(base), bytes(data)

    def __len__(self):
        return self.base + len(self.data)

    def __getitem__(self, s):
        if not isinstance(s, slice):
            raise TypeError("FarBytes gives slices only")
        if s.step not in (None, 1) or s.start is None or s.stop is None:
            raise IndexError("FarBytes: an open or strided slice")
        a, b = int(s.start), int(s.stop)
        if not self.base <= a <= b <= len(self):
            raise IndexError("FarBytes: [%d, %d) outside [%d, %d)" % (a, b, self.base, len(self)))
        return self.data[a - self.base: b - self.base]

    def __bytes__(self):
        raise TypeError("FarBytes: read as a whole")

    def __iter__(self):
        raise TypeError("FarBytes: read as a whole")


# ---- batches of units ---------------------------------------------------------------------------------------------------------------------
SHAPE = (("lz", 70000), ("words", 4097), ("random", 300), ("random", 1), ("random", 0))   # the five units of every plan case
CAPS = {"exact": lambda n: n, "short": lambda n: max(0, n - 1), "generous": lambda n: n + 5000}   # decompress capacities by plain length
_streams = {}


def units(seed):
    """the five units of SHAPE from cases.family; seed 1 is the data, seed 2 the decoy"""
    import random
    import cases
    rnd = random.Random(seed)
    return [cases.family(k, n, rnd) for k, n in SHAPE]


def streams(oracle, f):
    """(units(1), their streams, decoy streams), once per format: a decoy is the stream of the same unit of units(2), cut or zero-padded
    to the length of the real one (a raw-stored unit keeps its length, so its decoy is a valid stream; the others decode to an error or to
    other bytes, and both differ from the oracle's answer for the real stream)"""
    if f not in _streams:
        plain = units(1)
        comp = [oracle.oracle_compress(f, u)[1] for u in plain]
        other = [oracle.oracle_compress(f, u)[1] for u in units(2)]
        decoy = [(o + bytes(len(c)))[: len(c)] for o, c in zip(other, comp)]
        assert all(d != c for d, c in zip(decoy[:4], comp[:4]))
        _streams[f] = (plain, comp, decoy)
    return _streams[f]


def far_batch(batch, base_in, base_out):
    """a plans_rig.layout batch with its two offset columns shifted: the first unit's input at base_in, its capacity at base_out. The blob
    and out_total stay what they were: the lengths of the two windows (in_window, out_window)."""
    assert int(batch.in_off[0]) == 0 and int(batch.out_off[0]) == PR.GAP
    return batch._replace(in_off=batch.in_off + np.uint64(base_in), out_off=batch.out_off + np.uint64(base_out - PR.GAP))


class FarRun:
    """the two windows of a far batch in an arena: the blob written into the input window (and ``decoy``, a blob of the same length,
    into its aliases), the output window guard-filled, its aliases canaries"""

    def __init__(self, arena, near, base_in, base_out, decoy=None):
        self.near, self.batch = near, far_batch(near, base_in, base_out)
        self.win = Window(arena, base_in, len(near.blob), "input")
        self.wout = Window(arena, base_out - PR.GAP, near.out_total, "output")
        self.win.put(0, near.blob)
        if decoy is not None:
            assert len(decoy) == len(near.blob)
            self.win.put_alias(0, decoy)

    def intact(self):
        """the input window and its edges are what was written; both windows' aliases hold what was put there; the output window's
        edges are guards (inside it, plans_rig.same / guards_intact look, on result()'s bytes)"""
        img = self.win.image()
        assert (img[:EDGE] == GUARD).all() and (img[EDGE + self.win.room:] == GUARD).all(), "input edges"
        assert bytes(img[EDGE: EDGE + self.win.room]) == bytes(self.near.blob), "the input was written"
        img = self.wout.image()
        assert (img[:EDGE] == GUARD).all() and (img[EDGE + self.wout.room:] == GUARD).all(), "output edges"
        return self.win.aliases_intact() and self.wout.aliases_intact()


# ---- containers -----------------------------------------------------------------------------------------------------------------------------
def far_container(con, arena, base, decoy=None):
    """Container.far of ``con`` with its stored bytes written at ``base`` of the arena, in a window of their own (returned container's
    ``win``); ``decoy``: other stored bytes of the same length (another container's under the same table) for the window's aliases"""
    win = Window(arena, base, con.plen, "container")
    win.put(0, con.packed)
    if decoy is not None:
        assert len(decoy) == con.plen
        win.put_alias(0, decoy)
    c = con.far(arena, base)
    c.win = win
    return c


def decoy_stored(oracle, con):
    """the stored bytes of ``con`` with one byte of every block changed: a raw block's sixth (or last) byte, a compressed block's byte that
    still decodes (blocks_rig.flip) where there is one, else one that does not; kept with the container"""
    from blocks_rig import flip
    if getattr(con, "decoy", None) is None:
        out = bytearray(con.packed)
        for r in range(con.n):
            for k in range(con.blocks(r)):
                j, e = int(con.first[r]) + k, min(con.B, con.lens[r] - k * con.B)
                o0, o1 = int(con.off[j]), int(con.off[j + 1])
                if o1 - o0 == e:
                    out[o0 + min(5, e - 1)] ^= 0xFF
                    continue
                try:
                    at = flip(oracle, con, j, e, True)
                except AssertionError:
                    at = flip(oracle, con, j, e, False)
                out[at] ^= 0x01
        con.decoy = bytes(out)
        assert con.decoy != con.packed
    return con.decoy


def far_of(oracle, arena, con, place):
    """the far copy of a near container at a place of PLACES, decoy_stored in its aliases; its first stored block straddles the boundary"""
    c = far_container(con, arena, PLACES[place], decoy_stored(oracle, con))
    assert place.startswith("above") or straddles(place, int(c.off[0]), int(c.off[1] - c.off[0]))
    return c


def settled(*cons):
    """after a call: the stored bytes of the far containers, their guards and their aliases are what was written"""
    for c in cons:
        assert bytes(c.win.get()) == c.packed.data and c.win.guards_intact([(0, c.win.room)]) and c.win.aliases_intact()
    return True


def plain_window(arena, place, bufs, room, what):
    """buffers at the odd spacing of blocks_rig.odd_offsets in a far window, the same buffers with every byte inverted in its aliases:
    (window, absolute offsets, offsets inside the window)"""
    from blocks_rig import odd_offsets
    off, blob = odd_offsets(bufs, room)
    w = Window(arena, PLACES[place], room, what)
    w.put(0, blob)
    w.put_alias(0, odd_offsets([inverted(b) for b in bufs], room)[1])
    assert place.startswith("above") or straddles(place, w.base + off[0], len(bufs[0]))
    return w, [w.base + o for o in off], off


def same(a, b, what=""):
    """two model answers, whole: dicts, lists and tuples entry by entry, arrays and bytes by value"""
    if isinstance(a, dict):
        assert isinstance(b, dict) and a.keys() == b.keys(), what
        for k in a:
            same(a[k], b[k], (what, k))
    elif isinstance(a, (list, tuple)) and not isinstance(b, np.ndarray):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, (what, i))
    elif isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        assert np.array_equal(np.asarray(a), np.asarray(b)), what
    else:
        assert a == b, (what, a, b)
    return True


def inverted(b):
    return bytes(255 - u8(b))


# ---- the cases of tests/test_gpu_far_blocks.py, which tests/test_far_rig.py runs through the models alone --------------------------------------
ALL = (1 << 64) - 1
SECOND = (2, 0, 1)                                               # the order of the store's buffers in the second source of a call
RANGES = [(1, 2), (0, 9), (0, 1)]                                # the middle blocks; clipped at the end; the one block
PICKS = [(1, 0), (0, 0), (0, 2), (1, 1), (0, 7), (0, 1), (1, 2)]  # both sources by turns; (0, 7) names no resource
EXTENTS = [[(0, 0, 1, 2), (1, 0, 0, 1)], [(1, 1, 0, 4)], [(0, 0, 3, 1)], [(2, 0, 0, 1)], [], [(1, 2, 0, 5), (0, 1, 1, 3)]]   # (2, ...) names no source
TRANSCODES = [("join", 2, 4096, 2, 16384), ("split", 2, 16384, 2, 4096), ("codec", 2, 4096, 3, 4096), ("wide", 4, 65536, 3, 65536)]
PARITY = (4, 2)                                                  # k, m


def store_buffers(B, order=(0, 1, 2)):
    import sync_model as Y
    bufs = Y.store_buffers(B)
    return [bufs[i] for i in order]


def edited_buffers(B):
    """a later version of the store: a block of the first resource overwritten, the second shortened by a block, the third grown"""
    import sync_model as Y
    A, Z, X = Y.store_buffers(B)
    return [A[:B] + Y.rnd(51, B) + A[2 * B:], Z[: 4 * B], X + Y.rnd(52, 100)]


def collision_buffers(B):
    """dedup_model's full-key collision: ([data, 7 bytes], [its CRC twin, data])"""
    import blocks_model as M
    import dedup_model as D
    data = M.build({"kind": "random", "seed": 9, "mult": 3, "add": 17}, B)
    twin = D.crc_twin(data, B + B // 2)
    assert twin != data
    return [data, np.random.RandomState(3).bytes(7)], [twin, data]


def read_requests(B, n):
    """the whole first resource (the first output buffer straddles), ranges that straddle blocks, a short last block, one refusal"""
    return [(0, 0, ALL), (0, B - 3, 10), (1, B + 100, 2 * B), (2, 5, 100), (0, 3 * B - 1, 18), (1, 0, ALL), (n + 4, 0, 1), (2, B - 1, 5)]


def write_requests(B, n, L):
    """(requests, the kinds of blocks_rig.sources): the first source buffer straddles; (n + 2, ...) names no resource"""
    return ([(0, 0, B + 100), (0, B - 3, 10), (1, B - 1, B + 2), (0, L - 1, 1), (2, 0, ALL), (1, 2 * B + 5, ALL), (n + 2, 0, 9), (0, L, ALL)],
            [1, 2, 1, 1, 0, 2, 1, 1])


def resize_want(lens, B):
    return [B + 5, lens[1], B + 100]                            # a cut inside a block; untouched; a raw block extended by zeros


def decode_cases(bufs, B):
    """(ranges, the resource whose capacity is a byte short, capacities) of the decompress cases"""
    out = []
    for ranges, short in ((None, None), (RANGES, None), (None, 1)):
        want = [len(b) if ranges is None else len(b[f0 * B: (f0 + c) * B]) for b, (f0, c) in zip(bufs, ranges or [(0, 0)] * len(bufs))]
        out.append((ranges, short, [w - 1 if r == short else w for r, w in enumerate(want)]))
    return out


def damaged_stored(oracle, con):
    """the stored bytes of the store with its first block, stored raw, hurt (seen by its checksum) and its second, compressed, made
    undecodable"""
    from blocks_rig import flip
    j = int(con.first[0])
    out = bytearray(con.packed)
    assert int(con.off[j + 1] - con.off[j]) == con.B and int(con.off[j + 2] - con.off[j + 1]) < con.B
    out[int(con.off[j]) + 7] ^= 0xFF
    out[flip(oracle, con, j + 1, con.B, False)] ^= 0x01
    return bytes(out)
