"""GPU: the scratch contract -- what an execution reads from scratch it has written itself, and no kernel touches the
slack behind the bytes a buffer was reserved for.

Every case makes its plan or object on a FRESH context with bounds equal to its batch, executes once into guard-filled outputs and checks
the result as the module that owns the operation does (the oracle, or that module's model). Then, for 0x00, 0xFF and 0xA5 in turn, it
fills every buffer the context and the target own with that byte (mscomp_amd_debug_scratch_poison; a host plan's uploaded tables: their
slack alone), executes again on the same plan -- eager, captured and replayed executions all occur -- and requires the complete output
image, guards included, every length and every status to be those of the first execution, and every slack byte [asked, cap) of every buffer
to hold the poison still (mscomp_amd_debug_scratch_report). Last it shows that the instrument can fail: slack filled with 0x11 and read
against 0x22 reports every buffer with slack as damaged.

Each case names the context buffers of the path it is about (CLAIMS) and asserts from the report that they were reserved;
test_every_context_buffer_is_claimed_by_a_case asserts that the cases together name every buffer a context has."""
import ctypes as C

import numpy as np
import pytest

import cases
import test_foreign_streams as tf
import crc_model as K
import blocks_model as M
import blocks_rig as G
import plans_rig as PR
import read_model as R
from plans_rig import FMTS, GUARD, LZG_MIN_CAP, XPS_MIN_IN

pytestmark = pytest.mark.gpu
POISONS = (0x00, 0xFF, 0xA5)

SCAN = ("prefix", "tile_sums")
CLAIMS = {                                                             # the context buffers each kind of case shows to be reserved
    ("compress", 2): ("slots", "slot_size", "lzrec") + SCAN,
    ("compress_sa", 2): ("slots", "slot_size") + SCAN,
    ("compress", 3): ("links", "lasthead", "mlen3", "wtok", "wmat", "wfar"),
    ("compress_mode4", 3): ("links", "lasthead", "mlen3", "wtok", "wmat", "wfar", "wrec", "sbrec"),
    ("compress", 4): ("links", "lasthead", "mlen3", "tokbits", "counts", "extra", "lens", "codes", "fb_list", "fbflag", "slot_size") + SCAN,
    ("decode", 2): ("dz_cin", "dz_csize", "dz_unit") + SCAN,
    ("decode", 3): ("dz_tok", "dz_ntok"),
    ("decode", 4): ("dz_tok", "dz_ntok", "dz_xhc", "dz_scr"),
    ("size", 2): ("dz_cin", "dz_csize", "dz_unit") + SCAN,
    ("size", 3): ("dz_ntok",),
    ("size", 4): ("dz_ntok", "dz_xhc"),
    ("large", 3): ("dz_tok", "dz_ntok", "xps_buf", "lzg_bsum", "lzg_dir", "lzg_words"),
    ("large", 4): ("dz_tok", "dz_ntok", "dz_xhc", "dz_scr", "lzg_bsum", "lzg_dir", "lzg_words"),
    ("compact",): ("cp_tab",),
    ("one_shot",): ("one_in", "one_out", "one_meta"),
}
_memo = {}


def _memoized(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


@pytest.fixture
def ctx():
    """a fresh context per case: `asked` of its buffers is this case's own"""
    import torch
    import ms_compress_amd as m
    c = m.Context()
    yield c
    torch.cuda.synchronize()
    c.close()                                                      # (and with it what a failed case left open)


@pytest.fixture(scope="module")
def fixture():
    return M.load()


def _slack_clean(target, byte, what):
    import ms_compress_amd as m
    rep = m.api.scratch_report(target, byte)
    bad = {k: v for k, v in rep.items() if v[2]}
    assert not bad, "%s: slack bytes touched (name: asked, cap, changed) %r" % (what, bad)
    return rep


ASSERTED = set()                                                      # the context buffers a case has shown to be reserved, over the cases that ran


def _poison(target, byte, whole):
    """fill `target`. The count is that of its buffers with bytes to fill -- for a context, all the buffers it has but the empty ones --
    and a report against the same byte right afterwards finds every slack byte filled"""
    import ms_compress_amd as m
    before = m.api.scratch_report(target, byte)
    want = sum(1 for a, c, _ in before.values() if (c > 0 if whole else a < c))
    if whole and (target is None or isinstance(target, m.Context)):
        assert want == len(m.api.scratch_names()) - sum(1 for _, c, _ in before.values() if c == 0)
    assert m.api.scratch_poison(target, byte, slack_only=not whole) == want, (want, before)
    after = m.api.scratch_report(target, byte)
    assert {k: v[:2] for k, v in after.items()} == {k: v[:2] for k, v in before.items()}            # nothing moved or grew
    assert all(ch == 0 for _, _, ch in after.values()), ("the fill left slack bytes out", after)
    return want


def _same(base, got, what):
    assert len(base) == len(got)
    for k, (a, b) in enumerate(zip(base, got)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k)
        bad = np.nonzero(a.reshape(-1) != b.reshape(-1))[0]
        assert bad.size == 0, "%s: result %d differs from the first execution at %r (%d places)" % (what, k, bad[:8].tolist(), bad.size)


def cycle(ctx, runs, claims, targets=(), check=None):
    """steps 2-4 of the module's docstring. `runs`: one callable or a list of them -- the calls of the case, a healthy and a damaged input for
    instance; each executes once into freshly guard-filled outputs and returns its complete result as a tuple of arrays, and EVERY one of
    them is preceded by a poison of its own, so that no call starts from what the call before it left. check(result) (single runs)
    compares a result with the oracle or the model; targets: [(object, whole)] besides the context (`ctx` None: the calling thread's
    one-shot context); claims: context buffers that must have been reserved"""
    import ms_compress_amd as m
    runs = list(runs) if isinstance(runs, (list, tuple)) else [runs]
    base = [run() for run in runs]
    if check:
        check(base[0])
    rep = m.api.scratch_report(ctx, 0)
    assert sorted(rep) == sorted(m.api.scratch_names())
    for name in claims:
        assert rep[name][0] > 0 and rep[name][1] > rep[name][0], ("the case did not reserve", name, rep[name])
        ASSERTED.add(name)
    for obj, whole in targets:
        if not whole:
            assert m.api.scratch_poison(obj, 0xA5) == -1           # uploaded tables: the whole-buffer form is refused
    for byte in POISONS:
        for k, run in enumerate(runs):
            what = "call %d after poison 0x%02X" % (k, byte)
            assert _poison(ctx, byte, True) >= len(claims)
            for obj, whole in targets:
                _poison(obj, byte, whole)
            try:
                got = run()
            except AssertionError as e:                                # (a check inside run: say which poison it was)
                raise AssertionError("%s: %s" % (what, e)) from e
            _same(base[k], got, what)
            if check:
                check(got)
            _slack_clean(ctx, byte, "context, " + what)
            for obj, _ in targets:
                _slack_clean(obj, byte, "%s, %s" % (type(obj).__name__, what))
    # the instrument itself: slack that differs from the byte asked about is reported, in every buffer that has slack
    for t in [ctx] + [obj for obj, _ in targets]:
        n = _poison(t, 0x11, False)
        rep = m.api.scratch_report(t, 0x22)
        hit = [k for k, (a, c, ch) in rep.items() if a < c]
        assert len(hit) == n and all(rep[k][2] == rep[k][1] - rep[k][0] for k in hit), rep
        assert all(rep[k][2] == 0 for k in rep if k not in hit)
        _slack_clean(t, 0x11, "control")


def _check_against(batch, want, rejected=()):
    """want[i] = (status, bytes): status and length of every unit, its bytes where the status is MSCOMP_OK; guards; rejected units: ARG_ERROR, 0"""
    def check(res):
        for i, (ws, wb) in enumerate(want):
            if i in rejected:
                assert (int(res[1][i]), int(res[0][i])) == (-2, 0), i
                continue
            assert int(res[1][i]) == ws, (i, int(res[1][i]), ws)
            if ws == 0:
                assert int(res[0][i]) == len(wb) and PR.unit(res, batch, i) == wb, i
        PR.guards_intact(res, batch)
    return check


# ---- compress host plans -------------------------------------------------------------------------------------------------------------------
def _compress_units():
    return cases.edge_cases()[::3] + [cases.mixed_buffer()]


def _compress_want(oracle, f, sa=False, short=None):
    """([(status, bytes)] of the checker at the reference's largest size, the capacities of the case -- exactly the compressed size, or
    (short) one byte less --, [(status, bytes)] of the checker at those capacities)"""
    def make():
        comp = oracle.oracle_compress_sa if sa else (lambda u, c=None: oracle.oracle_compress(f, u, c))
        units = _compress_units()
        ref = [comp(u) for u in units]
        assert all(s == 0 for s, _ in ref)
        caps = [max(0, len(b) - (1 if short else 0)) for _, b in ref]
        return ref, caps, [comp(u, c) for u, c in zip(units, caps)]
    return _memoized(("cw", f, sa, bool(short)), make)


COMPRESS = [("lznt1", "exact", None), ("lznt1", "short", None), ("lznt1", "exact", ("lznt1", 1)), ("lznt1", "exact", ("lznt1", 2)), ("lznt1", "exact", ("sa", 1)),
            ("xpress", "exact", None), ("xpress", "short", None), ("xpress", "exact", ("emit", 1)), ("xpress", "exact", ("emit", 2)), ("xpress", "exact", ("emit", 3)),
            ("xpress", "exact", ("emit", 4)), ("xpress", "exact", ("finder", 2)),
            ("xpress_huff", "exact", None), ("xpress_huff", "short", None), ("xpress_huff", "exact", ("finder", 2))]


def _compress_claims(fmt, hook):
    f = FMTS[fmt]
    return CLAIMS[("compress_sa", 2)] if hook and hook[0] == "sa" else CLAIMS[("compress_mode4", 3)] if hook == ("emit", 4) else CLAIMS[("compress", f)]


@pytest.mark.parametrize("fmt,caps,hook", COMPRESS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_compress_host_plan(oracle, ctx, fmt, caps, hook):
    """all three formats on cases.edge_cases()[::3] + cases.mixed_buffer(), capacities exactly the compressed size, and one byte short
    (MSCOMP_BUF_ERROR for every unit with output); LZNT1 under both chunk kernels and the suffix-array flavour, Xpress under every emit
    kernel, Xpress and Xpress+Huffman under both finders -- the switch is set before the plan is made, so that its reserve sees it"""
    f, lib = FMTS[fmt], ctx.lib
    sa = hook is not None and hook[0] == "sa"
    units = _compress_units()
    ref, cap, want = _compress_want(oracle, f, sa, short=caps == "short")
    if caps == "exact":
        assert sum(w == r for w, r in zip(want, ref)) > len(units) // 2
    else:
        assert sum(s == -5 for s, _ in want) > len(units) // 2
    setter = {None: None, "lznt1": lib.mscomp_amd_debug_set_lznt1, "emit": lib.mscomp_amd_debug_set_xpress_emit, "finder": lib.mscomp_amd_debug_set_finder,
              "sa": None}[hook and hook[0]]
    try:
        if setter:
            setter(hook[1])
        if sa:
            ctx.set_lznt1_sa_dict(True)
        batch = PR.layout(units, cap)
        plan = PR.host_plan(ctx, f, batch, "compress")
        cycle(ctx, lambda: PR.host_execute(plan, batch), _compress_claims(fmt, hook), [(plan, False)], _check_against(batch, want))
        plan.close()
    finally:
        if setter:
            setter(1 if hook[0] == "finder" else 0)


# ---- decompress and size host plans ----------------------------------------------------------------------------------------------------------
def _decode_batch(oracle, f, family):
    """(units, capacities, [(status, bytes)] of the checker)"""
    def make():
        if family == "streams":
            pairs = cases.decode_streams(f, lambda d: oracle.oracle_compress(f, d)[1])
        else:
            pairs = [(s.data, s.cap) for s in tf.family(f)[0]]
        units, caps = [s for s, _ in pairs], [c for _, c in pairs]
        return units, caps, [oracle.oracle_decompress_ex(f, u, c)[:2] for u, c in pairs]
    return _memoized(("db", f, family), make)


@pytest.mark.parametrize("family", ["streams", "foreign"])
@pytest.mark.parametrize("kind", ["decode", "size"])
@pytest.mark.parametrize("fmt", list(FMTS))
def test_decode_and_size_host_plans(oracle, ctx, fmt, kind, family):
    """cases.decode_streams and the streams.FAMILIES variants (valid, cut, concatenated, corrupted, foreign streams): statuses, lengths and
    bytes are the checker's before and after every poison"""
    f = FMTS[fmt]
    units, caps, want = _decode_batch(oracle, f, family)
    assert sum(s == 0 for s, _ in want) > 20 and sum(s != 0 for s, _ in want) > 20
    batch = PR.layout(units, caps)
    plan = PR.host_plan(ctx, f, batch, kind)
    if kind == "decode":
        check = _check_against(batch, want)
    else:
        def check(res):
            for i, (ws, wb) in enumerate(want):
                assert (int(res[1][i]), int(res[0][i])) == (ws, len(wb) if ws == 0 else 0), i
            assert (res[2] == GUARD).all()
    cycle(ctx, lambda: PR.host_execute(plan, batch), CLAIMS[(kind, f)], [(plan, False)], check)
    plan.close()


def _large_units(oracle, f):
    """one unit just past the thresholds of the large-unit paths (512 KiB of Xpress input, 1 MiB of capacity), the same stream cut in
    half (it fails, or ends early) and at a capacity one byte short, between small units"""
    def make():
        import ms_compress_amd as m
        from ms_compress_amd import corpus
        plain = corpus.by_name("mozilla", 1_400_000).tobytes()
        comp = oracle.oracle_compress(f, plain)[1]
        assert len(plain) >= LZG_MIN_CAP and (f != 3 or len(comp) >= XPS_MIN_IN), (len(plain), len(comp))
        small = [oracle.oracle_compress(f, u)[1] for u in (b"small unit " * 50, plain[:70000])]
        pairs = [(small[0], 550), (comp, len(plain)), (comp[: len(comp) // 2], len(plain)), (small[1], 70000), (comp, len(plain) - 1)]
        units, caps = [s for s, _ in pairs], [c for _, c in pairs]
        return units, caps, [oracle.oracle_decompress_ex(f, u, c)[:2] for u, c in pairs]
    return _memoized(("lu", f), make)


@pytest.mark.parametrize("fmt", ["xpress", "xpress_huff"])
def test_large_unit_decode_host_plan(oracle, ctx, fmt):
    """the segment walk (Xpress), the all-CU byte stage and the candidate token scratch (Xpress+Huffman), with a failing unit among them"""
    import ms_compress_amd as m
    f = FMTS[fmt]
    units, caps, want = _large_units(oracle, f)
    assert want[1][0] == 0 and want[4][0] == -5
    batch = PR.layout(units, caps)
    plan = PR.host_plan(ctx, f, batch, "decode")
    paths = m.api.plan_paths(plan)
    assert paths[1] == 3 and (paths[0] == 2 if f == 3 else paths[2] > 0), paths     # (the half stream is below 512 KiB)
    ctx.lib.mscomp_amd_debug_lzg_open.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    words = sum(c + 64 for c in caps if c >= LZG_MIN_CAP)

    def run():                                                         # ... with what the debug hooks say of the paths: the per-unit verdicts, the words open after each pointer pass
        res = PR.host_execute(plan, batch)
        modes, opened = np.zeros(8, np.uint32), np.zeros(33, np.uint32)
        k = ctx.lib.mscomp_amd_debug_decode_modes(ctx._h, modes.ctypes.data, 8)
        assert k >= 0 and ctx.lib.mscomp_amd_debug_lzg_open(ctx._h, words, opened.ctypes.data) == 0
        opened = opened.tolist()                                       # (how fast the words close depends on the order the tiles run in: no two executions agree)
        assert opened[0] > 0 and 0 in opened and not any(opened[opened.index(0):]), opened   # the all-CU stage ran, counted from zero, and ended
        assert all(a >= b for a, b in zip(opened, opened[1:])), opened
        return res + (modes[: min(k, 8)].copy(),)
    cycle(ctx, run, CLAIMS[("large", f)], [(plan, False)], _check_against(batch, want))
    plan.close()


def test_lznt1_header_walk_fallback(oracle, ctx):
    """stored chunks full of 0x33: every offset looks like a chunk header, the verify kernel walks those segments itself"""
    hostile = b"".join(b"\xff\x3f" + b"\x33" * 4096 for _ in range(60))
    text = cases.mixed_buffer()[:100000]
    ctext = oracle.oracle_compress(2, text)[1]
    units = [hostile, ctext + hostile + ctext, hostile[:-1000]]
    caps = [4096 * 60, 2 * len(text) + 4096 * 60, 4096 * 60]
    want = [oracle.oracle_decompress_ex(2, u, c)[:2] for u, c in zip(units, caps)]
    assert want[0][0] == 0 and want[1][0] == 0 and want[2][0] != 0
    batch = PR.layout(units, caps)
    plan = PR.host_plan(ctx, 2, batch, "decode")
    ctx.lib.mscomp_amd_debug_lzd_walked(ctx._h)
    cycle(ctx, lambda: PR.host_execute(plan, batch), CLAIMS[("decode", 2)], [(plan, False)], _check_against(batch, want))
    assert ctx.lib.mscomp_amd_debug_lzd_walked(ctx._h) >= 3
    plan.close()


# ---- device-table plans --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("large", [False, True], ids=["plain", "large_units"])
@pytest.mark.parametrize("kind", ["decode", "size"])
@pytest.mark.parametrize("fmt", list(FMTS))
def test_decode_and_size_dev_plans(oracle, ctx, fmt, kind, large):
    """n_units, in_total_max and out_total_max exactly those of the accepted units; the last unit of the table crosses in_total_max and is
    rejected (MSCOMP_ARG_ERROR) before and after every poison; large_units: with a unit past the thresholds of the optional paths"""
    import ms_compress_amd as m
    f = FMTS[fmt]
    if large and f == 2:
        units, caps, want = _decode_batch(oracle, f, "foreign")      # (LZNT1 has no optional paths: the flag changes nothing)
    elif large:
        units, caps, want = _large_units(oracle, f)
    else:
        units, caps, want = _decode_batch(oracle, f, "streams")
    k = max(range(len(units)), key=lambda i: len(units[i]))           # (a unit with input: it crosses in_total_max)
    units, caps, want = units + [units[k]], caps + [caps[k]], want + [want[k]]
    n = len(units)
    in_max, out_max = sum(len(u) for u in units[:-1]), sum(caps[:-1])
    if kind == "decode":
        plan = m.DevPlan(ctx, f, n, in_max, out_max, large_units=large)
    else:
        plan = m.SizeDevPlan(ctx, f, n, in_max, large_units=large)
    batch = PR.layout(units, caps)
    r = PR.DevRun(plan, len(batch.blob), batch.out_total)
    if kind == "decode":
        check = _check_against(batch, want, rejected={n - 1})
    else:
        def check(res):
            for i, (ws, wb) in enumerate(want[:-1]):
                assert (int(res[1][i]), int(res[0][i])) == (ws, len(wb) if ws == 0 else 0), i
            assert (int(res[1][n - 1]), int(res[0][n - 1]), int(res[3][n - 1])) == (-2, 0, 0)
            assert (res[2] == GUARD).all()
    claims = CLAIMS[("large" if large and f != 2 and kind == "decode" else kind, f)]
    if large and kind == "size" and f == 3:
        claims = claims + ("xps_buf",)
    if not large and kind == "decode":
        claims = tuple(c for c in claims if c != "dz_scr")            # (the token scratch is one of the optional paths)
    cycle(ctx, lambda: r.run(batch), claims, [(plan, True)], check)
    if large and f != 2:
        paths = m.api.plan_paths(plan)
        assert (paths[0] == 2 if f == 3 else True) and (kind == "size" or (paths[1] == 3 and (f == 3 or paths[2] > 0))), paths
    plan.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_compress_dev_plan(oracle, ctx, fmt):
    """n_units, in_total_max and in_unit_max exactly those of the batch; one unit longer than in_unit_max is rejected"""
    import ms_compress_amd as m
    f = FMTS[fmt]
    units = _compress_units()
    _, caps, want = _compress_want(oracle, f)
    longest = max(len(u) for u in units)
    units, want = units + [bytes(longest + 1)], want + [(0, b"")]
    n = len(units)
    plan = m.CompressDevPlan(ctx, f, n, sum(len(u) for u in units[:-1]), longest)
    batch = PR.layout(units, caps + [longest + 600])
    r = PR.DevRun(plan, len(batch.blob), batch.out_total)
    cycle(ctx, lambda: r.run(batch), CLAIMS[("compress", f)], [(plan, True)], _check_against(batch, want, rejected={n - 1}))
    plan.close()


def test_crc_dev_plan_one_long_unit_and_many_short_ones(ctx):
    import torch
    import ms_compress_amd as m
    rs = np.random.RandomState(5)
    mem = rs.randint(0, 256, size=(3 << 20) + 600 * 48, dtype=np.uint8)
    offs = [5] + [(3 << 20) + 48 * k + k % 7 for k in range(600)] + [100]
    lens = [(3 << 20) - 11] + [40] * 600 + [77]                       # the last unit crosses in_total_max: rejected
    n = len(offs)
    plan = m.CrcDevPlan(ctx, n, sum(lens[:-1]))
    d_in, d_off, d_len = torch.from_numpy(mem).cuda(), PR.dt(offs), PR.dt(lens)
    d_crc, d_st = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    want, wst = K.units(mem, offs, lens, sum(lens[:-1]))
    assert not wst[:-1].any() and wst[-1] == -2

    def run():
        d_crc.fill_(0x5A5A5A5A); d_st.fill_(77)
        plan.execute(d_in, d_off, d_len, d_crc, d_st)
        ctx.stream.synchronize()
        return G.u32(d_crc, n), d_st.cpu().numpy()

    def check(res):
        assert (res[0] == want).all() and (res[1] == wst).all()
    cycle(ctx, run, (), [(plan, True)], check)
    rep = m.api.scratch_report(ctx, 0)                                 # the CRC path has no context scratch: its tables are the plan's own
    assert all(c == 0 for _, c, _ in rep.values()) and m.api.scratch_report(plan, 0)["tables"][0] == (2 * n + 1) * 8
    plan.close()


def test_layout_and_compact_dev_and_compact_batch(oracle, ctx):
    """mscomp_amd_plan_layout_dev (and mscomp_amd_layout_dev) -> a compress dev plan -> mscomp_amd_compact_dev, tables from tensors; and mscomp_amd_compact_batch, whose
    table is the one context buffer a compaction has"""
    import torch
    import ms_compress_amd as m
    f = 4
    units, ref = _compress_units(), _compress_want(oracle, f)[0]
    n = len(units)
    blob, in_off, lens, _, _, _ = PR.layout(units, [0] * n)
    d_in, d_ioff, d_ilen = torch.from_numpy(blob).cuda(), PR.dt(in_off), PR.dt(lens)
    h_off, h_cap = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    total = int(m.load_library().mscomp_amd_plan_layout(f, n, lens.ctypes.data, 16, h_off.ctypes.data, h_cap.ctypes.data))
    plan = m.CompressDevPlan(ctx, f, n, int(lens.sum()), int(lens.max()))
    d_off, d_cap = torch.empty(n + 1, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda")
    d_out = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
    d_len, d_st = torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    packed_cap = sum(len(b) for _, b in ref)
    d_packed, d_poff = torch.empty(packed_cap + 64, dtype=torch.uint8, device="cuda"), torch.empty(n + 1, dtype=torch.int64, device="cuda")
    d_off2 = torch.empty(n + 1, dtype=torch.int64, device="cuda")

    def run():
        for t in (d_off, d_off2, d_cap, d_len, d_poff):
            t.fill_(-7)
        d_st.fill_(-9); d_out.fill_(GUARD); d_packed.fill_(GUARD)
        m.api.plan_layout_dev(ctx, f, d_ilen, 16, d_off, d_cap)
        m.api.layout_dev(ctx, d_cap, 16, d_off2)
        plan.execute(d_in, d_ioff, d_ilen, d_out, d_off, d_cap, d_len, d_st)
        m.api.compact_dev(ctx, d_out, d_off, d_len, 1, d_packed, d_poff, packed_cap=packed_cap)
        p2, poff2 = m.api.compact_batch(ctx, h_off, h_cap, d_out, d_len)
        ctx.stream.synchronize()
        return (d_off.cpu().numpy(), d_cap.cpu().numpy(), d_len.cpu().numpy(), d_st.cpu().numpy(), d_out.cpu().numpy(), d_packed.cpu().numpy(),
                d_poff.cpu().numpy(), p2.cpu().numpy()[:packed_cap], poff2.cpu().numpy(), d_off2.cpu().numpy())

    def check(res):
        assert (res[0][:n] == h_off.view(np.int64)).all() and int(res[0][n]) == total and (res[1] == h_cap.view(np.int64)).all()
        assert (res[9] == res[0]).all()                              # layout_dev over the capacities: the same offsets
        assert not res[3].any() and res[2].tolist() == [len(b) for _, b in ref]
        stream = b"".join(b for _, b in ref)
        assert bytes(res[5][:packed_cap]) == stream and (res[5][packed_cap:] == GUARD).all() and int(res[6][n]) == packed_cap
        assert bytes(res[7]) == stream and int(res[8][n]) == packed_cap
    cycle(ctx, run, CLAIMS[("compact",)] + CLAIMS[("compress", f)], [(plan, True)], check)
    plan.close()


# ---- block containers ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(FMTS))
def test_block_container(oracle, ctx, fixture, fmt):
    """B = 4096, the committed blocks fixture: crc, compress, decompress and check on one container whose bounds are the batch's, against
    the models of tests/blocks_model.py and tests/crc_model.py, through the CrcRig of tests/blocks_rig.py; then a decompress from an offset table with a decreasing entry"""
    f, B = FMTS[fmt], 4096
    bufs = G.crc_bufs(fixture, f, B)
    n, lens, total = len(bufs), [len(b) for b in bufs], sum(len(b) for b in bufs)
    rig = G.CrcRig(ctx, f, B, n, total)
    rig.load(bufs)
    rig.set_out(lens)
    mp, mf, mo, ms = M.model_compress(oracle, f, bufs, B, total, total)
    j = int(mf[8])
    bad = mo.copy(); bad[j + 1] = bad[j] - 1
    d_bad = G.d64(bad, rig.dev)
    # once, unpoisoned: everything against its model
    rig.check_crc()
    rig.check_compress(oracle, packed_cap=total)
    st, st2, _ = rig.decode_and_check()
    assert st == [0] * n and st2 == [0] * n
    _, hurt = rig.check_decompress(oracle, (mp, len(mp), mf, bad), boff=d_bad)
    assert hurt[8] != 0 and hurt[0] == 0
    rig.compress(packed_cap=total)
    rig.ctx.stream.synchronize()

    def run_crc():
        rig.crc()
        rig.ctx.stream.synchronize()
        return G.u32(rig.d_bcrc, rig.nbmax).copy(), G.u32(rig.d_rcrc, n).copy(), rig.d_kst.cpu().numpy()

    def run_compress():
        rig.compress(packed_cap=total)
        return rig.compressed()

    def run_decompress():
        return rig.decompress(packed_len=len(mp))

    def run_check():                                                   # (on what run_decompress left in d_out: caller memory, not scratch)
        rig.d_olen.fill_(-1); rig.d_dst.fill_(0)
        rig.bk.check(rig.d_out, rig.d_ooff, rig.d_len, rig.d_first, rig.d_bcrc, rig.d_olen, rig.d_dst)
        rig.ctx.stream.synchronize()
        return rig.d_olen.cpu().numpy(), rig.d_dst.cpu().numpy(), rig.d_out.cpu().numpy()

    def run_damaged():
        return rig.decompress(packed_len=len(mp), boff=d_bad)
    claims = tuple(sorted(set(CLAIMS[("compress", f)] + CLAIMS[("decode", f)]) - {"dz_scr"}))   # (blocks of 4096 bytes: one chunk each)
    cycle(ctx, [run_crc, run_compress, run_decompress, run_check, run_damaged], claims, [(rig.bk, True)])
    rig.close()


# ---- readers, writers, splicers, dedupers ------------------------------------------------------------------------------------------------------
# The source containers and the operation rigs are those of tests/blocks_rig.py (Container and what is built on it), made once on the
# session's context; the object under test lives on the case's fresh context, with bounds equal to its call. Every execution, poisoned or
# not, is compared with the operation's model by that rig's own check.
B4 = 4096


def _flat(*parts):
    """what a check returned, as arrays"""
    out = []
    for p in parts:
        for k in sorted(p):
            if k != "d" and p[k] is not None:
                out.append(np.asarray(p[k]))
    return out


@pytest.fixture(scope="module")
def sources(gpu_ctx):
    made = {}

    def get(kind, fmt):
        if (kind, fmt) not in made:
            made[(kind, fmt)] = {"read": lambda: G.ReadRig.make(gpu_ctx, FMTS[fmt], B4, R.buffers(B4)), "splice": lambda: G.Splices(gpu_ctx, FMTS[fmt], B4),
                                 "extents": lambda: G.Extents(gpu_ctx, FMTS[fmt], B4)}[kind]()
        return made[(kind, fmt)]
    yield get
    for v in made.values():
        v.close()


def _falling(rig):
    """the offset table with a decreasing entry in the resource of raw and compressed blocks (the `damage` tests of the owning modules)"""
    j = int(rig.first[G.MIXED])
    bad = rig.off.copy(); bad[j + 2] = bad[j + 1] - np.uint64(1)
    return bad


@pytest.mark.parametrize("fmt", list(FMTS))
def test_block_reader(oracle, ctx, sources, fmt):
    import torch
    import ms_compress_amd as m
    rig = sources("read", fmt)
    reqs = G.geometry(rig)
    reqs = [reqs[i] for i in np.random.RandomState(3).permutation(len(reqs))]
    bmax = rig.budget(reqs)
    rd = m.BlockReader(ctx, rig.fmt, B4, rig.n, rig.nbt, len(reqs), bmax)
    d_out = torch.empty(rig.layout(rig.wants(reqs))[1], dtype=torch.uint8, device=rig.dev)
    bad = _falling(rig)

    def run():
        mo, ms, mc = rig.check(oracle, reqs, blocks_max=bmax, crc=True, reader=rd, d_out=d_out)
        assert ms == [0] * len(reqs) and mo == G.slices(rig, reqs)
        return np.array(ms), np.array(list(mc)), np.frombuffer(b"".join(mo), np.uint8)

    def run_damaged():
        mo, ms, mc = rig.check(oracle, reqs, blocks_max=bmax, boff=bad, reader=rd, d_out=d_out)
        assert M.DATA in ms and 0 in ms
        return np.array(ms), np.array(list(mc)), np.frombuffer(b"".join(o for o in mo if o), np.uint8)
    claims = tuple(c for c in CLAIMS[("decode", FMTS[fmt])] if c != "dz_scr")
    cycle(ctx, [run, run_damaged], claims, [(rd, True)])
    rd.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_block_writer_write_and_resize(oracle, ctx, sources, fmt):
    import ms_compress_amd as m
    rig = sources("read", fmt)
    ws = G.Writes(rig)
    B, L = B4, rig.lens[G.MIXED]
    reqs = [(G.MIXED, 0, 10), (G.MIXED, B // 2, 100), (G.MIXED, B - 3, 10), (G.MIXED5, B - 1, B + 2), (G.MIXED, L - 1, 1), (G.TEXT, B, B),
            (G.ZEROS5, 0, G.ALL), (G.TEXT, 2 * B + 5, G.ALL), (G.RANDOM1, 0, B), (G.MIXED5, 3 * B, B)]
    srcs = G.sources(rig, reqs, 21, [1, 2, 1, 2, 1, 1, 2, 0, 0, 1])
    bmax = rig.budget(reqs)
    wr = m.BlockWriter(ctx, rig.fmt, B, rig.n, rig.nbt, len(reqs), bmax)
    at = G.flip(oracle, rig, int(rig.first[G.MIXED]) + 1, B, False)     # a broken stream in the compressed block: refused with and without checksums
    hurt = bytearray(rig.packed); hurt[at] ^= 0x01
    d_hurt = rig.d_packed.clone(); d_hurt[at] = int(hurt[at])

    def run():
        mo, got = ws.check(oracle, reqs, srcs, blocks_max=bmax, writer=wr)
        assert mo["status"] == [0] * len(reqs) and mo["res_status"] == [0] * rig.n
        return _flat(got)

    def run_damaged():
        mo, got = ws.check(oracle, reqs, srcs, blocks_max=bmax, writer=wr, packed=d_hurt, model_packed=bytes(hurt))
        assert M.DATA in mo["status"] and 0 in mo["status"]
        return _flat(got)
    f = FMTS[fmt]
    claims = tuple(sorted(set(CLAIMS[("compress", f)] + CLAIMS[("decode", f)]) - {"dz_scr"}))
    cycle(ctx, [run, run_damaged], claims, [(wr, True)])
    wr.close()
    # resize, on a writer of its own: a table of SPARE more rows, no requests, G.BUDGET blocks
    zs = G.Resizes.__new__(G.Resizes)                               # (Resizes without its second container: only run / check are used)
    zs.rig = rig
    nb = int(rig.first[-1])
    zs.nbt = nb + G.SPARE
    zs.off = np.concatenate([rig.off[: nb + 1], np.full(G.SPARE, rig.off[nb], dtype=np.uint64)])
    zs.crc = np.concatenate([rig.crc[:nb], np.zeros(G.SPARE, dtype=np.uint32)])
    zs.d_boff, zs.d_crc = G.d64(zs.off, rig.dev), G.i32(zs.crc, rig.dev)
    zs.room = rig.total + G.BUDGET * B
    want = list(rig.lens)
    want[G.MIXED] = B + 100; want[G.TEXT] = rig.lens[G.TEXT] + 2 * B + 9; want[G.ZEROS5] = 0; want[G.RANDOM1] = B // 2
    wz = m.BlockWriter(ctx, rig.fmt, B, rig.n, zs.nbt, 0, G.BUDGET)
    bad = zs.off.copy(); j = int(rig.first[G.MIXED]); bad[j + 2] = bad[j + 1] - np.uint64(1)

    def run_resize():
        mo, got = zs.check(oracle, want, read_back=False, writer=wz)
        assert mo["res_status"] == [0] * rig.n and mo["new_len"] == want
        return _flat(got)

    def run_resize_damaged():
        mo, got = zs.check(oracle, want, read_back=False, writer=wz, boff=bad)
        assert any(mo["res_status"]) and 0 in mo["res_status"]
        return _flat(got)
    cycle(ctx, [run_resize, run_resize_damaged], claims, [(wz, True)])
    wz.close()


def test_block_splicer_by_picks_and_by_extents(ctx, sources):
    import ms_compress_amd as m
    import extents_model as X
    from extents_model import healthy_lists
    from splice_model import pick_lists
    zs = sources("splice", "lznt1")
    picks = pick_lists(zs.rig[0].n)[2]                             # by turns from the second container and the first
    nbt = zs.table_for(picks)
    sp = m.BlockSplicer(ctx, B4, 2, len(picks), nbt)
    hurt = [zs.rig[0].edited(off=_falling(zs.rig[0])), zs.src[1]]

    def run():
        mo, got = zs.check(picks, nbt, splicer=sp)
        assert mo["status"] == [0] * len(picks)
        return _flat(got)

    def run_damaged():
        return _flat(zs.check(picks, nbt, srcs=hurt, splicer=sp)[1])
    cycle(ctx, [run, run_damaged], (), [(sp, True)])
    sp.close()
    xs = sources("extents", "lznt1")
    resources = healthy_lists(xs.rig[0].n)["insert"]
    ef, ext = X.flat(resources)
    nbt = xs.table_for(resources)
    sx = m.BlockSplicer.for_extents(ctx, B4, 2, len(resources), len(ext), nbt)
    hurt_x = [xs.rig[0].edited(off=_falling(xs.rig[0])), xs.src[1]]

    def run_extents(srcs):
        got = xs.run(sx, srcs, ef, ext, xs.outputs(len(resources), nbt), xs.room)
        mo = X.model_splice_extents([s.model() for s in srcs], ef, ext, B4, len(ext), nbt, xs.room, with_crc=True)
        xs.compare(got, mo, len(resources), nbt, True)
        return _flat(got)
    cycle(ctx, [lambda: run_extents(xs.src), lambda: run_extents(hurt_x)], (), [(sx, True)])
    sx.close()


def test_block_deduper(ctx, sources):
    import ms_compress_amd as m
    zs = sources("splice", "lznt1")
    n, rows = sum(s.n for s in zs.src), sum(s.nbt for s in zs.src)
    dd = m.BlockDeduper(ctx, B4, 2, n, rows)
    outs = G.dedup_outs(zs.dev, n)
    hurt = [zs.rig[0].edited(off=_falling(zs.rig[0])), zs.src[1]]

    def run():
        mo, _ = G.check_dedup(zs, zs.src, deduper=dd, outs=outs)
        assert mo["status"] == [0] * n and mo["count"][0] == zs.rig[0].n - 1
        return _flat(mo)

    def run_damaged():
        return _flat(G.check_dedup(zs, hurt, deduper=dd, outs=outs)[0])
    cycle(ctx, [run, run_damaged], (), [(dd, True)])
    dd.close()


# ---- one-shot host-pointer calls -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(FMTS))
def test_one_shot_host_pointers(oracle, fmt):
    """ms_compress and ms_decompress on 150 000 bytes of the mixed buffer from this thread, whose one-shot context is the NULL target"""
    import ms_compress_amd as m
    f = FMTS[fmt]
    data = cases.mixed_buffer()[60000:210000]
    want = oracle.oracle_compress(f, data)[1]

    def run():
        comp = m.compress(f, data)
        back = m.decompress(f, comp, len(data))
        with pytest.raises(m.MSCompError) as e:
            m.decompress(f, comp[: len(comp) // 2], len(data))
        return (np.frombuffer(comp, np.uint8), np.frombuffer(back, np.uint8), np.array([e.value.status]))

    def check(res):
        assert bytes(res[0]) == want and bytes(res[1]) == data
        assert int(res[2][0]) == oracle.oracle_decompress_ex(f, want[: len(want) // 2], len(data))[0] != 0
    def body():                                                        # in a thread of its own: a fresh one-shot context, whose `asked` is this case's
        assert m.api.scratch_poison(None, 0, slack_only=True) == -1   # (none before the thread's first call)
        cycle(None, run, CLAIMS[("one_shot",)], [], check)
    failure = []

    def guarded():
        try:
            body()
        except BaseException as e:                                     # (an assertion of the thread is the test's)
            failure.append(e)
    import threading
    t = threading.Thread(target=guarded)
    t.start()
    t.join()
    if failure:
        raise failure[0]


# ---- the wrappers' order of destruction -------------------------------------------------------------------------------------------------------
def test_closing_a_context_destroys_what_lives_in_it_first(oracle):
    """mscomp_amd_plan_destroy reads the plan's context: Context.close() destroys the plans and block objects that are still open before the
    context, their handles are cleared, closing them afterwards does nothing, and the next context works"""
    import ms_compress_amd as m
    c = m.Context()
    off, ln = np.array([0, 16], np.uint64), np.array([10, 10], np.uint64)
    objs = [m.Plan(c, 2, off, ln, off, np.array([20, 20], np.uint64)), m.DevPlan(c, 3, 2, 64, 64), m.BlockContainer(c, 4, 4096, 2, 8192),
            m.BlockReader(c, 2, 4096, 2, 4, 1, 2), m.BlockSplicer(c, 4096, 1, 2, 4), m.BlockDeduper(c, 4096, 1, 2, 4)]
    gone = m.Plan(c, 2, off, ln, off, ln, decompress=True)
    gone.close()                                                       # (closed by hand: not touched again)
    assert all(o._h for o in objs) and not gone._h and len(c._handles) == len(objs) + 1
    c.close()
    assert not c._h and not any(o._h for o in objs)
    for o in objs + [gone]:
        o.close()
    c.close()
    data = cases.mixed_buffer()[:30000]
    again = m.Context()
    got, st = m.compress_units(2, [data], ctx=again)
    assert st == [0] and got[0] == oracle.oracle_compress(2, data)[1]
    again.close()


# ---- the cases together ----------------------------------------------------------------------------------------------------------------------
def test_every_context_buffer_is_claimed_by_a_case(request):
    """every buffer of a context is among the claims of the cases, every entry of CLAIMS is used by a case of this file, and -- when the
    whole module ran, which is how the suite runs it -- the buffers the cases have asserted from their reports (cycle) are all of them"""
    import inspect
    import re
    import sys
    import ms_compress_amd as m
    names = set(m.api.scratch_names())
    claimed = set()
    for v in CLAIMS.values():
        claimed |= set(v)
    assert claimed == names, (sorted(names - claimed), sorted(claimed - names))
    src = inspect.getsource(sys.modules[__name__])
    body = src[src.index("_memo = {}"):]
    for key in CLAIMS:                                                 # CLAIMS[("compress", f)], CLAIMS[(kind, f)], CLAIMS[("compact",)]: the kind is named in a case
        assert re.search(r'CLAIMS\[\(\s*"%s"' % key[0], body) or (key[0] in ("decode", "size") and "CLAIMS[(kind, f)]" in body), key
    cfg = request.config
    whole = not cfg.getoption("keyword") and not any("::" in a for a in cfg.args) and not cfg.getoption("lf", False)
    mine = [i for i in request.session.items if i.fspath == request.node.fspath]
    if whole and request.session.testsfailed == 0 and mine and mine[-1] is request.node:
        assert ASSERTED == names, sorted(names - ASSERTED)
