"""GPU: the decoders, the size query and the device-table plans on streams that no encoder writes (tests/streams.py), against the checker on
every unit and against the compiled reference's answer for every family (the same questions as test_foreign_streams.py), with the paths
they are meant to reach shown to have run: the chunk-parallel Xpress+Huffman walk (and its fall-back to the serial walk), the segment walk
of large Xpress streams, lzglobal.hip for capacities of 1 MiB or more."""
import ctypes as C

import numpy as np
import pytest

import plans_rig as PR
import test_foreign_streams as tf
from plans_rig import FMTS, LZG_MIN_CAP, XPS_MIN_IN
from refanswers import digest

pytestmark = pytest.mark.gpu
XHC_SERIAL, XHC_SPEC = 1, 2


def decode_modes(ctx, n):
    out = np.zeros(max(1, n), np.uint32)
    k = ctx.lib.mscomp_amd_debug_decode_modes(ctx._h, out.ctypes.data, n)
    assert k >= 0
    return out[:min(k, n)], k


def check_batch(oracle, m, ctx, f, units, caps, what):
    """decode a batch on the GPU: status, length and bytes of every unit as the checker's; returns [(status, bytes)]"""
    outs, sts = m.decompress_units(f, units, caps, ctx=ctx)
    res = []
    for i, (u, c, o, s) in enumerate(zip(units, caps, outs, sts)):
        so, oo, _ = oracle.oracle_decompress_ex(f, u, c)
        got = (int(s), o if s == 0 else b"")
        assert got[0] == so and (so != 0 or got[1] == oo), (what, i, len(u), c, got[0], so, len(got[1]), len(oo))
        res.append(got)
    return res


@pytest.mark.parametrize("fmt", list(FMTS))
def test_family_batch_matches_checker_and_reference(oracle, gpu_ctx, fmt):
    """the whole family in one batch at its capacities; Xpress with both decoders"""
    import ms_compress_amd as m
    f = FMTS[fmt]
    fam, _ = tf.family(f)
    _, undefined = tf.checker_results(oracle, f, fam)
    want = tf.reference_answer(oracle, f, fam, undefined)
    units, caps = [s.data for s in fam], [s.cap for s in fam]
    for mode in ((0, 1) if f == 3 else (0,)):
        if f == 3:
            gpu_ctx.lib.mscomp_amd_debug_set_xpress_decoder(mode)
        try:
            res = check_batch(oracle, m, gpu_ctx, f, units, caps, "decoder %d" % mode)
            modes, k = decode_modes(gpu_ctx, len(units))
        finally:
            if f == 3:
                gpu_ctx.lib.mscomp_amd_debug_set_xpress_decoder(0)
        assert digest([r for i, r in enumerate(res) if i not in undefined]) == want, "decoder %d" % mode
        if f == 4:                                                   # every buffer: chunk-parallel or serial; the multi-MB ones as their codes say
            assert k == len(units) and set(modes.tolist()) <= {XHC_SERIAL, XHC_SPEC}
            for i, s in enumerate(fam):
                if "big_complete" in s.tags:
                    assert modes[i] == XHC_SPEC, (i, modes[i])
                if "big_incomplete" in s.tags:
                    assert modes[i] == XHC_SERIAL, (i, modes[i])
            assert sum("big_complete" in s.tags for s in fam) >= 2 and sum("big_incomplete" in s.tags for s in fam) >= 2
        if f == 3 and mode == 0:                                     # the large streams were walked by segments
            big = [i for i, u in enumerate(units) if len(u) >= XPS_MIN_IN]
            assert k == len(big) and big
            for j, i in enumerate(big):
                if fam[i].plain is not None:
                    assert modes[j] == 2, (i, modes[j])


@pytest.mark.parametrize("fmt", list(FMTS))
def test_small_units_and_large_capacities(oracle, gpu_ctx, fmt):
    """the valid streams alone in batches of a few small units, and again with capacities of at least 1 MiB (lzglobal.hip takes those)"""
    import ms_compress_amd as m
    f = FMTS[fmt]
    fam, _ = tf.family(f)
    small = [s for s in fam if len(s.data) < 70000]
    for k in range(0, len(small), 7):
        part = small[k:k + 7]
        check_batch(oracle, m, gpu_ctx, f, [s.data for s in part], [s.cap for s in part], "small batch %d" % k)
    valid = [s for s in fam if s.plain is not None][::2]
    caps = [max(s.cap, LZG_MIN_CAP + (i % 3) * 777) for i, s in enumerate(valid)]
    caps[0] = max(caps[0], 8 << 20)                                  # (one large unit: the all-CU stage pays for the batch)
    res = check_batch(oracle, m, gpu_ctx, f, [s.data for s in valid], caps, "large capacities")
    assert all(r == (0, s.plain) for r, s in zip(res, valid))
    if f != 2:                                                       # lzglobal.hip ran (Xpress and Xpress+Huffman take it)
        opened = np.zeros(64, np.uint32)
        gpu_ctx.lib.mscomp_amd_debug_lzg_open.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        assert gpu_ctx.lib.mscomp_amd_debug_lzg_open(gpu_ctx._h, sum(c + 64 for c in caps), opened.ctypes.data) == 0
        assert opened[0] > 0 and opened[0] != 0xFFFFFFFF


@pytest.mark.parametrize("fmt", list(FMTS))
def test_size_query_agrees_with_the_decoder(oracle, gpu_ctx, fmt):
    """decompressed_sizes at the family's capacities: status and length as the decoder's; every valid stream decodes at capacity `need` and
    not at need - 1"""
    import ms_compress_amd as m
    f = FMTS[fmt]
    fam, _ = tf.family(f)
    units, caps = [s.data for s in fam], [s.cap for s in fam]
    lens, need, st = m.decompressed_sizes(f, units, caps, ctx=gpu_ctx)
    if f != 2:
        modes, k = decode_modes(gpu_ctx, len(units))
        if f == 4:
            assert all(modes[i] == XHC_SPEC for i, s in enumerate(fam) if "big_complete" in s.tags)
            assert all(modes[i] == XHC_SERIAL for i, s in enumerate(fam) if "big_incomplete" in s.tags)
        else:
            assert k == sum(len(u) >= XPS_MIN_IN for u in units) > 0
    for i, (s, c) in enumerate(zip(fam, caps)):
        so, oo, _ = oracle.oracle_decompress_ex(f, s.data, c)
        assert (int(st[i]), int(lens[i])) == (so, len(oo) if so == 0 else 0), (i, sorted(s.tags), int(st[i]), so, int(lens[i]), len(oo))
    ok = [i for i, s in enumerate(fam) if s.plain is not None]
    for i in ok:                                                     # need: the checker decodes there and not one byte below
        assert int(st[i]) == 0 and int(need[i]) <= fam[i].cap, (i, int(st[i]), int(need[i]), fam[i].cap)
        assert oracle.oracle_decompress_ex(f, units[i], int(need[i]))[0] == 0, i
        assert int(need[i]) == 0 or oracle.oracle_decompress_ex(f, units[i], int(need[i]) - 1)[0] != 0, i
    outs, sts = m.decompress_units(f, [units[i] for i in ok], [int(need[i]) for i in ok], ctx=gpu_ctx)
    assert all(s == 0 and o == fam[i].plain for i, o, s in zip(ok, outs, sts))
    some = [i for i in ok if need[i] > 0]
    _, sts = m.decompress_units(f, [units[i] for i in some], [int(need[i]) - 1 for i in some], ctx=gpu_ctx)
    assert all(s != 0 for s in sts)


@pytest.mark.parametrize("fmt", list(FMTS))
def test_device_table_plan_matches_host_plan(oracle, gpu_ctx, fmt):
    import ms_compress_amd as m
    f = FMTS[fmt]
    fam, _ = tf.family(f)
    units, caps = [s.data for s in fam], [s.cap for s in fam]
    batch = PR.layout(units, caps)
    blob, in_off, lens, out_off, caps, out_total = batch
    host = PR.host_run(gpu_ctx, f, batch, "decode")
    r = PR.DevRun(m.DevPlan(gpu_ctx, f, len(units), int(lens.sum()), int(caps.sum())), len(blob), out_total + 4096)
    r.load(batch)
    r.execute()
    dev = r.result()
    PR.same(host, dev, batch)
    for i, s in enumerate(fam):
        if s.plain is not None:
            o = int(out_off[i])
            assert dev[1][i] == 0 and bytes(dev[2][o: o + len(s.plain)]) == s.plain, i


@pytest.mark.parametrize("fmt", list(FMTS))
def test_drop_in_ms_decompress(oracle, gpu_ctx, fmt):
    import ms_compress_amd as m
    f = FMTS[fmt]
    fam, _ = tf.family(f)
    pick = [s for s in fam if s.plain is not None][:4] + [s for s in fam if s.plain is None][:3]
    pick += [s for s in fam if "big" in s.tags or "large_input" in s.tags or "multi_segment" in s.tags][:2]
    for s in pick:
        so, oo, _ = oracle.oracle_decompress_ex(f, s.data, s.cap)
        if so == 0:
            assert m.decompress(f, s.data, s.cap) == oo
        else:
            with pytest.raises(m.MSCompError) as e:
                m.decompress(f, s.data, s.cap)
            assert e.value.status == so
