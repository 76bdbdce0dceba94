"""The cases of tests/golden/scratch_asked.json: for each, a fresh context and one plan, created and never executed, and the bytes every
scratch buffer of the two was asked for (mscomp_amd_debug_scratch_report). tools/make_golden_scratch.py records them, tests/
test_gpu_scratch_sizes.py compares: a layout function that drifts from the size its buffer had shows up here, for every buffer at once.

Host plans need tables only, no data. in_len 70 000 is more than one chunk for every codec and, as a decode capacity, more than 64 KiB
(the Xpress+Huffman token scratch is on); n_units 1, 2 and 5 let the (n + 1) / 2 and (n + 2) / 2 paddings fall both ways. Dev plans are
made for 400 000 input bytes (capacities of 1 600 000, compress units of 100 000 at most), those with large units for 2 MiB and 4 MiB and
3 or 5 units: three and four units on each path, an odd and an even unit list."""
import os

import numpy as np

FMTS = {"lznt1": 2, "xpress": 3, "xpress_huff": 4}
NS = (1, 2, 5)
UNIT = 70_000
ENV_PREFIXES = ("MSCOMP_AMD_XPS_", "MSCOMP_AMD_LZG_MAX_MB", "MSCOMP_AMD_XHC_SCR_MAX_MB")   # they resize the optional paths


def env_in_the_way():
    return sorted(k for k in os.environ if k.startswith(ENV_PREFIXES))


def _tables(m, lens, caps):
    lens, caps = np.asarray(lens, dtype=np.uint64), np.asarray(caps, dtype=np.uint64)
    in_off, _ = m.pack_offsets(lens, 16)
    out_off, _ = m.pack_offsets(caps, 16)
    return in_off, lens, out_off, caps


def _host(kind, n):
    def make(m, ctx, f):
        lens = [UNIT] * n
        if kind == "size":
            in_off, lens, _, _ = _tables(m, lens, lens)
            return m.api.SizePlan(ctx, f, in_off, lens)
        caps = lens if kind == "decompress" else [m.max_compressed_size(f, UNIT)] * n
        return m.Plan(ctx, f, *_tables(m, lens, caps), decompress=kind == "decompress")
    return make


def _emit4(m, ctx, f):
    ctx.lib.mscomp_amd_debug_set_xpress_emit(4)                  # the block-per-super-block kernels: wrec and sbrec
    try:
        return _host("compress", 2)(m, ctx, f)
    finally:
        ctx.lib.mscomp_amd_debug_set_xpress_emit(0)


def _lznt1_sa(m, ctx, f):
    ctx.set_lznt1_sa_dict(True)                                  # the suffix-array flavour: no lzrec
    return _host("compress", 2)(m, ctx, f)


def _large_host(m, ctx, f):
    """two units past XPS_MIN_IN and LZG_MIN_CAP and a small one: an odd count of large units, so the unit list is padded"""
    plan = m.Plan(ctx, f, *_tables(m, [600_000, 600_000, 1_000], [1_200_000, 1_200_000, 4_000]), decompress=True)
    paths = m.api.plan_paths(plan)
    assert paths[0] == (2 if f == 3 else 0) and paths[1] == 2 and (paths[2] > 0) == (f == 4), paths   # a case whose path is off tests nothing
    return plan


def _dev(kind, n, large=False):
    def make(m, ctx, f):
        if kind == "compress":
            return m.api.CompressDevPlan(ctx, f, n, 400_000, 100_000)
        i, o = (2 << 20, 4 << 20) if large else (400_000, 1_600_000)
        plan = m.api.SizeDevPlan(ctx, f, n, i, large_units=large) if kind == "size" else m.api.DevPlan(ctx, f, n, i, o, large_units=large)
        return plan
    return make


def cases():
    """(name, format or None, make(m, ctx, f) -> plan)"""
    out = []
    for name, f in FMTS.items():
        for kind in ("compress", "decompress", "size"):
            out += [("host/%s/%s/n%d" % (name, kind, n), f, _host(kind, n)) for n in NS]
            out += [("dev/%s/%s/n%d" % (name, kind, n), f, _dev(kind, n)) for n in NS]
    out += [("mode4/xpress/compress", 3, _emit4), ("mode4/lznt1_sa/compress", 2, _lznt1_sa)]
    for name in ("xpress", "xpress_huff"):
        out.append(("large_host/%s/decompress" % name, FMTS[name], _large_host))
        out += [("dev_large/%s/%s/n%d" % (name, kind, n), FMTS[name], _dev(kind, n, True)) for kind in ("decompress", "size") for n in (3, 5)]
    out += [("crc/n%d" % n, None, lambda m, ctx, f, n=n: m.api.CrcDevPlan(ctx, n, 400_000)) for n in (1, 4)]
    return out


def asked(m, make, f):
    """{buffer name: asked} over a fresh context and the plan `make` creates in it"""
    ctx = m.Context()
    try:
        plan = make(m, ctx, f)
        got = {k: v[0] for k, v in m.api.scratch_report(ctx, 0).items()}
        got.update({k: v[0] for k, v in m.api.scratch_report(plan, 0).items()})
        plan.close()
        return got
    finally:
        ctx.close()
