"""CPU: the salvage and repair models (tests/repair_model.py). The GPU tests compare mscomp_amd_blocks_salvage and
mscomp_amd_deduper_repair with these models array for array, so the models are pinned here: on a healthy container a salvage is a
decompress; the damage recipes reach every verdict, every cause of TABLE, the precedence of TABLE over CRC, raw and compressed blocks
under CRC, lost rows and fully repaired resources -- so that no GPU test passes on all-GOOD tables --; and the header's consequence
holds over the extents model."""
import zlib

import numpy as np
import pytest

import blocks_model as M
import blocks_rig as G
import repair_model as P
from repair_model import GOOD, TABLE, DECODE, CRC, SKIPPED

FMTS = {"lznt1": 2, "xpress": 3, "xpress_huff": 4}
B = 4096


@pytest.fixture(scope="module")
def api():
    import ms_compress_amd                                       # noqa: F401  the models describe this library's calls: no library, no test
    from ms_compress_amd import api
    assert "mscomp_amd_blocks_salvage" in api.EXPORTS and "mscomp_amd_deduper_repair" in api.EXPORTS
    assert (api.MSCOMP_AMD_BLOCK_GOOD, api.MSCOMP_AMD_BLOCK_TABLE, api.MSCOMP_AMD_BLOCK_DECODE, api.MSCOMP_AMD_BLOCK_CRC,
            api.MSCOMP_AMD_BLOCK_SKIPPED) == (GOOD, TABLE, DECODE, CRC, SKIPPED)
    return api


@pytest.fixture(scope="module")
def shapes(oracle):
    made = {}

    def get(fmt):
        if fmt not in made:
            made[fmt] = P.shape_of(oracle, FMTS[fmt], B)
        return made[fmt]
    return get


def salvaged(oracle, s, edits, with_crc=True, only=None):
    return P.model_salvage(oracle, s.fmt, P.source_of(s, edits), B, s.total, edits.get("caps", s.lens), with_crc=with_crc, only=only)


@pytest.mark.parametrize("fmt", list(FMTS))
def test_flip_finds_its_byte_in_text_blocks(api, oracle, shapes, fmt):
    """blocks_rig.flip has a byte of either kind in every text block the recipes damage, for all three formats: no recipe can come up empty"""
    s = shapes(fmt)
    for r, k in ((P.TEXT, 1), (P.TEXT, 2), (P.SHORT_TEXT, 0), (P.TEXT_B1, 0), (P.MIXED5, 1), (P.MIXED5, 3), (P.MIXED, 1)):
        j, e = P.row(s, r, k), P.data_len(s, r, k)
        assert int(s.off[j + 1] - s.off[j]) < e, "a compressed block"
        for decodes in (True, False):
            at = G.flip(oracle, s, j, e, decodes)
            assert int(s.off[j]) <= at < int(s.off[j + 1])


@pytest.mark.parametrize("fmt", list(FMTS))
def test_healthy_salvage_is_a_decompress(api, oracle, shapes, fmt):
    s = shapes(fmt)
    for with_crc in (True, False):
        mo = salvaged(oracle, s, {}, with_crc)
        nb = int(s.first[-1])
        assert (mo["verdict"][:nb] == GOOD).all() and (mo["verdict"][nb:] == SKIPPED).all()
        assert mo["status"] == [0] * s.n and mo["bad"] == [0] * s.n and mo["out_len"] == s.lens and mo["count"] == [nb, 0, 0, 0]
        outs, sts = M.model_decompress(oracle, s.fmt, s.packed, s.plen, s.first, s.off, s.lens, B, s.total, s.lens)
        assert sts == [0] * s.n
        for r, mine in enumerate(mo["rows"]):
            assert b"".join(d for _, d, _ in mine) == outs[r] == s.bufs[r]


@pytest.mark.parametrize("fmt", list(FMTS))
def test_recipes_cover_every_verdict_and_cause(api, oracle, shapes, fmt):
    s = shapes(fmt)
    seen, causes, crc_forms = set(), set(), set()
    for name, recipe in P.RECIPES.items():
        edits = recipe(s, oracle)
        mo = salvaged(oracle, s, edits)
        bare = salvaged(oracle, s, edits, with_crc=False)
        assert any(v in P.BAD for v in mo["verdict"]), (name, "damages nothing")
        assert CRC not in bare["verdict"] and [v if v != CRC else GOOD for v in mo["verdict"]] == list(bare["verdict"]), name
        seen |= set(int(v) for v in mo["verdict"])
        for r, mine in enumerate(mo["rows"]):
            if mine is None:
                assert mo["bad"][r] == 0 and mo["out_len"][r] == 0 and mo["status"][r] in (P.ARG, P.DATA, P.BUF)
                continue
            assert mo["out_len"][r] == int(P.source_of(s, edits)[4][r]), "the length, whatever the rows say"
            assert mo["bad"][r] == sum(1 for v, _, _ in mine if v in P.BAD) and mo["status"][r] == (P.DATA if mo["bad"][r] else 0)
            for k, (v, data, cause) in enumerate(mine):
                causes |= {cause} if v == TABLE else set()
                assert (v == TABLE) == (cause is not None)
                if v in P.BAD:
                    assert data == bytes(len(data)) and len(data) > 0, "a bad row is zeros"
                if v == CRC:
                    crc_forms.add(mo["stored"][P.row(s, r, k)])
        assert mo["count"] == [sum(len(m) for m in mo["rows"] if m), sum(mo["bad"]), mo["count"][2], sum(1 for b in mo["bad"] if b)]
    assert seen == {GOOD, TABLE, DECODE, CRC, SKIPPED}
    assert causes == set(P.CAUSES), causes
    assert crc_forms == {"raw", "compressed"}
    # the precedence: a TABLE row whose CRC word is wrong too stays TABLE
    edits = P.r_table_and_crc(s, oracle)
    j = P.row(s, P.MIXED, 0)
    assert int(edits["crc"][j]) != int(s.crc[j]) and salvaged(oracle, s, edits)["verdict"][j] == TABLE
    # rules 1-3 each refuse a resource of "refused", beside damaged ones
    mo = salvaged(oracle, s, P.r_refused(s, oracle))
    assert {P.ARG, P.DATA, P.BUF} <= set(mo["status"]) and DECODE in mo["verdict"] and CRC in mo["verdict"]


@pytest.mark.parametrize("fmt", list(FMTS))
def test_mask_judges_only_what_it_names(api, oracle, shapes, fmt):
    s = shapes(fmt)
    edits = P.r_everything(s, oracle)
    whole = salvaged(oracle, s, edits)
    nothing = salvaged(oracle, s, edits, only=np.zeros(s.nbt, dtype=np.uint32))
    assert (nothing["verdict"] == SKIPPED).all() and nothing["count"] == [0, 0, 0, 0] and nothing["status"] == [0] * s.n
    assert not P.image_pieces(nothing, [0] * s.n, B)
    masked = salvaged(oracle, s, {}, only=whole["verdict"])        # a healthy mirror, looked at only where the primary is bad
    bad_rows = [j for j, v in enumerate(whole["verdict"]) if v in P.BAD]
    assert [j for j, v in enumerate(masked["verdict"]) if v != SKIPPED] == bad_rows and all(masked["verdict"][j] == GOOD for j in bad_rows)
    assert masked["count"] == [len(bad_rows), 0, 0, 0]


def repair_case(oracle, s, recipes, with_crc=True):
    edits = [r(s, oracle) for r in recipes]
    srcs = [P.source_of(s, e) for e in edits]
    verdicts = [P.model_salvage(oracle, s.fmt, srcs[0], B, s.total, s.lens, with_crc)["verdict"]]
    for e, src in zip(edits[1:], srcs[1:]):
        only = verdicts[0] if src[4] == srcs[0][4] else None
        verdicts.append(P.model_salvage(oracle, s.fmt, src, B, s.total, s.lens, with_crc, only=only)["verdict"])
    return srcs, verdicts


@pytest.mark.parametrize("fmt", list(FMTS))
def test_repair_case_loses_and_mends(api, oracle, shapes, fmt):
    s = shapes(fmt)
    srcs, verdicts = repair_case(oracle, s, P.REPAIR_CASE)
    mo = P.model_repair(srcs, verdicts, B, s.n, int(s.first[-1]))
    look = lambda r, k: mo["choice"][r][k]
    assert look(P.TEXT, 1) == (0, True), "bad in every copy: lost, and the primary's"
    assert look(P.TEXT, 2) == (1, False) and look(P.SHORT_TEXT, 0) == (1, False) and look(P.MIXED5, 1) == (1, False)
    assert look(P.RANDOM3, 1) == (2, False), "the first mirror lacks it too"
    assert look(P.MIXED5, 3) == (0, True), "the only good copy has another length: never a candidate"
    assert look(P.ZEROS5, 4) == (0, True), "a damaged CRC word is in no mirror"
    assert mo["lost"][P.TEXT] == 1 and mo["status"][P.TEXT] == P.DATA
    assert mo["status"][P.RANDOM3] == 0 and mo["fixed"][P.RANDOM3] == 1 and mo["status"][P.SHORT_TEXT] == 0, "fully repaired resources"
    assert mo["count"][:2] == [sum(mo["fixed"]), sum(mo["lost"])] and mo["count"][0] >= 4 and mo["count"][1] == 3 and mo["count"][3] == 3
    assert mo["ext_first"][-1] == len(mo["ext"]) and all(c <= 2 and n >= 1 for c, _, _, n in mo["ext"])
    for r in range(s.n):                                           # the runs are maximal, in order, and cover the resource
        ext = mo["ext"][mo["ext_first"][r]: mo["ext_first"][r + 1]]
        assert [k for _, _, k, _ in ext] == [sum(n for _, _, _, n in ext[:i]) for i in range(len(ext))]
        assert sum(n for _, _, _, n in ext) == (s.lens[r] + B - 1) // B and all(a[0] != b[0] for a, b in zip(ext, ext[1:]))
    got = P.holds_consequence(srcs, mo, B, P.source_of(s))
    assert got["new_len"] == s.lens and np.array_equal(got["first"], s.first), "the primary's shape, lost rows and all"
    # without checksums nothing tells a row that decodes to other bytes: fewer rows are bad, none is CRC
    srcs2, verdicts2 = repair_case(oracle, s, P.REPAIR_CASE, with_crc=False)
    assert not any(CRC in v for v in verdicts2)
    P.holds_consequence(srcs2, P.model_repair(srcs2, verdicts2, B, s.n, int(s.first[-1]), with_crc=False), B, P.source_of(s), with_crc=False)


@pytest.mark.parametrize("fmt", list(FMTS))
def test_mended_container_is_the_undamaged_one(api, oracle, shapes, fmt):
    s = shapes(fmt)
    srcs, verdicts = repair_case(oracle, s, (P.r_mendable, lambda s, o: {}))
    mo = P.model_repair(srcs, verdicts, B, s.n, int(s.first[-1]))
    assert mo["status"] == [0] * s.n and sum(mo["fixed"]) == 6 and sum(mo["lost"]) == 0
    got = P.holds_consequence(srcs, mo, B, P.source_of(s))
    assert got["packed"] == s.packed and int(got["crc"][P.row(s, P.RANDOM3, 1)]) == zlib.crc32(s.bufs[P.RANDOM3][B: 2 * B])
    # the room rule and a resource the primary does not have
    tight = P.model_repair(srcs, verdicts, B, s.n + 1, int(s.first[P.TEXT + 1]) - 1)
    assert tight["status"][P.TEXT] == P.ARG and tight["status"][s.n] == P.ARG and tight["status"][P.MIXED] == 0
    assert all(st == P.ARG for st, L in zip(tight["status"][P.TEXT:s.n], s.lens[P.TEXT:]) if L) and tight["fixed"][P.TEXT] == 0
