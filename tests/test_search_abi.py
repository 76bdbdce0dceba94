"""CPU, no device: the block searchers' C ABI (include/mscomp_amd_search.h) and its binding (ms_compress_amd/search.py). The library exports
the four symbols; search.SIGNATURES is held to the new header prototype by prototype, with the parser and the rules tests/test_binding.py
holds api.SIGNATURES to the old one with; BlockSearcher.search passes every tensor where the header names it; every creation error is
answered before a device is touched; and the old header keeps its 135 prototypes and does not know the new names."""
import ctypes as C
import inspect
import os
import re

import abi_rig as R
import test_binding as TB

SEARCH_HEADER = os.path.join(os.path.dirname(R.HEADER), "mscomp_amd_search.h")
NAMES = ["mscomp_amd_searcher_create", "mscomp_amd_searcher_destroy", "mscomp_amd_searcher_search", "mscomp_amd_searcher_counts"]
BIG = 0x7FFFFFF1                                                  # one above the largest count


def _search_prototypes(monkeypatch):
    """test_binding's prototype parser over the new header"""
    text = open(SEARCH_HEADER).read()
    monkeypatch.setattr(R, "header", lambda: text)
    return TB._prototypes()


def test_the_library_exports_the_four_symbols():
    import ms_compress_amd as m
    lib = m.load_library()
    assert m.search.EXPORTS == NAMES
    for s in NAMES:
        assert hasattr(lib, s), "libmscomp_amd.so does not export " + s
    lib = m.search.bind(lib)
    for s in NAMES:
        f = getattr(lib, s)
        assert (f.restype, f.argtypes) == m.search.signature(s), s
    assert m.BlockSearcher is m.search.BlockSearcher and m.blocks_search is m.search.blocks_search
    assert not issubclass(m.BlockSearcher, m.api._Handle)          # composed, not derived: the old header's walk over the handle classes does not meet it


def test_every_signature_is_the_new_headers_prototype(monkeypatch):
    import ms_compress_amd as m
    protos = _search_prototypes(monkeypatch)
    assert list(protos) == m.search.EXPORTS == NAMES
    assert sorted(protos) == sorted(set(re.findall(TB.SYMBOL, TB._code())))        # no declared name escaped the parser
    for name, (ret, params) in protos.items():
        rcode, _, args = m.search.SIGNATURES[name].partition(":")
        acodes = "".join(c * int(n or 1) for c, n in re.findall(r"(\D)(\d*)", args))
        assert rcode == {"void": "-", "const char*": "s"}.get(ret) or rcode == TB.SCALARS[ret], (name, ret, rcode)
        assert len(acodes) == len(params), (name, len(acodes), len(params))
        for code, (ctype, pname) in zip(acodes, params):
            if "*" not in ctype:
                assert code == TB.SCALARS[ctype], (name, pname, ctype, code)
            elif code == "H":
                assert ctype.count("*") == 2, (name, pname, ctype, code)
            else:
                assert code == "v" or TB.POINTEES[code] == ctype, (name, pname, ctype, code)
    text = open(SEARCH_HEADER).read()
    assert re.search(r"#define MSCOMP_AMD_SEARCH_PAT_MAX %du\b" % m.MSCOMP_AMD_SEARCH_PAT_MAX, text)
    assert re.search(r"#define MSCOMP_AMD_SEARCH_LEN_MAX %du\b" % m.MSCOMP_AMD_SEARCH_LEN_MAX, text)
    assert '#include "mscomp_amd.h"' in text


def test_search_passes_every_tensor_where_the_header_names_it(monkeypatch):
    import ms_compress_amd as m
    _search_prototypes(monkeypatch)
    fn = m.BlockSearcher.search
    obj = m.BlockSearcher.__new__(m.BlockSearcher)
    obj.ctx, obj._h = TB._Ctx(), C.c_void_p(0xB0)
    given = TB._arguments(fn, 1)
    header_names = [p for _, p in TB._prototypes()["mscomp_amd_searcher_search"][1]]
    assert list(inspect.signature(fn).parameters)[1:] == header_names[1:]      # the same names at the same positions
    fn(obj, **given)
    calls = list(obj.ctx.lib.calls)
    assert [c[0] for c in calls] == ["mscomp_amd_searcher_search"] and calls[0][1][0].value == 0xB0
    assert TB._check_calls("BlockSearcher.search", calls, given) == 13
    obj._h = C.c_void_p()                                          # (nothing to destroy)


def test_create_argument_errors_without_gpu():
    import ms_compress_amd as m
    lib = m.search.bind(m.load_library())
    create = lib.mscomp_amd_searcher_create
    ctx = C.c_void_p(8)                                            # never dereferenced: every check below comes before the context is used

    def refused(*args):
        obj = C.c_void_p(123)
        return create(*args, C.byref(obj)) == m.MSCOMP_ARG_ERROR and not obj.value
    good = [ctx, m.MSCOMP_XPRESS, 4096, 4, 16, 8, 32, 3, 16, 100, 0]
    changed = lambda at, v: good[:at] + [v] + good[at + 1:]
    assert refused(*changed(0, None))                              # a null context
    assert create(*good, None) == m.MSCOMP_ARG_ERROR               # a null result
    for fmt in (m.MSCOMP_NONE, 1, 5, -1):
        assert refused(*changed(1, fmt)), fmt
    for bs in (0, 4095, 6144, 2048, 1048576, 0x80000000):
        assert refused(*changed(2, bs)), bs
    for n_pat in (0, 65, 0xFFFFFFFF):
        assert refused(*changed(7, n_pat)), n_pat
    for len_max in (0, 257, 0xFFFFFFFF):
        assert refused(*changed(8, len_max)), len_max
    for at in (3, 4, 5, 6, 9):                                     # n_res, n_blocks_table, n_req, blocks_max, hits_max
        assert refused(*changed(at, BIG)), at
    for flags in (1, 2, 0x80000000):
        assert refused(*changed(10, flags)), flags
    # what a decompress dev plan cannot address is MSCOMP_MEM_ERROR, still before the context is used -- as the reader says it
    obj = C.c_void_p(123)
    assert create(*changed(2, 524288)[:6], 1 << 30, 3, 16, 100, 0, C.byref(obj)) == m.MSCOMP_MEM_ERROR and not obj.value


def test_null_objects():
    import ms_compress_amd as m
    lib = m.search.bind(m.load_library())
    p = C.c_void_p(8)
    assert lib.mscomp_amd_searcher_search(None, p, 0, p, p, p, p, p, p, p, p, p, p, p, p) == m.MSCOMP_ARG_ERROR
    out = (C.c_uint32 * 3)()
    assert lib.mscomp_amd_searcher_counts(None, out) == -1
    lib.mscomp_amd_searcher_destroy(None)                          # a null searcher is nothing to destroy


def test_the_old_header_is_what_it_was():
    import ms_compress_amd as m
    protos = TB._prototypes()
    assert len(protos) == len(m.api.EXPORTS) == 135 and list(protos) == m.api.EXPORTS
    assert "searcher" not in R.header() and not set(NAMES) & set(m.api.SIGNATURES)
