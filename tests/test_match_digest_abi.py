"""CPU, no device: the C ABI of match by digest (include/mscomp_amd_match_digest.h) and its binding (ms_compress_amd/match_digest.py). The
library exports the two symbols; match_digest.SIGNATURES is held to the new header prototype by prototype, with the parser and the rules
tests/test_binding.py holds api.SIGNATURES to the old one with; BlockDigestMatcher.match passes every tensor where the header names it;
every creation error is answered in match's order before a context is used; the old header keeps its 135 prototypes and does not know the
new names; and importing the module pulls in no torch."""
import ctypes as C
import os
import re
import subprocess
import sys

import abi_rig as R
import test_binding as TB

NEW_HEADER = os.path.join(os.path.dirname(R.HEADER), "mscomp_amd_match_digest.h")
NAMES = ["mscomp_amd_deduper_create_match_digest", "mscomp_amd_deduper_match_digest"]
BIG = 0x7FFFFFF1                                                  # one above the largest count


def _new_prototypes(monkeypatch):
    """test_binding's prototype parser over the new header"""
    text = open(NEW_HEADER).read()
    monkeypatch.setattr(R, "header", lambda: text)
    return TB._prototypes()


def test_the_library_exports_the_two_symbols():
    import ms_compress_amd as m
    lib = m.load_library()
    assert m.match_digest.EXPORTS == NAMES
    for s in NAMES:
        assert hasattr(lib, s), "libmscomp_amd.so does not export " + s
    lib = m.match_digest.bind(lib)
    for s in NAMES:
        f = getattr(lib, s)
        assert (f.restype, f.argtypes) == m.match_digest.signature(s), s
    assert m.BlockDigestMatcher is m.match_digest.BlockDigestMatcher and m.blocks_match_digest is m.match_digest.blocks_match_digest
    assert m.blocks_match_digest_delta is m.match_digest.blocks_match_digest_delta
    assert not issubclass(m.BlockDigestMatcher, m.api._Handle)     # composed, not derived: the old header's walk over the handle classes does not meet it


def test_every_signature_is_the_new_headers_prototype(monkeypatch):
    import ms_compress_amd as m
    protos = _new_prototypes(monkeypatch)
    assert list(protos) == m.match_digest.EXPORTS == NAMES
    assert sorted(protos) == sorted(set(re.findall(TB.SYMBOL, TB._code())))        # no declared name escaped the parser
    for name, (ret, params) in protos.items():
        rcode, _, args = m.match_digest.SIGNATURES[name].partition(":")
        acodes = "".join(c * int(n or 1) for c, n in re.findall(r"(\D)(\d*)", args))
        assert rcode == TB.SCALARS[ret], (name, ret, rcode)
        assert len(acodes) == len(params), (name, len(acodes), len(params))
        for code, (ctype, pname) in zip(acodes, params):
            if "*" not in ctype:
                assert code == TB.SCALARS[ctype], (name, pname, ctype, code)
            elif code == "H":
                assert ctype.count("*") == 2, (name, pname, ctype, code)
            else:
                assert code == "v" or TB.POINTEES[code] == ctype, (name, pname, ctype, code)
    text = open(NEW_HEADER).read()
    assert '#include "mscomp_amd.h"' in text
    # the creates of match and of match by digest take the same arguments; the call takes match's and the two digest arguments
    monkeypatch.undo()
    base = TB._prototypes()
    assert protos["mscomp_amd_deduper_create_match_digest"] == base["mscomp_amd_deduper_create_match"]
    call, mcall = protos["mscomp_amd_deduper_match_digest"][1], base["mscomp_amd_deduper_match"][1]
    assert [p for p in call if p[1] not in ("d_store_digest", "d_next_digest")] == mcall
    assert [p[1] for p in call][:5] == ["dd", "store", "d_store_digest", "next", "d_next_digest"]


def test_match_passes_every_tensor_where_the_header_names_it(monkeypatch):
    import ms_compress_amd as m
    protos = _new_prototypes(monkeypatch)
    header_names = [p for _, p in protos["mscomp_amd_deduper_match_digest"][1]]

    class Lib:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            return lambda *a: self.calls.append((name, a)) or 0

    class T:
        def __init__(self, at):
            self.at = at

        def data_ptr(self):
            return self.at

    class Ctx:
        lib = Lib()
    obj = m.BlockDigestMatcher.__new__(m.BlockDigestMatcher)
    obj.ctx, obj._h, obj.n_src = Ctx(), C.c_void_p(0xB0), 2
    outs = {name: T(0x1000 * (i + 1)) for i, name in enumerate(header_names[5:])}
    view = lambda k: (None, T(k + 1), T(k + 2), T(k + 3), None, 77, 2, 5)
    cols = [T(0xD000), T(0xD100)]
    m.BlockDigestMatcher.match(obj, [view(0x10), view(0x20)], cols, view(0x30), T(0xD200), **outs)
    (name, args), = obj.ctx.lib.calls
    assert name == "mscomp_amd_deduper_match_digest" and args[0].value == 0xB0
    views = args[1]
    assert [views[i].d_block_first for i in range(3)] == [0x11, 0x21, 0x31] and [views[i].packed_len for i in range(3)] == [77] * 3
    assert all(views[i].d_packed is None and views[i].d_block_crc is None for i in range(3))
    assert list(args[2]) == [0xD000, 0xD100]                       # the stores' columns, a host array of device pointers
    assert C.cast(args[3], C.POINTER(m.BlocksView)).contents.d_block_first == 0x31        # next: the view behind the stores'
    assert [a.value for a in args[4:]] == [0xD200] + [outs[n].at for n in header_names[5:]]
    obj._h = C.c_void_p()                                          # (nothing to destroy)


def test_create_argument_errors_come_in_matchs_order_without_gpu():
    import ms_compress_amd as m
    lib = m.match_digest.bind(m.load_library())
    ctx = C.c_void_p(8)                                            # never dereferenced: every check below comes before the context is used
    good = [ctx, 4096, 2, 10, 100, 40, 0]
    changed = lambda at, v: good[:at] + [v] + good[at + 1:]
    for create in (lib.mscomp_amd_deduper_create_match_digest, lib.mscomp_amd_deduper_create_match):     # the same answers from both

        def refused(*args):
            obj = C.c_void_p(123)
            return create(*args, C.byref(obj)) == m.MSCOMP_ARG_ERROR and not obj.value
        assert create(*good, None) == m.MSCOMP_ARG_ERROR           # a null result
        assert refused(*changed(0, None))                          # a null context
        for flags in (1, 2, 0x80000000):
            assert refused(*changed(6, flags)), flags
        for bs in (0, 4095, 6144, 2048, 1048576, 0x80000000):
            assert refused(*changed(1, bs)), bs
        for n_src in (4, 5, 0xFFFFFFFF):
            assert refused(*changed(2, n_src)), n_src
        assert refused(*changed(3, BIG)) and refused(*changed(4, BIG))
        assert refused(*changed(5, 101))                           # n_blocks_new above n_blocks_total
        assert refused(None, 4095, 4, BIG, BIG, BIG + 1, 1)        # everything wrong at once is still an argument error, *dd cleared


def test_null_objects_and_wrong_kinds_without_gpu():
    import ms_compress_amd as m
    lib = m.match_digest.bind(m.load_library())
    p = C.c_void_p(8)
    assert lib.mscomp_amd_deduper_match_digest(None, None, None, None, p, p, p, p, p, p, p, p) == m.MSCOMP_ARG_ERROR
    lib.mscomp_amd_deduper_destroy(None)                           # a null deduper is nothing to destroy


def test_the_old_header_is_what_it_was():
    import ms_compress_amd as m
    protos = TB._prototypes()
    assert len(protos) == len(m.api.EXPORTS) == 135 and list(protos) == m.api.EXPORTS
    assert "match_digest" not in R.header() and not set(NAMES) & set(m.api.SIGNATURES)


def test_importing_the_module_pulls_in_no_torch():
    """in an interpreter of its own: this one may have imported torch long ago"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); import ms_compress_amd.match_digest as g; "
            "assert 'torch' not in sys.modules, 'torch was imported'; assert g.EXPORTS and g.BlockDigestMatcher") % root
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
