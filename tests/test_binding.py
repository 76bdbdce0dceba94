"""CPU, no library and no device: the Python binding held to include/mscomp_amd.h. api.SIGNATURES against every prototype of the header --
names, argument counts, pointer against pointer, the exact scalar widths, return types, the two structures --, and every wrapper that takes
d_* tensors against the header's parameter names: called over a library that only records, each tensor must arrive at the position the
header gives its name."""
import ctypes as C
import inspect
import re

import abi_rig as R

SYMBOL = r"\b((?:ms|lznt1|xpress|xpress_huff|mscomp_amd)_[a-z0-9_]+)\s*\("        # a declared function's name, as tests/test_abi.py finds them


def _code():
    """the header without comments and preprocessor lines, on one line"""
    txt = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", " ", R.header(), flags=re.S))
    return " ".join(re.sub(r"^\s*#.*$", "", txt, flags=re.M).split())


def _prototypes():
    """{name: (return type, [(type, parameter name), ...])} of every ``ret name(params);`` of the header, in its order; a type keeps its
    '*'s, and a parameter declared ``t x[n]`` has the type ``t*``"""
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ *]*?)" + SYMBOL + r"([^()]*)\)\s*;", _code()):
        args = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            t, pname, arr = re.fullmatch(r"\s*(.*?)\s*\b([A-Za-z_][A-Za-z0-9_]*)\s*(\[\d*\])?\s*", p).groups()
            args.append((" ".join(t.split()) + ("*" if arr else ""), pname))
        assert name not in out, name
        out[name] = (" ".join(ret.split()), args)
    return out


def _struct_fields(name):
    """[(type, field name), ...] of ``typedef struct name { ... } name;`` in the header, in its order"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _code()).group(1)
    out = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        t, names = re.fullmatch(r"(.*?[\s*])([A-Za-z_][A-Za-z0-9_]*(?:\s*,\s*[A-Za-z_][A-Za-z0-9_]*)*)", decl).groups()
        out += [(" ".join(t.split()), n.strip()) for n in names.split(",")]
    return out


SCALARS = {"int": "i", "MSCompFormat": "i", "MSCompStatus": "i", "MSCompFlush": "i", "size_t": "z", "uint64_t": "q", "uint32_t": "u"}
# a typed pointer code and what it must point to; "v" stands for any pointer, "H" for any pointer to pointers
POINTEES = {"U": "uint32_t*", "Q": "uint64_t*", "Z": "size_t*", "B": "const mscomp_amd_blocks_view*", "R": "mscomp_amd_scratch_rec*", "S": "const char**"}


def _codes(name):
    """the codes of api.SIGNATURES[name], repeats written out: (return code, argument codes)"""
    import ms_compress_amd as m
    ret, _, args = m.api.SIGNATURES[name].partition(":")
    return ret, "".join(c * int(n or 1) for c, n in re.findall(r"(\D)(\d*)", args))


def test_the_type_codes_are_the_ctypes_classes_they_stand_for():
    import ms_compress_amd as m
    api = m.api
    assert api._CODES == {"i": C.c_int, "z": C.c_size_t, "q": C.c_uint64, "u": C.c_uint32, "-": None, "s": C.c_char_p, "v": C.c_void_p,
                          "H": C.POINTER(C.c_void_p), "B": C.POINTER(api.BlocksView), "R": C.POINTER(api.ScratchRec), "U": C.POINTER(C.c_uint32),
                          "Q": C.POINTER(C.c_uint64), "S": C.POINTER(C.c_char_p), "Z": C.POINTER(C.c_size_t)}
    assert api.signature("mscomp_amd_writer_write") == (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_void_p] * 8 + [C.c_uint64] + [C.c_void_p] * 5)
    assert api.signature("mscomp_amd_version") == (C.c_char_p, []) and api.signature("mscomp_amd_ctx_destroy") == (None, [C.c_void_p])
    assert api.EXPORTS == list(api.SIGNATURES)


def test_every_signature_is_the_headers_prototype():
    import ms_compress_amd as m
    protos = _prototypes()
    assert len(protos) == len(m.api.EXPORTS) == 135
    assert sorted(protos) == sorted(set(re.findall(SYMBOL, _code())))          # no declared name escaped the prototype parser
    assert list(protos) == m.api.EXPORTS                                          # the table is kept in the header's order
    for name, (ret, params) in protos.items():
        rcode, acodes = _codes(name)
        assert rcode == {"void": "-", "const char*": "s"}.get(ret) or rcode == SCALARS[ret], (name, ret, rcode)
        assert len(acodes) == len(params), (name, len(acodes), len(params))
        for code, (ctype, pname) in zip(acodes, params):
            if "*" not in ctype:
                assert code == SCALARS[ctype], (name, pname, ctype, code)
            elif code == "H":
                assert ctype.count("*") == 2, (name, pname, ctype, code)
            else:
                assert code == "v" or POINTEES[code] == ctype, (name, pname, ctype, code)


def test_the_structures_have_the_headers_fields():
    import ms_compress_amd as m
    for cls, name in ((m.api.BlocksView, "mscomp_amd_blocks_view"), (m.api.ScratchRec, "mscomp_amd_scratch_rec")):
        want = [(f, {"uint64_t": C.c_uint64, "const char*": C.c_char_p}.get(t, C.c_void_p)) for t, f in _struct_fields(name)]
        assert all("*" in t or t == "uint64_t" for t, _ in _struct_fields(name))
        assert [(f, t) for f, t in cls._fields_] == want, name


class _Lib:
    """stands in for the library: records every call as (export, arguments) and answers 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, export):
        if export.startswith("__"):
            raise AttributeError(export)
        return lambda *args: self.calls.append((export, args)) or 0


class _Unbound:
    """stands in for a freshly opened library: one plain object per function asked for"""

    def __init__(self):
        self.functions = {}

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return self.functions.setdefault(name, type("Function", (), {})())


def test_load_library_binds_every_entry(monkeypatch):
    import torch  # noqa: F401  (load_library imports it, and it opens its own libraries through ctypes.CDLL)
    import ms_compress_amd as m
    lib = _Unbound()
    monkeypatch.setattr(m.api._abi, "_lib", None)                # (the loader's own module: api only imports its names)
    monkeypatch.setattr(m.api._abi, "LIB_PATH", __file__)
    monkeypatch.setattr(C, "CDLL", lambda path: lib)
    assert m.api.load_library() is lib
    assert sorted(lib.functions) == sorted(m.api.EXPORTS)
    for name, f in lib.functions.items():
        assert (f.restype, f.argtypes) == m.api.signature(name), name


class _Tensor:
    """a tensor as the wrappers use one: an address and a size"""

    def __init__(self, address):
        self.address = address

    def data_ptr(self):
        return self.address

    def numel(self):
        return 1 << 40


class _Ctx:
    def __init__(self):
        self.lib, self._h, self.device = _Lib(), C.c_void_p(0xC0), 0


# header pointers that no parameter of their wrapper shares a name with: {wrapper: ({header name: the wrapper's name, or None}, reason)}
UNSHARED = {
    "plan_layout_dev": ({"d_out_off": "d_off", "d_out_cap": "d_cap"}, "the wrapper names the two results as layout_dev names its one"),
    "compact_batch": ({"d_packed": None, "d_packed_off": None}, "the wrapper allocates both results and returns them"),
    "BlockDeduper.repair": ({"d_verdict": None}, "d_verdicts, one tensor per source, goes as an array of their addresses"),
}


def _arguments(fn, skip):
    """one distinct stand-in per parameter of ``fn`` behind the first ``skip``: a tensor for d_*, source tuples of tensors for the containers,
    a small integer for the rest"""
    given, address = {}, iter(range(0x1000, 0x100000, 0x100))
    source = lambda: tuple(_Tensor(next(address)) for _ in range(5)) + (None,)
    for k, name in enumerate(list(inspect.signature(fn).parameters)[skip:]):
        if name == "d_verdicts":
            given[name] = [_Tensor(next(address))]
        elif name.startswith("d_"):
            given[name] = _Tensor(next(address))
        elif name in ("sources", "stores"):
            given[name] = [source()]
        elif name in ("source", "store", "base", "new"):
            given[name] = source()
        else:
            given[name] = 3 + k                                 # (packed_len, new_cap, align, ...: all within a tensor's numel())
    return given


def _check_calls(who, calls, given):
    """every recorded call has the header's argument count, and every header parameter that ``given`` has too -- by its own name, or by the
    one UNSHARED gives -- got that value at its position. Returns the pointers checked."""
    renamed = UNSHARED.get(who, ({}, ""))[0]
    pointers = 0
    assert calls, who + " called nothing"
    for export, args in calls:
        params = _prototypes()[export][1]
        assert len(args) == len(params), (who, export, len(args), len(params))
        unshared = {p for t, p in params if p.startswith("d_") and "*" in t and p not in given}
        assert unshared == set(renamed), (who, export, sorted(unshared))
        for got, (ctype, pname) in zip(args, params):
            want = given.get(renamed.get(pname) or pname)
            if isinstance(want, _Tensor):
                assert isinstance(got, C.c_void_p) and got.value == want.address, (who, export, pname)
                pointers += 1
            elif isinstance(want, int):
                assert got == want, (who, export, pname)
    return pointers


def _handle_classes(cls):
    return [cls] + [c for sub in cls.__subclasses__() for c in _handle_classes(sub)]


def test_every_method_passes_its_tensors_where_the_header_names_them():
    import ms_compress_amd as m
    methods = [(cls, name, fn) for cls in _handle_classes(m.api._Handle) for name, fn in vars(cls).items()
               if inspect.isfunction(fn) and any(p.startswith("d_") for p in inspect.signature(fn).parameters)]
    pointers = 0
    for cls, name, fn in methods:
        obj = cls.__new__(cls)
        obj.ctx, obj._h, obj.n_src = _Ctx(), C.c_void_p(0xB0), 1
        given = _arguments(fn, 1)
        fn(obj, **given)
        pointers += _check_calls("%s.%s" % (cls.__name__, name), list(obj.ctx.lib.calls), given)
    assert len(methods) >= 26 and pointers >= 214, (len(methods), pointers)


def test_the_module_level_calls_pass_their_tensors_where_the_header_names_them():
    import ms_compress_amd as m
    for fn in (m.api.res_crc_dev, m.api.layout_dev, m.api.plan_layout_dev, m.api.compact_dev):     # (given every tensor they allocate nothing)
        ctx = _Ctx()
        given = _arguments(fn, 1)
        fn(ctx, **given)
        assert _check_calls(fn.__name__, ctx.lib.calls, given) == sum(isinstance(v, _Tensor) for v in given.values()), fn.__name__
    # compact_batch allocates its results: by its parameters alone
    params = _prototypes()["mscomp_amd_compact_batch"][1]
    assert {p for _, p in params if p.startswith("d_")} - set(inspect.signature(m.api.compact_batch).parameters) == set(UNSHARED["compact_batch"][0])
    assert len(UNSHARED) <= 3 and sum(len(names) for names, _ in UNSHARED.values()) <= 5
