"""CPU, no library and no device: ms_compress_amd/device.py held to include/mscomp_amd.h. A table that is one entry short is an out-of-bounds
write by a kernel, so the entry counts are proven here before anything runs on a GPU: device.sizes() against counts this file states on its
own from the header's text, then the whole layer run over CPU tensors and a library that only records -- every recorded call has the
prototype's argument count, every pointer lies in a tensor with at least the entries the header asks of that parameter, none is null where
the header requires one, every stated byte length fits its tensor --, then the capture guard and the layering."""
import ctypes as C
import re
import weakref

import pytest

import abi_rig as R

SYMBOL = r"\b((?:ms|lznt1|xpress|xpress_huff|mscomp_amd)_[a-z0-9_]+)\s*\("
SHAPES = [(n, total, B) for n in (0, 1, 4) for total in (0, 4095, 4096, 6 * 4096) for B in (4096, 524288)]
NQ, CAP_EACH, SLACK = 3, 100, 64


def _prototypes():
    """{name: [(type, parameter name), ...]} of every prototype of the header, as tests/test_binding.py parses them"""
    txt = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", " ", R.header(), flags=re.S))
    code = " ".join(re.sub(r"^\s*#.*$", "", txt, flags=re.M).split())
    out = {}
    for _, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ *]*?)" + SYMBOL + r"([^()]*)\)\s*;", code):
        args = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            t, pname, arr = re.fullmatch(r"\s*(.*?)\s*\b([A-Za-z_][A-Za-z0-9_]*)\s*(\[\d*\])?\s*", p).groups()
            args.append((" ".join(t.split()) + ("*" if arr else ""), pname))
        out[name] = args
    return out


PROTOS = _prototypes()


# ---- what the header says, stated here and nowhere taken from device.py -------------------------------------------------------------------
def header_counts(n, nb, nq, n_ext):
    """{export: {pointer parameter: entries}} from the header's sections on the container, the reader, the writer, the splicer and diff, for a
    container of n resources and nb = n_blocks_max table rows, nq requests, n_ext extents, n pairs and nb new blocks"""
    con = {"d_block_first": n + 1, "d_block_off": nb + 1, "d_res_len": n, "d_block_crc": nb}
    new = {"d_new_block_first": n + 1, "d_new_block_off": nb + 1, "d_new_block_crc": nb, "d_new_res_len": n}
    req = {"d_req": 3 * nq}
    return {
        "mscomp_amd_blocks_compress": {"d_res_off": n, "d_res_len": n, "d_block_first": n + 1, "d_block_off": nb + 1, "d_status": n},
        "mscomp_amd_blocks_crc": {"d_res_off": n, "d_res_len": n, "d_block_crc": nb, "d_res_crc": n, "d_status": n},
        "mscomp_amd_blocks_decompress": dict(con, d_range=2 * n, d_out_off=n, d_out_cap=n, d_out_len=n, d_status=n),
        "mscomp_amd_blocks_check": dict(con, d_range=2 * n, d_out_off=n, d_out_len=n, d_status=n),
        "mscomp_amd_layout_dev": {"d_cap": n, "d_off": n + 1},
        "mscomp_amd_reader_read": dict(con, **req, d_out_off=nq, d_out_cap=nq, d_out_len=nq, d_status=nq),
        "mscomp_amd_writer_write": dict(con, **req, d_src_off=nq, d_new_block_off=nb + 1, d_new_block_crc=nb, d_written=nq, d_status=nq, d_res_status=n),
        "mscomp_amd_writer_resize": dict(con, **new, d_want_len=n, d_res_status=n),
        "mscomp_amd_splicer_splice": dict(new, d_pick=2 * n, d_status=n),
        "mscomp_amd_splicer_splice_extents": dict(new, d_ext_first=n + 1, d_ext=4 * n_ext, d_status=n),
        "mscomp_amd_deduper_diff": {"d_pair": 2 * n, "d_delta_ext_first": n + 1, "d_delta_ext": 4 * nb, "d_patch_ext_first": n + 1, "d_patch_ext": 4 * nb,
                                    "d_changed": n, "d_count": 4, "d_status": n},
    }


MAY_BE_NULL = {"d_range", "d_res_crc"}                              # "may be NULL" whatever the bounds; the checksum arrays only without checksums
BYTES = {"d_in", "d_data", "d_src", "d_packed", "d_new_packed", "d_out"}
LENGTH_OF = {"packed_len": "d_packed", "packed_cap": "d_packed", "new_cap": "d_new_packed"}


@pytest.mark.parametrize("n,total,B", SHAPES)
def test_sizes_states_the_headers_entry_counts(n, total, B):
    from ms_compress_amd import device
    nb = n + total // B
    h = header_counts(n, nb, NQ, 7)
    new = {"d_new_packed": (total + SLACK, "uint8"), "d_new_block_first": (n + 1, "int64"), "d_new_block_off": (nb + 1, "int64"),
           "d_new_block_crc": (nb, "int32"), "d_new_res_len": (n, "int64")}
    want = {
        "container": {"d_packed": (total + SLACK, "uint8"), "d_block_first": (n + 1, "int64"), "d_block_off": (nb + 1, "int64"), "d_block_crc": (nb, "int32"),
                      "d_status": (n, "int32"), "d_out": (total + 16 * n, "uint8"), "d_out_off": (n + 1, "int64"), "d_out_len": (n, "int64")},
        "read": {"d_out": (NQ * 112, "uint8"), "d_out_off": (NQ, "int64"), "d_out_cap": (NQ, "int64"), "d_out_len": (NQ, "int64"), "d_status": (NQ, "int32")},
        "write": {"d_new_packed": new["d_new_packed"], "d_new_block_off": (nb + 1, "int64"), "d_new_block_crc": (nb, "int32"), "d_written": (NQ, "int64"),
                  "d_status": (NQ, "int32"), "d_res_status": (n, "int32")},
        "resize": dict(new, d_res_status=(n, "int32")),
        "splice": dict(new, d_status=(n, "int32")),
        "splice_extents": dict(new, d_status=(n, "int32")),
        "diff": {"d_pair": (2 * n, "int64"), "d_delta_ext_first": (n + 1, "int64"), "d_delta_ext": (4 * nb, "int64"), "d_patch_ext_first": (n + 1, "int64"),
                 "d_patch_ext": (4 * nb, "int64"), "d_changed": (n, "int64"), "d_count": (4, "int64"), "d_status": (n, "int32")},
    }
    bounds = {"container": {"in_total_max": total}, "read": {"n_req": NQ, "cap_each": CAP_EACH}, "write": {"in_total_max": total, "n_req": NQ},
              "resize": {"in_total_max": total}, "splice": {"in_total_max": total}, "splice_extents": {"in_total_max": total, "n_ext": 7}, "diff": {}}
    assert sorted(want) == sorted(device.KINDS)
    for kind in device.KINDS:
        assert device.sizes(kind, n, nb, **bounds[kind]) == want[kind], kind
    # and the same counts once more against the per-export statement the recorded calls are held to below
    exports = {"container": ("mscomp_amd_blocks_compress", "mscomp_amd_blocks_crc", "mscomp_amd_blocks_decompress"), "read": ("mscomp_amd_reader_read",),
               "write": ("mscomp_amd_writer_write",), "resize": ("mscomp_amd_writer_resize",), "splice": ("mscomp_amd_splicer_splice",),
               "splice_extents": ("mscomp_amd_splicer_splice_extents",), "diff": ("mscomp_amd_deduper_diff",)}
    for kind, names in exports.items():
        for name, (entries, _) in want[kind].items():
            stated = [h[e][name] for e in names if name in h[e]]
            assert name in BYTES or (stated and entries >= max(stated)), (kind, name)
    with pytest.raises(ValueError):
        device.sizes("read", n, nb, n_ext=1)
    with pytest.raises(ValueError):
        device.sizes("dedup", n, nb)


# ---- the layer over a library that records ----------------------------------------------------------------------------------------------
class _Lib:
    """stands in for the library: records every call as (export, arguments) and answers 0; a create call also gets a handle that is not
    null, so that the object's close() reaches its destroy call"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, export):
        if export.startswith("__"):
            raise AttributeError(export)

        def call(*args):
            self.calls.append((export, args))
            if "_create" in export:
                args[-1]._obj.value = 0xB000 + len(self.calls)
            return 0
        return call


class _Ctx:
    def __init__(self):
        self.lib, self._h, self.device, self.stream, self._handles = _Lib(), C.c_void_p(0xC0), 0, None, weakref.WeakSet()


class _Rig:
    """A BlockOps over CPU tensors and a recording library. Every tensor is kept alive and remembered by its address range: those the layer
    made (through _alloc, the one place it may) with the parameter name they were made for, those the test hands in as "given"."""

    def __init__(self, n, total, B, crc=True):
        import torch
        from ms_compress_amd import device
        self.n, self.total, self.B, self.nb, self.crc, self.tensors = n, total, B, n + total // B, crc, []
        self.ctx, rig = _Ctx(), self

        class Ops(device.BlockOps):
            def _alloc(self, name, entries, dtype, fill=0):
                t = device.BlockOps._alloc(self, name, entries, dtype, fill)
                assert t.numel() >= max(1, entries) and t.dtype == getattr(torch, dtype)
                rig.tensors.append((t, name))
                return t

        self.ops = Ops(self.ctx, 3, B, n, total, crc=crc, _device="cpu")
        assert self.ops.n_blocks_max == self.nb

    def given(self, entries, dtype="int64"):
        import torch
        t = torch.zeros(max(1, entries), dtype=getattr(torch, dtype))
        self.tensors.append((t, None))
        return t

    def find(self, address):
        """(tensor, the name it was made for or None) of the tensor ``address`` lies in"""
        hits = [(t, name) for t, name in self.tensors if t.data_ptr() <= address < t.data_ptr() + t.numel() * t.element_size()]
        assert len(hits) == 1, ("an address of no tensor, or of two", hex(address), len(hits))
        return hits[0]

    def run_all(self):
        """every method once; returns the containers made"""
        ops, n, nb, g = self.ops, self.n, self.nb, self.given
        a = ops.compress(g(self.total + 16, "uint8"), g(n), g(n))
        ops.decompress(a)
        ops.decompress(a, d_range=g(2 * n), check=False)
        ops.read(a, g(3 * NQ), CAP_EACH)
        b, _, _ = ops.write(a, g(3 * NQ), g(NQ * 16 + 16, "uint8"), g(NQ))
        c = ops.resize(b, g(n))
        d = ops.splice([a, c], g(2 * n))
        e = ops.splice_extents([a], g(n + 1), g(4 * 7))
        ops.diff(a, c)
        ops.diff(a, c, d_pair=g(2 * n))
        f, df = ops.delta(a, c)
        h = ops.patch(a, f, df)
        return [a, b, c, d, e, f, h]


def _check_pointer(rig, export, pname, ctype, address, want, lengths):
    """one pointer argument, or one pointer field of a view"""
    nullable = pname in MAY_BE_NULL or (pname in ("d_block_crc", "d_new_block_crc") and not rig.crc)
    nullable = nullable or (export == "mscomp_amd_layout_dev" and pname == "d_cap" and rig.n == 0)      # "n_units && !d_cap": no units, no array
    if not address:
        assert nullable, (export, pname, "is null")
        return
    t, made_for = rig.find(address)
    assert address == t.data_ptr(), (export, pname, "points into a tensor, not at it")
    if not ctype.startswith("const"):
        assert made_for is not None, (export, pname, "a result the layer did not make through _alloc")
    if pname in BYTES:
        lengths[pname] = t.numel()
    else:
        assert pname in want, (export, pname, "no count stated for it")
        assert t.numel() >= want[pname], (export, pname, t.numel(), want[pname])
        assert t.element_size() == (4 if pname.endswith(("crc", "status")) else 8), (export, pname, t.dtype)


def _check_calls(rig, n_ext_of):
    """the recorded calls of ``rig`` against the header; returns how many pointers were held to a count"""
    n, nb, B = rig.n, rig.nb, rig.B
    scalars = {"n_res": n, "n_blocks_table": nb, "block_size": B, "n_pair": n, "n_pick": n, "n_blocks_new": nb, "in_total_max": rig.total, "flags": 0}
    checked = 0
    for export, args in rig.ctx.lib.calls:
        params = PROTOS[export]
        assert len(args) == len(params), (export, len(args), len(params))
        if export.endswith(("_destroy", "_bound")):
            continue
        n_ext = n_ext_of.get(export, 0)
        want = header_counts(n, nb, NQ, n_ext).get(export, {})
        lengths = {}
        for arg, (ctype, pname) in zip(args, params):
            if "blocks_view" in ctype:                          # a host array of views, or one by reference
                views = [arg._obj] if not isinstance(arg, C.Array) else list(arg)
                for v in views:
                    assert (v.n_res, v.n_blocks_table) == (n, nb), export
                    inner = {}
                    for field in ("d_packed", "d_block_first", "d_block_off", "d_res_len", "d_block_crc"):
                        _check_pointer(rig, export, field, "const", getattr(v, field), {"d_block_first": n + 1, "d_block_off": nb + 1, "d_res_len": n,
                                                                                          "d_block_crc": nb}, inner)
                        checked += 1
                    assert v.packed_len <= inner["d_packed"] and v.packed_len <= rig.total, export
            elif "*" in ctype and (arg is None or isinstance(arg, C.c_void_p)) and pname not in ("ctx", "bk", "rd", "wr", "sp", "dd"):
                _check_pointer(rig, export, pname, ctype, None if arg is None else arg.value, want, lengths)
                checked += 1
            elif pname in LENGTH_OF:
                assert LENGTH_OF[pname] in lengths and arg <= lengths[LENGTH_OF[pname]], (export, pname, arg)
                assert arg <= rig.total, (export, pname, arg)
            elif pname in scalars and export.endswith(("_create", "_create_extents", "_create_diff")):
                assert arg == scalars[pname], (export, pname, arg)
    return checked


@pytest.mark.parametrize("crc", [True, False])
@pytest.mark.parametrize("n,total,B", SHAPES)
def test_every_call_of_the_layer_fits_the_header(n, total, B, crc):
    rig = _Rig(n, total, B, crc)
    made = rig.run_all()
    names = [e for e, _ in rig.ctx.lib.calls]
    for export in header_counts(0, 0, 0, 0):
        assert export in names or (export in ("mscomp_amd_blocks_crc", "mscomp_amd_blocks_check") and not crc), export + " was never called"
    # one extent splicer per (n_src, n_ext): for the 7 extents of run_all's own list, and for a diff's lists over one source and over two
    n_ext = {"mscomp_amd_splicer_splice_extents": 0}
    creates = [args for e, args in rig.ctx.lib.calls if e == "mscomp_amd_splicer_create_extents"]
    assert {(a[2], a[4]) for a in creates} == {(1, 7), (1, rig.nb), (2, rig.nb)} and len(creates) == len({(a[2], a[4]) for a in creates})
    assert _check_calls(rig, n_ext) >= 100
    # the extent lists themselves: the given one holds its 7 extents, a diff's hold n_blocks_new
    for e, args in rig.ctx.lib.calls:
        if e == "mscomp_amd_splicer_splice_extents":
            t, made_for = rig.find(args[3].value)
            assert t.numel() >= 4 * (7 if made_for is None else rig.nb)
    for con in made:
        assert (con.n_res, con.n_blocks_table, con.cap) == (n, rig.nb, total) and con.packed.numel() == total + SLACK
        assert (con.block_crc is not None) == crc
        assert con.block_first.numel() >= n + 1 and con.block_off.numel() >= rig.nb + 1 and con.res_len.numel() >= n and con.status.numel() >= n
    rig.ops.close()
    assert sum(e.endswith("_destroy") for e, _ in rig.ctx.lib.calls) >= sum("_create" in e for e, _ in rig.ctx.lib.calls) - 1


def test_a_container_of_another_shape_or_a_short_table_is_refused_before_any_call():
    import torch
    a, b = _Rig(4, 6 * 4096, 4096), _Rig(4, 5 * 4096, 4096)
    con = a.ops.compress(a.given(6 * 4096, "uint8"), a.given(4), a.given(4))
    other = b.ops.compress(b.given(6 * 4096, "uint8"), b.given(4), b.given(4))
    df = a.ops.diff(con, con)
    calls = len(a.ctx.lib.calls)
    z = lambda k: torch.zeros(k, dtype=torch.int64)
    for call in (lambda: a.ops.decompress(other), lambda: a.ops.read(other, z(3), 8), lambda: a.ops.write(other, z(3), z(1), z(1)),
                 lambda: a.ops.resize(other, z(4)), lambda: a.ops.splice([con, other], z(8)), lambda: a.ops.splice_extents([other], z(5), z(4)),
                 lambda: a.ops.diff(con, other), lambda: a.ops.delta(other, con), lambda: a.ops.patch(con, other, df),
                 lambda: a.ops.compress(z(8), z(3), z(4)), lambda: a.ops.resize(con, z(3)), lambda: a.ops.splice([con], z(7)),
                 lambda: a.ops.splice_extents([con], z(4), z(4)), lambda: a.ops.write(con, z(6), z(1), z(1)), lambda: a.ops.diff(con, con, d_pair=z(7)),
                 lambda: a.ops.decompress(con, d_range=z(7)), lambda: a.ops.resize(con, torch.zeros(4, dtype=torch.int32))):
        with pytest.raises(ValueError):
            call()
    assert a.ctx.lib.calls[calls:] == []


# ---- the capture guard ------------------------------------------------------------------------------------------------------------------
def _capturing(monkeypatch):
    """torch.cuda.is_current_stream_capturing says True, and the runtime counts as initialised: the layer asks nothing of a process that
    never touched the GPU"""
    import torch
    mp = monkeypatch.context()
    m = mp.__enter__()
    m.setattr(torch.cuda, "is_initialized", lambda: True)
    m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    return mp


@pytest.mark.parametrize("kind", ["container", "read", "write", "resize", "splice", "splice_extents", "diff"])
def test_an_unprepared_kind_raises_while_the_stream_is_capturing(monkeypatch, kind):
    """An unprepared kind raises RuntimeError naming the kind with no call made; a prepared one goes through without a create call."""
    rig = _Rig(4, 6 * 4096, 4096)
    ops, g, n = rig.ops, rig.given, 4
    a = None if kind == "container" else ops.compress(g(6 * 4096, "uint8"), g(n), g(n))
    call = {"container": lambda: ops.compress(g(6 * 4096, "uint8"), g(n), g(n)), "read": lambda: ops.read(a, g(3 * NQ), CAP_EACH),
            "write": lambda: ops.write(a, g(3 * NQ), g(64, "uint8"), g(NQ)), "resize": lambda: ops.resize(a, g(n)), "splice": lambda: ops.splice([a], g(2 * n)),
            "splice_extents": lambda: ops.splice_extents([a], g(n + 1), g(4 * 7)), "diff": lambda: ops.diff(a, a)}[kind]
    bounds = {"read": {"n_req": NQ}, "write": {"n_req": NQ}, "splice_extents": {"n_src": 1, "n_ext": 7}}.get(kind, {})
    seen = len(rig.ctx.lib.calls)
    assert kind != "container" or seen == 0
    mp = _capturing(monkeypatch)
    with pytest.raises(RuntimeError, match="prepare\\('%s'" % kind):
        call()
    with pytest.raises(RuntimeError, match="prepare\\('%s'" % kind):
        ops.prepare(kind, **bounds)
    assert len(rig.ctx.lib.calls) == seen
    mp.__exit__(None, None, None)
    ops.prepare(kind, **bounds)
    if kind == "diff":
        assert ops._pairs.tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
    seen = len(rig.ctx.lib.calls)
    mp = _capturing(monkeypatch)
    call()
    ops.prepare(kind, **bounds)                                           # (prepared already: nothing to make)
    mp.__exit__(None, None, None)
    assert len(rig.ctx.lib.calls) > seen and not any("_create" in e for e, _ in rig.ctx.lib.calls[seen:])


def test_resize_runs_on_a_prepared_writer_that_fits():
    rig = _Rig(4, 6 * 4096, 4096)
    ops = rig.ops
    ops.prepare("write", n_req=NQ, blocks_max=5)
    ops.prepare("resize", blocks_max=5)
    assert ops._made[("resize",)] is ops._made[("write", NQ)]
    ops.prepare("resize", blocks_max=6)                                   # no longer fits: a writer of its own, the shared one stays
    assert ops._made[("resize",)] is not ops._made[("write", NQ)] and ops._made[("resize",)].n_req == 0
    ops.prepare("write", n_req=NQ, blocks_max=8)                          # and back onto the wider writer
    assert ops._made[("resize",)] is ops._made[("write", NQ)] and ops._made[("write", NQ)].blocks_max == 8
    creates = [e for e, _ in rig.ctx.lib.calls if e == "mscomp_amd_writer_create"]
    destroys = [e for e, _ in rig.ctx.lib.calls if e == "mscomp_amd_writer_destroy"]
    assert (len(creates), len(destroys)) == (3, 2)
    with pytest.raises(ValueError):
        ops.prepare("read")                                              # a reader is made for one request count
    with pytest.raises(ValueError):
        ops.prepare("write", n_ext=3)


def test_read_lays_its_slots_out_without_touching_the_requests():
    rig = _Rig(1, 4096, 4096)
    a = rig.ops.compress(rig.given(4096, "uint8"), rig.given(1), rig.given(1))
    d_req = rig.given(3 * NQ)
    d_req[2] = -1                                                         # a length of 2^64 - 1: "to the end"
    d_out, d_off, d_len, d_st = rig.ops.read(a, d_req, CAP_EACH)
    assert d_off.tolist() == [0, 112, 224] and d_out.numel() == 3 * 112 and d_req.tolist() == [0, 0, -1] + [0] * 6
    args = [args for e, args in rig.ctx.lib.calls if e == "mscomp_amd_reader_read"][0]
    cap = rig.find(args[10].value)[0]
    assert cap.tolist() == [CAP_EACH] * NQ


# ---- import and layering ----------------------------------------------------------------------------------------------------------------
def test_the_layer_imports_without_a_gpu_and_composes_the_handle_classes():
    import inspect
    import ms_compress_amd as m
    assert m.BlockOps is m.api.BlockOps is m.device.BlockOps and m.DeviceBlocks is m.api.DeviceBlocks and m.BlockDiff is m.api.BlockDiff
    assert not issubclass(m.DeviceBlocks, m.api._Handle) and not issubclass(m.BlockOps, m.api._Handle)
    named = set(re.findall(r"\bmscomp_amd_[a-z0-9_]+", inspect.getsource(m.device)))
    assert named <= set(m.api.EXPORTS), sorted(named - set(m.api.EXPORTS))
    assert m.BlockDiff._fields == ("delta_ext_first", "delta_ext", "patch_ext_first", "patch_ext", "changed", "count", "status")


def test_a_container_from_host_arrays_has_the_tables_it_states():
    import numpy as np
    import ms_compress_amd as m
    ctx = _Ctx()
    host = (np.arange(10, dtype=np.uint8), [0, 1, 2], [0, 4, 10], [4096, 100], np.array([7, 9], dtype=np.uint32))
    con = m.DeviceBlocks.from_host(ctx, 2, 4096, host, n_blocks_table=5, cap=8192, _device="cpu")
    assert (con.n_res, con.n_blocks_table, con.cap, con.packed.numel()) == (2, 5, 8192, 8192 + SLACK)
    assert con.block_off.tolist() == [0, 4, 10, 10, 10, 10] and con.block_first.tolist() == [0, 1, 2] and con.block_crc.tolist() == [7, 9, 0, 0, 0]
    assert con.view()[5:] == (8192, 2, 5) and con.view(crc=False)[4] is None
    with pytest.raises(ValueError):
        m.DeviceBlocks.from_host(ctx, 2, 4096, host, n_blocks_table=1, _device="cpu")
    with pytest.raises(ValueError):
        m.DeviceBlocks(ctx, 2, 4096, 2, 5, con.packed, 8192, con.block_first, con.block_off[:5], con.res_len, None, con.status)
