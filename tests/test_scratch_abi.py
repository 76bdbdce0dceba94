"""CPU: the three scratch hooks (mscomp_amd_debug_scratch_names / _poison / _report) are exported, declared in the header
with their prototypes and named in api.EXPORTS; they answer -1 with the hooks off, for null handles and for unknown kinds before they touch
a device; and the names of a context's buffers are exactly the DevBuf members of mscomp_amd_ctx -- in the manner of tests/test_dedup_abi.py.
(What they do to real scratch is in tests/test_gpu_scratch.py.)"""
import ctypes as C
import os
import re
import subprocess
import sys

import abi_rig as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mscomp_amd_debug_scratch_names", "mscomp_amd_debug_scratch_poison", "mscomp_amd_debug_scratch_report")
PROTOTYPES = (
    "int mscomp_amd_debug_scratch_names(const char** names, int cap);",
    "int mscomp_amd_debug_scratch_poison(int kind, void* object, int slack_only, int byte);",
    "int mscomp_amd_debug_scratch_report(int kind, void* object, int byte, mscomp_amd_scratch_rec* recs, int cap);",
)
KINDS = ("CTX", "PLAN", "BLOCKS", "READER", "WRITER", "SPLICER", "DEDUPER")


def _ctx_members():
    """the DevBuf members of struct mscomp_amd_ctx in csrc/host.h, in the order they are declared, and the list bufs() is made from"""
    src = open(os.path.join(ROOT, "ms_compress_amd", "csrc", "host.h")).read()
    body = src[src.index("struct mscomp_amd_ctx {"): src.index("struct mscomp_amd_plan {")]
    declared = []
    for line in body.splitlines():
        mm = re.match(r"\s*msc::DevBuf ([a-z0-9_, ]+);", line)
        if mm:
            declared += [x.strip() for x in mm.group(1).split(",")]
    listed = re.findall(r"X\((\w+)\)", body[body.index("#define MSC_CTX_BUFS(X)"): body.index("std::vector<msc::DevBuf*> bufs()")])
    return declared, listed


def test_scratch_symbols_are_exported_and_declared():
    import ms_compress_amd as m
    lib = m.load_library()
    R.check_declared(lib, NAMES, PROTOTYPES)
    flat = R.flat_header()
    for k, name in enumerate(KINDS):
        assert "#define MSCOMP_AMD_SCRATCH_%s %d " % (name, k) in flat + " ", name
    assert "typedef struct mscomp_amd_scratch_rec { const char* name; uint64_t asked, cap, changed; } mscomp_amd_scratch_rec;" in flat
    assert C.sizeof(m.api.ScratchRec) == 32
    assert callable(m.api.scratch_names) and callable(m.api.scratch_poison) and callable(m.api.scratch_report)


def test_context_names_are_the_buffers_of_bufs():
    import ms_compress_amd as m
    assert m.load_library().mscomp_amd_debug_hooks_enabled() == 1            # tests/conftest.py asked for them
    declared, listed = _ctx_members()
    names = m.api.scratch_names()
    assert len(names) == len(set(names)) >= 30
    assert names == listed                                       # bufs() and the names come from the one list ...
    assert sorted(names) == sorted(declared)                     # ... which holds every DevBuf the context declares, and nothing else
    lib = m.load_library()
    few = (C.c_char_p * 3)()
    assert lib.mscomp_amd_debug_scratch_names(few, 3) == len(names) and [x.decode() for x in few] == names[:3]
    assert lib.mscomp_amd_debug_scratch_names(None, 3) == -1                 # room stated, none given


def test_null_handles_and_unknown_kinds_are_refused():
    import ms_compress_amd as m
    lib = m.load_library()
    import threading
    recs = (m.api.ScratchRec * 4)()
    got = []

    def nulls():                                                  # kind 0 with a null object: a thread that has made no one-shot call has no such context
        for kind in range(len(KINDS)):
            got.append((lib.mscomp_amd_debug_scratch_poison(kind, None, 0, 0xA5), lib.mscomp_amd_debug_scratch_poison(kind, None, 1, 0xA5),
                        lib.mscomp_amd_debug_scratch_report(kind, None, 0xA5, recs, 4), m.api.scratch_poison(None, 0x11)))
    t = threading.Thread(target=nulls)
    t.start()
    t.join()
    assert got == [(-1, -1, -1, -1)] * len(KINDS), got
    obj = C.c_void_p(8)                                           # never dereferenced: the kind is refused first
    for kind in (-1, len(KINDS), 1000):
        assert lib.mscomp_amd_debug_scratch_poison(kind, obj, 1, 0) == -1, kind
        assert lib.mscomp_amd_debug_scratch_report(kind, obj, 0, recs, 4) == -1, kind
    assert all(not r.name and r.cap == 0 for r in recs)          # nothing was written


def test_hooks_off_answers_minus_one():
    """a process that did not ask for the hooks before the library loaded gets -1 from all three, whatever it passes"""
    code = ("import sys, ctypes as C; sys.path.insert(0, %r); import ms_compress_amd as m; l = m.load_library(); p = C.c_void_p(8);"
            "r = (m.api.ScratchRec * 2)(); n = (C.c_char_p * 2)();"
            "print(l.mscomp_amd_debug_hooks_enabled(), l.mscomp_amd_debug_scratch_names(n, 2),"
            " [l.mscomp_amd_debug_scratch_poison(k, o, s, 1) for k in range(7) for o in (None, p) for s in (0, 1)],"
            " [l.mscomp_amd_debug_scratch_report(k, o, 1, r, 2) for k in range(7) for o in (None, p)], n[0], r[0].name)") % ROOT
    env = {k: v for k, v in os.environ.items() if k != "MSCOMP_AMD_TEST_HOOKS"}
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-500:]
    assert r.stdout.strip().splitlines()[-1] == "0 -1 %r %r None None" % ([-1] * 28, [-1] * 14), r.stdout
