"""CPU: how the library reads its environment. csrc/envnum.h is host code without HIP, so tests/envnum_host.cpp is compiled against it with
the host C++ compiler and prints what every numeric accessor of csrc/hooks.hip computes from a given string. The table below was printed
once by the hand-written getenv lambdas that the accessors replaced (one per variable, spread over five files), for every variable and for
the strings unset, empty, abc, 0, 1, -5, 12abc, " 7", 4294967296, both ends of the range and one past each end -- none overflows a long.
The second half holds the documentation to the code: INTEGRATION.md section 5 names exactly the variables hooks.hip reads, and no other
file under csrc/ asks the environment. Compiled and run once per session."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ms_compress_amd", "csrc")
COMMON = (None, "", "abc", "0", "1", "-5", "12abc", " 7", "4294967296")
M = 1 << 20
# name: (lo, hi or None, what the strings of COMMON give, then lo, lo - 1, and where there is an upper end hi, hi + 1)
TABLE = {
    "MSCOMP_AMD_LZG_MAX_MB": (0, None, (65536 * M, 0, 0, 0, M, 0, 12 * M, 7 * M, 4294967296 * M, 0, 0)),
    "MSCOMP_AMD_XHC_SCR_MAX_MB": (0, None, (32768 * M, 0, 0, 0, M, 0, 12 * M, 7 * M, 4294967296 * M, 0, 0)),
    "MSCOMP_AMD_ONE_SLICE_MB": (1, 4096, (24 * M, 24 * M, 24 * M, 24 * M, M, 24 * M, 12 * M, 7 * M, 24 * M, M, 24 * M, 4096 * M, 24 * M)),
    "MSCOMP_AMD_ONE_RANGED_MIN_MB": (1, 65536, (8 * M, 8 * M, 8 * M, 8 * M, M, 8 * M, 12 * M, 7 * M, 8 * M, M, 8 * M, 65536 * M, 8 * M)),
    "MSCOMP_AMD_ONE_RANGE_CHUNKS": (1, 65536, (256, 256, 256, 256, 1, 256, 12, 7, 256, 1, 256, 65536, 256)),
    "MSCOMP_AMD_HOST_BATCH_MB": (1, 65536, (0, 0, 0, 0, M, 0, 12 * M, 7 * M, 0, M, 0, 65536 * M, 0)),
    "MSCOMP_AMD_HOST_SLOTS": (1, 8, (8, 8, 8, 8, 1, 8, 8, 7, 8, 1, 8, 8, 8)),
    "MSCOMP_AMD_XPS_SEG_KB": (4, 65536, (16384, 16384, 16384, 16384, 16384, 16384, 12288, 7168, 16384, 4096, 16384, 65536 << 10, 16384)),
    "MSCOMP_AMD_XPS_WARM_KB": (1, 65536, (16384, 16384, 16384, 16384, 1024, 16384, 12288, 7168, 16384, 1024, 16384, 16384, 16384)),
    "MSCOMP_AMD_XPS_ROUNDS": (1, 256, (8, 8, 8, 8, 1, 8, 12, 7, 8, 1, 8, 256, 8)),
    "MSCOMP_AMD_LZB_MIN_KB": (1, 1048575, (32768, 32768, 32768, 32768, 1024, 32768, 12288, 7168, 32768, 1024, 32768, 1048575 << 10, 32768)),
    "MSCOMP_AMD_LZG_HOPS": (1, 999, (8, 8, 8, 8, 1, 8, 12, 7, 8, 1, 8, 999, 8)),
}
# the warm-up is capped by the segment, whatever set the segment
WARM_UNDER_SEG = (("MSCOMP_AMD_XPS_WARM_KB=8;MSCOMP_AMD_XPS_SEG_KB=4", 4096), ("MSCOMP_AMD_XPS_WARM_KB=2;MSCOMP_AMD_XPS_SEG_KB=4", 2048),
                  ("MSCOMP_AMD_XPS_WARM_KB;MSCOMP_AMD_XPS_SEG_KB=8", 8192))
FLAGS = ("MSCOMP_AMD_LZNT1_SA_DICT", "MSCOMP_AMD_NO_GRAPH", "MSCOMP_AMD_ONE_ZEROCOPY", "MSCOMP_AMD_HOST_ORDER", "MSCOMP_AMD_HOST_TRACE",
         "MSCOMP_AMD_TEST_HOOKS")
DEFAULTS = {"XPS_SEG": "kernels.h", "XPS_WARM": "kernels.h", "XPS_ROUNDS": "kernels.h", "LZB_MIN_KB": "kernels.h", "LZG_HOPS": "kernels.h",
            "HB_SLOTS": "host.h"}


def _read(*path):
    with open(os.path.join(*path), encoding="utf-8") as f:
        return f.read()


def _strings(name):
    lo, hi, _ = TABLE[name]
    return COMMON + (str(lo), str(lo - 1)) + ((str(hi), str(hi + 1)) if hi is not None else ())


def _compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = c and shutil.which(c)
        if path:
            return path
    pytest.fail("no host C++ compiler: this test does not skip")


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    """{input line: the number the program printed for it}"""
    exe = str(tmp_path_factory.mktemp("envnum") / "envnum_host")
    subprocess.run([_compiler(), "-O2", "-std=c++17", "-I", CSRC, os.path.join(HERE, "envnum_host.cpp"), "-o", exe], check=True)
    lines = [n if s is None else "%s=%s" % (n, s) for n in TABLE for s in _strings(n)] + [l for l, _ in WARM_UNDER_SEG]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split()
    assert len(out) == len(lines)
    return dict(zip(lines, out))


@pytest.mark.parametrize("name", sorted(TABLE))
def test_accessor_reads_what_its_lambda_read(printed, name):
    want = TABLE[name][2]
    strings = _strings(name)
    assert len(want) == len(strings)
    assert all(len(s) <= 10 for s in strings if s), "no string may overflow a long"
    got = [int(printed[name if s is None else "%s=%s" % (name, s)]) for s in strings]
    assert got == list(want), list(zip(strings, got, want))


def test_warm_up_is_capped_by_the_segment(printed):
    assert [int(printed[l]) for l, _ in WARM_UNDER_SEG] == [w for _, w in WARM_UNDER_SEG]


def test_the_program_restates_the_accessors_of_hooks_hip():
    """every parser call of envnum_host.cpp is the call of the same variable in hooks.hip, text for text, over the same defaults"""
    hooks, prog = _read(CSRC, "hooks.hip"), _read(HERE, "envnum_host.cpp")
    for name in TABLE:
        calls = [re.findall(r'=\s*([^=;]*?)(?:getenv|E)\("%s"\)([^;]*);' % name, text) for text in (hooks, prog)]
        assert len(calls[0]) == 1 and calls[0] == calls[1], (name, calls)
    assert re.findall(r"static uint64_t mib_budget[^\n]*", hooks) == re.findall(r"static uint64_t mib_budget[^\n]*", prog) != []
    for macro, header in DEFAULTS.items():
        pat = r"#define %s\s+(\w+)" % macro
        assert re.findall(pat, prog) == re.findall(pat, _read(CSRC, header)) != [], macro


def test_integration_md_names_the_variables_hooks_hip_reads():
    hooks = _read(CSRC, "hooks.hip")
    read = set(re.findall(r'getenv\("(MSCOMP_AMD_\w+)"\)', hooks))
    assert len(re.findall(r"getenv\(", hooks)) == len(read), "one getenv call per variable, each with its name as a literal"
    assert read == set(TABLE) | set(FLAGS)
    section = re.search(r"\n## 5\. Environment variables.*?\n## 6\. ", _read(ROOT, "INTEGRATION.md"), re.S).group(0)
    named = set(re.findall(r"MSCOMP_AMD_[A-Z0-9_]*[A-Z0-9]", section))
    assert named - {"MSCOMP_AMD_LIB"} == read, (sorted(named - read), sorted(read - named))       # (MSCOMP_AMD_LIB: the Python package's)


def test_no_other_file_asks_the_environment():
    others = [f for f in sorted(os.listdir(CSRC)) if f != "hooks.hip" and os.path.isfile(os.path.join(CSRC, f))
              and not f.endswith((".o", ".so")) and "getenv" in _read(CSRC, f)]
    assert others == []
