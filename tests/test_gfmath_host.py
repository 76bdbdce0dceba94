"""CPU: csrc/gfmath.h itself -- the header is host and device code, so what the solver of the parity kernels computes with can be run here.
tests/gfmath_host.cpp is compiled against it with the host C++ compiler and prints every table the header can make: gf_x2 and gf_mulc in
every lane of a dword with other bytes beside them, gf_mul, gf_exp past its wrap (0 .. 765 = 3 * 255), gf_inv. They are compared with
tests/parity_model.py's log / antilog field (EXP, mul, inv, x2_packed), which tests/test_parity_model.py pins. gf_invert runs over every
parity subset of {0, 1, 2} with every member, member pair and member triple of k = 255 -- 3 * 255 + 3 * 32 385 + 2 731 135 matrices --; the
program checks A inv = I itself by a table product and prints the counts, and a fixed sample of its inverses is held to
parity_model.invert here, entry by entry. Compiled and run once per session."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import parity_model as Y

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ms_compress_amd", "csrc")
PATTERNS = (0x00000000, 0xA55A3CC3, 0xFFFFFFFF)
SAMPLE = 2039
MATRICES = 3 * 255 + 3 * (255 * 254 // 2) + 255 * 254 * 253 // 6


def _compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = c and shutil.which(c)
        if path:
            return path
    pytest.fail("no host C++ compiler: this test does not skip")


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    """{section: array of its numbers}, the sampled matrices, and the counts line"""
    exe = str(tmp_path_factory.mktemp("gfmath") / "gfmath_host")
    subprocess.run([_compiler(), "-O2", "-std=c++17", "-I", CSRC, os.path.join(HERE, "gfmath_host.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    tables, sample, counts = {}, [], None
    for line in out.splitlines():
        head, _, rest = line.partition(" ")
        if head == "M":
            sample.append([int(x) for x in rest.split()])
        elif head == "invert":
            w = rest.split()
            counts = {w[i]: int(w[i + 1]) for i in range(0, len(w), 2)}
        else:
            tables[head] = np.array([int(x, 16) for x in rest.split()], dtype=np.int64)
    return tables, sample, counts


def _lanes(words):
    return [(words >> (8 * o)) & 0xFF for o in range(4)]


def test_times_alpha_in_every_lane(printed):
    got = printed[0]["x2"].reshape(3, 4, 256)
    v = np.arange(256, dtype=np.int64)
    for pat, P in enumerate(PATTERNS):
        for lane in range(4):
            words = (P & ~(0xFF << (8 * lane)) & 0xFFFFFFFF) | v << (8 * lane)
            assert got[pat, lane].tolist() == [Y.x2_packed(w) for w in words], (pat, lane)
            for o, (g, w) in enumerate(zip(_lanes(got[pat, lane]), _lanes(words))):
                assert np.array_equal(g, Y.mul(2, w)), (pat, lane, o)


def test_every_product_in_every_lane(printed):
    got = printed[0]["mulc"].reshape(4, 256, 256)                 # [lane][c][v]
    c, v = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    assert (got >> 32 == 0).all()
    for lane in range(4):
        words = (PATTERNS[1] & ~(0xFF << (8 * lane)) & 0xFFFFFFFF) | v << (8 * lane)
        for o, (g, w) in enumerate(zip(_lanes(got[lane]), _lanes(words))):
            assert np.array_equal(g, Y.mul(w, c)), (lane, o)       # the lane under test: all 65536 products; beside it: the other bytes' own
    assert np.array_equal(printed[0]["mul"].reshape(256, 256), Y.mul(c, v))


def test_powers_past_the_wrap_and_inverses(printed):
    exp, inv = printed[0]["exp"], printed[0]["inv"]
    assert len(exp) == 766 and exp.tolist() == [int(Y.EXP[n % 255]) for n in range(766)]
    assert exp[255] == exp[510] == exp[765] == 1 and exp[256] == 2, "2 * 128 is the first product of a parity and a member that wraps"
    assert inv.tolist() == [Y.inv(a) for a in range(1, 256)]
    assert all(int(Y.mul(a, int(inv[a - 1]))) == 1 for a in range(1, 256))


def test_every_matrix_the_solver_can_meet_is_inverted(printed):
    _, sample, counts = printed
    assert counts == {"checked": MATRICES, "bad": 0, "singular": 0, "garbage": 0}, counts
    assert len(sample) == MATRICES // SAMPLE + 3 * 5
    seen = set()
    for row in sample:
        e = row[0]
        ps, members, got = row[1: 1 + e], row[1 + e: 1 + 2 * e], row[1 + 2 * e:]
        want = Y.invert([[Y.coef(p, i) for i in members] for p in ps])
        assert want is not None and got == [x for r in want for x in r], (ps, members, got, want)
        seen.add(tuple(ps))
    assert seen == {(0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)} and max(max(r[1 + r[0]: 1 + 2 * r[0]]) for r in sample) >= 250
