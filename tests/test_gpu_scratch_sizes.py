"""GPU: every scratch buffer of a context and of a plan is asked for the bytes tests/golden/scratch_asked.json records (tools/
make_golden_scratch.py; the cases: tests/scratch_cases.py). The layout functions of csrc/host.h give both a buffer's size and its columns, so a
layout that changes shows here for every buffer at once, where the slack canaries of test_gpu_scratch.py see only an overrun. Plans are
created and never executed."""
import json
import os

import pytest

import scratch_cases as S

pytestmark = pytest.mark.gpu
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scratch_asked.json")) as fh:
    GOLDEN = json.load(fh)
CASES = S.cases()


def test_the_fixture_has_these_cases_and_no_others():
    assert sorted(GOLDEN) == sorted(name for name, _, _ in CASES)


@pytest.mark.parametrize("name,f,make", CASES, ids=[c[0] for c in CASES])
def test_asked_bytes_are_the_recorded_ones(gpu_ctx, name, f, make):
    import ms_compress_amd as m
    if S.env_in_the_way():
        pytest.skip("set in the environment, they resize the optional paths: %s" % ", ".join(S.env_in_the_way()))
    got, want = S.asked(m, make, f), GOLDEN[name]
    assert got == want, {k: (got.get(k), want.get(k)) for k in sorted(set(got) | set(want)) if got.get(k) != want.get(k)}
