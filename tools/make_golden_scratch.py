"""tests/golden/scratch_asked.json: the bytes every scratch buffer of a context and of a plan is asked for, {case: {buffer name: asked}},
over the cases of tests/scratch_cases.py. Nothing is executed. Needs a GPU; run it with the library of the commit whose sizes are to be
kept, before a change to the layout functions of csrc/host.h.        python tools/make_golden_scratch.py [out.json]
"""
import json
import os
import sys

os.environ.setdefault("MSCOMP_AMD_TEST_HOOKS", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import ms_compress_amd as m
import scratch_cases as S

if S.env_in_the_way():
    sys.exit("unset %s first: they resize the optional paths" % ", ".join(S.env_in_the_way()))
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "scratch_asked.json")
golden = {name: S.asked(m, make, f) for name, f, make in S.cases()}
with open(out, "w") as fh:
    json.dump(golden, fh, indent=0, sort_keys=True)
    fh.write("\n")
print("%d cases, %d buffers -> %s" % (len(golden), sum(len(v) for v in golden.values()), out))
