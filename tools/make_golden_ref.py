"""Record the compiled reference's answers (oracle/_ref, built by oracle/Makefile from the reference's sources) into
tests/golden/ref_answers.json and tests/golden/ref_c_symbols.json, so that the tests comparing against the reference run where it
cannot be built (tests/refanswers.py). Run where oracle/_ref exists; no GPU needed:

    python tools/make_golden_ref.py
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import pytest

import refanswers
from oracle import loader

ref, ref_sa = loader.load_ref(), loader.load_ref_sa()
assert ref is not None and ref_sa is not None, "oracle/_ref missing: run make -C oracle"

# 1. the CPU tests: every answer they ask the live reference for is kept
rc = pytest.main(["-q", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_oracle_vs_ref.py"), os.path.join(ROOT, "tests", "test_foreign_streams.py"),
                  os.path.join(ROOT, "tests", "test_abi.py") + "::test_xpress_deflate_entry_points_answer_like_the_reference"])
assert rc == 0, "the CPU tests against the live reference failed: nothing recorded"

# 2. the reference's side of the GPU tests (the GPU side is not needed to know what the reference answers)
import test_gpu_decompress
import test_gpu_stream as ts
for data, steps, tail in ts.deflate_cases():
    ts.ref_drive(ref, 2, data, steps, tail)
for stream, cap, steps, tail in ts.inflate_cases(loader):
    ts.ref_drive_inflate(ref, 2, stream, steps, tail, cap)
for data, steps, tail in ts.sa_deflate_cases():
    ts.ref_drive(ref_sa, 2, data, steps, tail, "deflate sa")
refanswers.answer(("deflate look-ahead",), lambda: ts.deflate_look_ahead_run(ref))
import cases
data = cases.mixed_buffer()
for f in (2, 3, 4):
    bad = test_gpu_decompress.corrupted(f, loader.oracle_compress(f, data)[1])
    refanswers.answer(("decompress", f, bad, len(data)), lambda: loader.ref_decompress(f, bad, len(data)))
import test_foreign_streams as tf          # (the GPU side of test_gpu_foreign_streams.py asks the same family questions)
for f in (2, 3, 4):
    fam, _ = tf.family(f)
    tf.reference_answer(loader, f, fam, tf.checker_results(loader, f, fam)[1])
refanswers.record()
print("%d answers recorded in %s" % (len(refanswers.live_answers), refanswers.PATH))

# 3. the C-linkage functions the compiled reference exports (tests/test_abi.py)
out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "oracle", "_ref", "libMSCompression.so")],
                     capture_output=True, text=True, check=True).stdout
syms = sorted({l.split()[2] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T"} - {""})
syms = [s for s in syms if not s.startswith("_")]
with open(os.path.join(ROOT, "tests", "golden", "ref_c_symbols.json"), "w") as f:
    json.dump(syms, f, indent=0)
    f.write("\n")
