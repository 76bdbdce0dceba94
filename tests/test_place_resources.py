"""CPU: the resources of the LZNT1 placement kernel (csrc/util.hip concat_slots_kernel, both instances) as the compiler reports them for
gfx950 with the Makefile's flags, in the manner of test_rowpass_resources.py: a wave holds the four 16-byte loads of an image in registers
between its loads and its stores and a unit's row in scalar registers; neither may end in scratch memory, and nothing may spill. Registers
and occupancy are not pinned. No other kernel of the file may use scratch memory either."""
import functools
import os
import re
import subprocess
import tempfile

import pytest

from test_lznt1_resources import CSRC, HIPCC, _makefile_flags


@functools.lru_cache(maxsize=None)
def _resources():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.run([HIPCC] + _makefile_flags() + ["-c", os.path.join(CSRC, "util.hip"), "-o", os.path.join(tmp, "util.o"),
                                                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True).stderr
    ks, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = ks.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    for k in sorted(ks):
        print(k, {f: ks[k][f] for f in ("TotalSGPRs", "VGPRs", "Occupancy", "SGPRs Spill", "VGPRs Spill", "ScratchSize", "LDS Size")})
    return ks


def test_both_instances_are_seen():
    place = [k for k in _resources() if "concat_slots_kernel" in k]
    assert len(place) == 2 and any("ILb0E" in k for k in place) and any("ILb1E" in k for k in place), sorted(_resources())


def test_no_scratch_memory_and_no_spills():
    for k, r in _resources().items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)


def test_the_placement_uses_no_lds():
    for k, r in _resources().items():
        if "concat_slots_kernel" in k:
            assert r["LDS Size"] == 0, (k, r)
