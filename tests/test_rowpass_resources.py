"""CPU: the resources of the deduper calls' kernels (dedup.hip, diff.hip, match.hip, repair.hip), of the syncer's (sync.hip), which walks
the same key table, of the digest passes (digest.hip) and of the parity object's kernels (parity.hip) as the compiler reports them for gfx950, compiled with the Makefile's flags.
What the files share lives in rowpass.h as function templates over functors, inlined into every kernel; where such a template goes
wrong it does so silently -- an array passed by reference that ends in scratch memory, a struct that is spilled -- and this is where it shows: no kernel may use scratch memory, but for the 40 bytes per lane that mt_keys_kernel,
mt_confirm_kernel and mt_settle_kernel were written with, and no kernel may spill registers. Registers and occupancy are
not pinned. Each file is compiled once.

Before rowpass.h the kernels that took four views as four arguments held all of them in scalar registers for the selects -- 64 of 106 --
and spilled (dd_seed_kernel 2, dd_confirm_kernel 4, dd_settle_kernel 26, df_seed_kernel 8, mt_seed_kernel 2, mt_confirm_kernel 32,
mt_settle_kernel 38); they take one SpliceSrc now, which a lane indexes in the kernel-argument segment, and nothing spills. The 40 bytes
of scratch went with it; the bound of 40 is kept as it was set.

parity.hip came under these assertions with two kernels that spilled scalar registers: pa_damage_kernel 23 at 106 -- gf_invert's 44
products, each unrolled to eight selects whose masks the scheduler kept alive side by side; they are gf_mul4 now (gfmath.h: four products to a dword, masks by
arithmetic), 68 scalar registers -- and pa_scan_kernel 2 -- eight "entry < n" masks held across the block scan beside the scan's own; a lane whose
eight entries all exist no longer tests them one by one, 93."""
import functools
import os
import re
import subprocess
import tempfile

import pytest

from test_lznt1_resources import CSRC, HIPCC, _makefile_flags

FILES = ("dedup", "diff", "match", "repair", "sync", "digest", "parity")
EACH = pytest.mark.parametrize("name", FILES)
SCRATCH_KNOWN = ("mt_keys_kernel", "mt_confirm_kernel", "mt_settle_kernel")      # 40 bytes per lane each, at most
# the kernels a file must be found to hold, by substring: a renamed kernel must not slip out of the checks
HOLDS = {"dedup": ("dd_seed_kernel", "dd_rows_kernel", "dd_insert_kernel", "dd_cand_kernel", "dd_confirm_kernel", "dd_settle_kernel"),
         "diff": ("df_seed_kernel", "df_verdict_kernel", "df_confirm_kernel", "df_tile_kernel", "rows_tilescan_kernel", "df_runs_kernel", "df_counts_kernel"),
         "match": ("mt_seed_kernel", "mt_keys_kernel", "mt_confirm_kernel", "mt_settle_kernel", "mt_tile_kernel", "rows_tilescan_kernel", "mt_runs_kernel",
                   "mt_counts_kernel"),
         "repair": ("rp_seed_kernel", "rp_choice_kernel", "rp_tile_kernel", "rp_runs_kernel", "rp_counts_kernel"),
         "sync": ("sy_clear_kernel", "sy_seed_kernel", "sy_keys_kernel", "sy_units_kernel", "sy_piece_kernel", "sy_pre_kernel", "sy_abs_kernel", "sy_scan_kernel",
                  "sy_tilescan_kernel", "sy_req_kernel", "sy_confirm_kernel", "sy_dunits_kernel", "sy_dcompare_kernel", "sy_select_kernel"),
         "digest": ("dg_leaf_kernel", "dg_root_kernel"),
         "parity": ("pa_rows_kernel", "pa_groups_kernel", "pa_scan_kernel", "pa_units_kernel", "pa_build_kernel", "pa_head_kernel", "pa_check_kernel",
                    "pa_damage_kernel", "pa_solve_kernel", "pa_tail_kernel")}


@functools.lru_cache(maxsize=None)
def _resources(name):
    """{kernel name: {remark: value}} of one file's kernels"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.run([HIPCC] + _makefile_flags() + ["-c", os.path.join(CSRC, name + ".hip"), "-o", os.path.join(tmp, name + ".o"),
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


@EACH
def test_every_kernel_is_seen(name):
    ks = _resources(name)
    for part in HOLDS[name]:
        assert any(part in k for k in ks), (part, sorted(ks))


@EACH
def test_no_scratch_memory(name):
    for k, r in _resources(name).items():
        assert r["ScratchSize"] <= (40 if any(part in k for part in SCRATCH_KNOWN) else 0), (k, r)


@EACH
def test_no_vector_register_spills(name):
    for k, r in _resources(name).items():
        assert r["VGPRs Spill"] == 0, (k, r)


@EACH
def test_no_scalar_register_spills(name):
    spilled = {k: r["SGPRs Spill"] for k, r in _resources(name).items() if r["SGPRs Spill"]}
    assert not spilled, spilled
