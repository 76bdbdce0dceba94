"""bench.py end to end on the GPU box: the multi-rank path (two ranks sharing the one GPU: SURVEY.md 8e) and the parity gate on data
that is NOT the synthetic corpus (SILESIA_DIR: the reference's encoder is run on the host, BASELINE.json north_star "full Silesia corpus")."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bench(args, env=None, timeout=900):
    import signal
    e = dict(os.environ)
    e.update(env or {})
    # (its own session: on a timeout the WHOLE tree goes -- the launcher's workers too, which subprocess.run's own kill would leave behind on the GPU)
    p = subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, err = p.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        out, err = p.communicate()
        raise AssertionError("bench.py %s did not finish in %d s\n%s" % (" ".join(args), timeout, err[-2000:]))
    assert p.returncode == 0, err[-2000:]
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out[-2000:]
    return json.loads(lines[0])


def test_the_drivers_own_command_prints_one_short_parseable_line():
    """EXACTLY the --full run made once per change at N = 1 (all legs, CPU baselines included; only K and W smaller): the last stdout line must parse,
    stay under 4 KiB (a benchmark record keeps the last 8 KB of stdout: round 4's 20 KB line was lost to it) and carry the headline objects;
    the long document goes to bench_extra.json."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--full"], cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.rstrip("\n").splitlines()
    assert len(r.stdout) < 8192 and len(out[-1]) < 4096, (len(r.stdout), len(out[-1]))
    line = json.loads(out[-1])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in line, key
    assert line["n_gpus"] == 1 and line["steps"] == 2 and line["warmup"] == 1 and line["value"] > 0 and line["unit"] == "MB/s"
    from ms_compress_amd import corpus
    total = sum(corpus.SIZES) * 16 if corpus.source() == "synthetic" else None        # (SILESIA_DIR: the real files have the same sizes by corpus.source()'s own check)
    assert "configs[4]" in line["config"]["workload"] and line["config"]["bytes_per_step"] == (total or 3391017280)
    assert 0 < line["roofline"]["frac"] < 1 and line["roofline"]["bound"] == "hbm" and line["roofline"]["kernel_ms_per_launch"] > 0
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["balanced_value"] >= line["cpu_baseline"]["value"] * 0.5 and line["cpu_baseline"]["cores"] >= 1
    assert line["parity_checked"] == {"lznt1": True, "xpress": True, "xpress_huff": True}
    for codec in ("lznt1", "xpress", "xpress_huff"):
        assert line["config"]["%s_MB_per_s" % codec] > 0 and 0 < line["config"]["%s_roofline_frac" % codec] < 1

    def no_prose(x, where="line"):
        if isinstance(x, dict):
            for k, v in x.items():
                no_prose(v, where + "." + k)
        elif isinstance(x, str):
            assert len(x) <= 200, (where, len(x))
    no_prose(line)
    full = json.load(open(os.path.join(ROOT, "bench_extra.json")))
    assert full["value"] == line["value"] and "single_gpu" in full["extra"] and "decompress" in full["extra"]


def test_a_plain_run_times_the_headline_leg_alone():
    """The plain command (no --full): one short line with the contract's keys and the headline leg through the parity gate, and nothing else --
    no other codec, no CPU baseline, no bench_extra.json."""
    extra = os.path.join(ROOT, "bench_extra.json")
    before = os.stat(extra).st_mtime_ns if os.path.exists(extra) else None
    line = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1"])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline"):
        assert key in line, key
    assert line["metric"] == "input MB/s (lznt1 compress, bit-exact with the reference CPU encoder)" and line["unit"] == "MB/s" and line["dtype"] == "u8"
    assert line["higher_is_better"] is True and line["steps"] == 2 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["config"]["bytes_per_step"] == 3391017280 and 0 < line["roofline"]["frac"] < 1
    assert line["parity_checked"] == {"lznt1": True} and "cpu_baseline" not in line
    assert not [k for k in line["config"] if k.startswith("xpress")], line["config"]
    assert (os.stat(extra).st_mtime_ns if os.path.exists(extra) else None) == before


def test_dump_outputs_writes_what_the_last_step_computed(tmp_path):
    """--dump-outputs DIR: float arrays of the headline leg's last timed step (status, compressed length and checksum per unit, a seeded
    sample of compressed bytes), under 64 MB in all; the lengths of the first replica are the reference's (tests/golden/corpus_full.json)."""
    from ms_compress_amd import corpus
    line = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--no-cpu", "--no-extra", "--dump-outputs", str(tmp_path)])
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    a = {n: np.load(str(tmp_path / (n + ".npy"))) for n in ("status", "compressed_len", "compressed_checksum", "sample_units", "sample_offsets", "sample_bytes")}
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert sum(os.path.getsize(str(p)) for p in tmp_path.iterdir()) <= 64 << 20
    n = len(a["status"])
    assert n == line["config"]["units"] == 192 and (a["status"] == 0).all() and len(a["compressed_len"]) == len(a["compressed_checksum"]) == n
    if corpus.source() == "synthetic":
        gold = json.load(open(os.path.join(ROOT, "tests", "golden", "corpus_full.json")))
        assert a["compressed_len"][:12].tolist() == [gold[name]["lznt1"]["len"] for name in corpus.NAMES]
    assert (a["compressed_len"].reshape(16, 12) == a["compressed_len"][:12]).all()                  # every replica compressed alike
    assert (a["compressed_checksum"].reshape(16, 12) == a["compressed_checksum"][:12]).all()
    u = a["sample_units"].astype(int)
    assert len(u) == min(n, 256) and (np.diff(a["sample_offsets"]) == np.minimum(a["compressed_len"][u], 32768)).all()
    assert len(a["sample_bytes"]) == a["sample_offsets"][-1] and a["sample_bytes"].min() >= 0 and a["sample_bytes"].max() <= 255


def test_two_ranks_share_the_gpu():
    """python bench.py --gpus 2 --oversubscribe: the sharded multi-rank path end to end (self-spawned ranks, gloo timing reduction,
    every rank's shard through the parity gate). One line, marked as a test run."""
    line = _bench(["--gpus", "2", "--oversubscribe", "--steps", "1", "--warmup", "0", "--no-cpu", "--no-extra"])
    assert line["n_gpus"] == 2 and "oversubscribed" in line and line["scaling"] == "strong" and line["config"]["backend"] == "gloo"
    assert line["parity_checked"] == {"lznt1": True}
    assert line["config"]["bytes_per_step"] == 3391017280 and line["config"]["bytes_rank0"] * 2 == 3391017280
    assert line["config"]["lznt1_parity_checked"] is True and line["value"] > 0


def test_rccl_that_cannot_come_up_leaves_a_gloo_job():
    """RCCL asked for (MSCOMP_AMD_BENCH_BACKEND=nccl) with two ranks on ONE GPU -- a communicator with a duplicate device cannot come up: RCCL
    refuses it or, as measured on this stack, never answers --: the bring-up's deadline must fire, the ranks must agree on gloo, finish the job and
    name the backend in the line (sharding.init_distributed)."""
    import torch
    if torch.cuda.device_count() != 1:
        pytest.skip("the duplicate-device refusal needs exactly one visible GPU")
    line = _bench(["--gpus", "2", "--oversubscribe", "--steps", "1", "--warmup", "0", "--no-cpu", "--no-extra"],
                  env={"MSCOMP_AMD_BENCH_BACKEND": "nccl", "MSCOMP_AMD_RCCL_TIMEOUT_S": "30"}, timeout=300)
    assert line["n_gpus"] == 2 and line["parity_checked"] == {"lznt1": True} and line["value"] > 0
    assert line["config"]["backend"].startswith("gloo (nccl failed"), line["config"]["backend"]      # (failed or hung: on this stack two ranks on one GPU sit in communicator creation)


def test_two_ranks_on_two_gpus_over_rccl():
    """python bench.py --gpus 2 exactly as the driver runs it for N = 2 (no test switches): needs two GPUs, runs by itself wherever they are visible"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (%d visible)" % torch.cuda.device_count())
    line = _bench(["--gpus", "2", "--steps", "2", "--warmup", "1", "--no-cpu", "--config5-only"])
    assert line["n_gpus"] == 2 and "oversubscribed" not in line and line["config"]["backend"] in ("nccl",) or line["config"]["backend"].startswith("gloo (nccl failed")
    assert line["parity_checked"] == {"lznt1": True, "xpress": True, "xpress_huff": True} and line["value"] > 0


def test_two_ranks_launched_the_drivers_way():
    """the launch line the driver uses for N > 1 (python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
    --master-port P bench.py --gpus N ...): bench.py is then one of the ranks and must not spawn again; rank 0 prints the one line"""
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--oversubscribe", "--steps", "1", "--warmup", "0", "--no-cpu", "--no-extra"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["parity_checked"] == {"lznt1": True} and line["value"] > 0


def test_three_ranks_all_codecs():
    """three ranks (an uneven split of the 192 / 51 824 units), all three codecs: only rank 0's shard starts at a replica, the job totals must still add up"""
    line = _bench(["--gpus", "3", "--oversubscribe", "--steps", "1", "--warmup", "0", "--no-cpu", "--config5-only"])
    assert line["n_gpus"] == 3
    assert line["parity_checked"] == {"lznt1": True, "xpress": True, "xpress_huff": True}
    for codec in ("lznt1", "xpress", "xpress_huff"):
        assert line["config"]["%s_MB_per_s" % codec] > 0 and line["config"]["%s_roofline_frac" % codec] > 0


def test_parity_gate_on_real_data(tmp_path):
    """Data that is not the synthetic corpus (SILESIA_DIR holds 12 files of the Silesia sizes -- here the synthetic bytes written to disk, so
    the test needs no download): the gate must run the reference's encoder on the host instead of returning None, for all three codecs."""
    from ms_compress_amd import corpus
    saved = os.environ.pop("SILESIA_DIR", None)
    try:
        for i, name in enumerate(corpus.NAMES):
            corpus.file_bytes(i).tofile(str(tmp_path / name))
    finally:
        if saved is not None:
            os.environ["SILESIA_DIR"] = saved
    line = _bench(["--steps", "1", "--warmup", "0", "--no-cpu", "--config5-only"], env={"SILESIA_DIR": str(tmp_path)})
    assert line["data"].startswith("silesia:")
    assert line["parity_checked"] == {"lznt1": True, "xpress": True, "xpress_huff": True}


@pytest.mark.skipif(not os.environ.get("SILESIA_DIR"), reason="SILESIA_DIR not set: the real corpus is not in this image")
def test_parity_gate_on_the_real_silesia_corpus():
    line = _bench(["--steps", "1", "--warmup", "0", "--no-cpu", "--config5-only"])
    assert line["data"].startswith("silesia:")
    assert line["parity_checked"] == {"lznt1": True, "xpress": True, "xpress_huff": True}
