"""bench.py end to end on the GPU (-m gpu), at reduced sizes.

* N = 1, --full: the headline line plus the same-process C1 / C3 / C5 records,
  every record bit-exact against the oracle sample and carrying its own metric,
  roofline and CPU baseline.
* N = 1, plain: the headline alone, and --dump-outputs.
* N = 2, --full, rehearsed on ONE GPU (NFFACL_BENCH_ONE_GPU=1, gloo — RCCL refuses two
  ranks on one device): the root-scattered leg's dist.scatter / dist.gather
  path, whose verdicts must equal rank 0's own classify of the whole batch.
"""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _json_line(stdout: str) -> dict:
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    assert lines, stdout[-2000:]
    return json.loads(lines[-1])


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_bench_n1_with_extra_configs(gpu_available):
    if not gpu_available:
        pytest.skip("no HIP device")
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--full", "--steps", "3", "--warmup", "1",
                        "--packets", str(1 << 18), "--cpu-seconds", "1", "--no-host"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _json_line(r.stdout)
    assert d["metric"].startswith("Mpackets/s device-resident L3 ACL classify, 64B pkts @1k rules")
    assert d["bit_exact_sample"] and d["cpu_baseline"]["bit_exact_vs_gpu"]
    assert set(d["configs"]) == {"c1", "c3", "c5"}
    assert list(d)[-1] == "summary" and d["summary"]["all_bit_exact"]
    assert {"c2", "c1", "c3", "c5"} <= set(d["summary"])
    assert d["configs"]["c1"]["config"]["rules_ip4"] == 4 and d["configs"]["c1"]["config"]["rules_ip6"] == 1
    for c, rec in d["configs"].items():
        assert "@1k rules" not in rec["metric"], rec["metric"]  # labelled per config
        assert rec["bit_exact_sample"] and rec["cpu_baseline"]["bit_exact_vs_gpu"], c
        assert rec["roofline"]["frac"] > 0 and rec["value"] > 0
    # 8 B descriptor + 64 B line + 4 B verdict, plus the second
    # 64 B line of the ~0.3 % of frames whose IP options (IHL >= 12) reach
    # past the first (76.185 B for C3's IMIX mix)
    assert 76.0 < d["configs"]["c3"]["config"]["algorithmic_bytes_per_packet"] < 76.5
    assert d["configs"]["c5"]["config"]["rules_ip4"] + d["configs"]["c5"]["config"]["rules_ip6"] == 100000
    # the C-ABI device group over the same batch: one
    # device = no collective, the Engine's kernel; bit-exact vs the Engine
    grp = d["device_group"]
    assert grp["bit_exact_vs_engine"] and grp["curve"][0]["devices"] == 1
    assert 0.5 < grp["curve"][0]["vs_engine"] < 2.0, grp
    assert d["summary"]["device_group"][0]["devices"] == 1


def test_bench_plain_run_is_lean_and_dumps_its_verdicts(gpu_available, tmp_path):
    """Without --full: the headline only, and --dump-outputs writes the last
    timed launch's verdicts, which must be the oracle's on the seeded batch
    (n is no multiple of 64: the last permit word is partial)."""
    if not gpu_available:
        pytest.skip("no HIP device")
    import numpy as np
    from nffacl import synth
    from oracle import oracle, rules_oracle as ro
    n = (1 << 16) + 37
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2",
                        "--packets", str(n), "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _json_line(r.stdout)
    assert d["metric"].startswith("Mpackets/s device-resident L3 ACL classify, 64B pkts @1k rules")
    assert d["unit"] == "Mpps" and d["higher_is_better"] is True and d["dtype"] == "u32"
    assert d["steps"] == 4 and d["warmup"] == 2 and d["value"] > 0
    # ms_per_step is rounded to 1e-4 ms: <= 1 % of a launch that takes >= 5 us of wall clock
    assert d["value"] == pytest.approx(n / d["ms_per_step"] / 1e3, rel=0.02)
    assert d["roofline"]["frac"] > 0
    assert not {"configs", "cpu_baseline", "device_group", "call_shapes", "host_inclusive", "summary",
                "bit_exact_sample"} & set(d)
    g = synth.gen_rules(synth.SPECS["c2"], synth.RULE_SEEDS["c2"])
    a4, a6 = ro.parse_text_table(g.text.encode()).arrays()
    want = oracle.classify_slots(synth.gen_slots(g, n, synth.PACKET_SEEDS["c2"]), 64, n, a4, a6, threads=8)
    port = np.load(tmp_path / "out" / "port.npy")
    words = np.load(tmp_path / "out" / "permit_bits.npy")
    assert port.dtype == np.float64 and port.shape == (n,) and (port == want).all()
    assert words.dtype == np.float64 and words.shape == ((n + 63) // 64, 2)
    bits = words[:, 0].astype(np.uint64) | words[:, 1].astype(np.uint64) << np.uint64(32)
    permit = np.zeros((n + 63) // 64 * 64, np.uint64)
    permit[:n] = want != 0
    assert (bits == np.bitwise_or.reduce(permit.reshape(-1, 64) << np.arange(64, dtype=np.uint64), axis=1)).all()


def test_bench_two_ranks_one_gpu_scatter(gpu_available):
    if not gpu_available:
        pytest.skip("no HIP device")
    env = dict(os.environ, NFFACL_BENCH_ONE_GPU="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(ROOT / "bench.py"),
           "--full", "--gpus", "2", "--steps", "3", "--warmup", "1", "--packets", str((1 << 18) + 64 * 3),
           "--backend", "gloo", "--no-host"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _json_line(r.stdout)
    assert d["n_gpus"] == 2 and d["ranks"] == 2 and d["backend"] == "gloo" and "rccl_ranks" not in d
    assert d["bit_exact_sample"]
    sc = d["scatter_inclusive"]
    assert sc["bit_exact_vs_local"] and sc["collectives"] == "dist.scatter + dist.gather"
