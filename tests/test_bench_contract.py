"""bench.py contract: one JSON line with the fields the driver reads; the N>1 path is rehearsed with two
ranks on one GPU (`--rehearsal`: bitmap exchange over gloo, since RCCL refuses two ranks per device), here in
the explicit torchrun form the driver uses for N > 1 (tests/test_multi_gpu.py covers the self-launching form)."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _check_line(out, n_gpus):
    lines = [l for l in out.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out
    d = json.loads(lines[0])
    for k in REQUIRED:
        assert k in d, k
    assert d["n_gpus"] == n_gpus and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["data"] == "synthetic" and "workload" in d["config"]
    r = d["roofline"]
    # what binds the dominant kernel is integer VALU issue; achieved / peak / frac stay the tier's nominal HBM figure
    assert r["bound"] == "valu" and r["nominal_bound"] == "hbm" and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["valu_issue_frac"] is None or 0 < r["valu_issue_frac"] <= 1.0
    assert r["pipeline_valu_issue_frac"] is None or 0 < r["pipeline_valu_issue_frac"] <= 1.0
    assert 0 < r["pipeline_frac"] <= r["frac"] and (r["traffic"] is None or r["traffic"] > 0)
    assert d["value"] > 0 and d["ms_per_step"] > 0
    return d


def test_bench_refuses_without_gpu():
    import rsvload
    if rsvload.load_package().device_count() > 0:
        pytest.skip("a HIP device is present")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--proofs", "64"], capture_output=True, text=True)
    assert out.returncode != 0 and "no CPU fallback" in (out.stderr + out.stdout)


@pytest.mark.gpu
def test_bench_single_gpu_line():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--proofs", "2048", "--steps", "2", "--warmup", "1",
                          "--cpu-sample", "64", "--perm-log2", "16"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    d = _check_line(out.stdout, 1)
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["cores"] >= 1 and d["cpu_baseline"]["value"] > 0
    assert 4000 < d["cpu_baseline"]["perms_per_proof"] < 6000
    assert d["cpu_baseline"]["one_thread"]["value"] > 0 and d["cpu_baseline"]["one_thread"]["cores"] == 1 and d["cpu_baseline"]["cpu_model"]
    # the headline CPU figure uses every CPU the process may use (all host cores; min of logical CPUs,
    # affinity and cgroup quota), and says what it found
    share = d["cpu_baseline"]["cpu_share"]
    assert share["usable_cpus"] >= 1 and d["cpu_baseline"]["cores"] == min(share["usable_cpus"], 64)
    assert d["host_path"]["value"] > 0 and d["host_path"]["GBps"] > 0  # PCIe-inclusive rate, reported beside `value`
    assert d["host_path"]["pinned_arena"]["GBps"] > 0                   # the same from an rsv_host_alloc arena (no gather copy)
    assert 0 < d["single_proof"]["min_ms"] <= d["single_proof"]["latency_ms"] < 50   # one proof per call: the reference's own use
    assert d["config"]["exchange"]["world_size"] == 1 and len(d["config"]["exchange"]["devices"]) == 1
    v = d["valu"]
    assert 0 < v["frac_of_ceiling"] <= 1.0 and 0 < v["pipeline_frac_of_ceiling"] <= 1.0
    assert v["ceiling_perms_per_s"] > v["poseidon2_perms_per_s"] > 1e9
    e = d["emulated_poseidon2"]
    assert e["bound"] == "hbm" and 0 < e["frac"] <= 1.0 and e["algorithmic_bytes_per_perm"] == 65 + 416 * 16
    w = d["recursion_circuit_witness"]
    assert w["proofs"] == 1024 and w["variables_per_proof"] == 47788 and w["levels"] > 100 and w["proofs_per_s"] > 1e4
    assert w["cpu_baseline"]["kind"] == "port" and 0 < w["cpu_baseline"]["value"] < w["proofs_per_s"]


@pytest.mark.gpu
def test_bench_two_ranks_rehearsal():
    env = dict(os.environ)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--rehearsal", "--proofs", "2048",
           "--steps", "2", "--warmup", "1", "--cpu-sample", "0", "--perm-log2", "0"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    d = _check_line(out.stdout, 2)
    assert d["config"]["parallelism"] == "shard2"


def test_committed_profile_holds_the_large_batch_line():
    """VERDICT r3 #6 — hold, don't dig: the committed profile of the default workload (profiles/pmc_latest.json, written by
    tools/profile.sh + tools/pmc_summary.py from a gpurun of `python bench.py` on one MI355X) must show >= 1.90 M proofs/s
    and <= 2.6 x the algorithmic bytes in HBM traffic over the pipeline; a change that costs the large batch more than
    that does not get committed with a fresh profile."""
    with open(os.path.join(ROOT, "profiles", "pmc_latest.json")) as f:
        prof = json.load(f)
    if "pipeline_traffic_ratio" not in prof:
        pytest.skip("profile written before round 4")
    assert prof["proofs"] == 65536 and prof["bench_value_proofs_per_s"] >= 1.90e6, prof["bench_value_proofs_per_s"]
    assert prof["pipeline_traffic_ratio"] <= 2.6, prof["pipeline_traffic_ratio"]
    dom = prof["kernels"]["k_pair_merkle"]
    # the FRI trees' span: 21-22 ms while k_query ended ~8 ms into the step; ~25 since it ends at ~4.5 ms and the trees start
    # beside the trace trees that much earlier (same step time: the whole-step figure below is the one that must hold)
    assert dom["avg_ms"] < 27.0 and dom["SQ_INSTS_VALU"] > 1e10
    if "pipeline_valu_insts" in prof:
        frac = prof["pipeline_valu_insts"] / (prof["bench_ms_per_step"] * 1e-3) / (1024 * 2.4e9 / 2.0)
        assert 0.5 <= frac <= 1.0, frac
    # the evidence is ONE build — the profile and the large soak carry the hash of the same kernel sources
    # (tests/soak.py prints it; tools/round5_artifacts.sh runs the soak last), and those are the committed sources
    tag = prof["tag"].split("_")[0]
    soak = os.path.join(ROOT, "profiles", f"{tag}_soak_large.txt")
    if tag >= "r5":
        import re
        shas = set(re.findall(r"kernel sources ([0-9a-f]{16})", open(soak).read()))
        assert shas == {prof["kernel_sources_sha"]}, (shas, prof["kernel_sources_sha"])
        sys.path.insert(0, ROOT)
        import bench
        assert bench.kernel_sources_sha() == prof["kernel_sources_sha"], "profiles/ were taken on other kernel sources than the committed ones"


def test_dump_outputs_writes_a_fixed_bounded_sample(tmp_path, monkeypatch):
    """--dump-outputs: float64 .npy files, exact 32-bit words, within the size limit; every group of arrays over proofs that
    does not fit is cut to one seeded sample of its proofs (<group>_sample.npy), the same on every call."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 16)
    n = 1024
    accept = (np.arange(n) % 17 != 5).astype(np.uint8)
    words = np.random.default_rng(1).integers(-2 ** 31, 2 ** 31, size=(n, 3, 2), dtype=np.int32)
    job = np.tile(accept, 4)
    samples = []
    for k in range(2):
        d = str(tmp_path / f"out{k}")
        bench.dump_outputs(d, {"accepted_count": np.array([int(job.sum())])},
                           {"proof": {"accept": accept, "flow": words}, "job": {"job_accept": job}})
        files = sorted(os.listdir(d))
        assert files == ["accept.npy", "accepted_count.npy", "flow.npy", "job_accept.npy", "job_sample.npy", "proof_sample.npy"]
        got = {f[:-4]: np.load(os.path.join(d, f)) for f in files}
        assert all(a.dtype == np.float64 for a in got.values())
        assert sum(a.size * 8 for a in got.values()) <= 1 << 16
        s, j = got["proof_sample"].astype(np.int64), got["job_sample"].astype(np.int64)
        assert 0 < len(s) < n and np.all(np.diff(s) > 0) and 0 < len(j) < len(job) and np.all(np.diff(j) > 0)
        assert np.array_equal(got["accept"], accept[s]) and np.array_equal(got["flow"], words[s].view(np.uint32))
        assert np.array_equal(got["job_accept"], job[j]) and got["accepted_count"].tolist() == [job.sum()]
        samples.append((s, j))
    assert all(np.array_equal(x, y) for x, y in zip(*samples))
    # what fits is written whole, without a sample
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 20)
    d = str(tmp_path / "whole")
    bench.dump_outputs(d, {}, {"proof": {"accept": accept, "flow": words}, "job": {"job_accept": job}})
    assert sorted(os.listdir(d)) == ["accept.npy", "flow.npy", "job_accept.npy"]
    assert np.array_equal(np.load(os.path.join(d, "flow.npy")), words.view(np.uint32))


# a fresh child process: bench.main() with ShardedVerifier.step counted, then the number of calls on the last line
_COUNT_STEPS = """
import sys
sys.path.insert(0, sys.argv[1])
import rsvload
rsvload.load_package()
from recursive_stwo_amd import sharding
calls = [0]
step = sharding.ShardedVerifier.step
def counted(self, *a, **k):
    calls[0] += 1
    return step(self, *a, **k)
sharding.ShardedVerifier.step = counted
import bench
sys.argv = ["bench.py"] + sys.argv[2:]
bench.main()
print("step calls", calls[0])
"""


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [["--emit-flow"], ["--workload", "copies", "--emit-paths"]], ids=["flow", "paths"])
def test_bench_dump_outputs_are_the_timed_steps_outputs(tmp_path, extra):
    """--steps K --warmup W runs the verifying step K + W times; --dump-outputs DIR then holds the last step's accept / reason
    bytes, the job's gathered accept vector and the hint outputs, identical from run to run with the same arguments (with
    --emit-flow on the mixed-shape workload, the flow rows past a proof's own count included)."""
    import numpy as np
    runs = []
    for k in range(2):
        d = str(tmp_path / f"out{k}")
        out = subprocess.run([sys.executable, "-c", _COUNT_STEPS, ROOT, "--proofs", "512", "--steps", "3", "--warmup", "2",
                              "--cpu-sample", "0", "--perm-log2", "0", "--no-single-proof", "--dump-outputs", d] + extra,
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        assert out.stdout.strip().splitlines()[-1] == "step calls 5", out.stdout[-500:]
        line = _check_line(out.stdout, 1)
        assert line["steps"] == 3 and line["warmup"] == 2
        got = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 << 20
        assert all(a.dtype == np.float64 for a in got.values())
        s = got["proof_sample"].astype(np.int64) if "proof_sample" in got else np.arange(512)
        j = got["job_sample"].astype(np.int64) if "job_sample" in got else np.arange(512)
        want = (np.arange(512) % 17 != 5).astype(np.float64)
        assert np.array_equal(got["accept"], want[s]) and np.array_equal(got["job_accept"], want[j])
        assert got["accepted_count"].tolist() == [want.sum()] and np.all((got["reason"] == 0) == (want[s] == 1))
        if "flow" in got:
            count = got["flow_count"].astype(np.int64)
            assert count.max() > 0 and count.min() < got["flow"].shape[1]  # mixed shapes: rows past the count exist
            past = np.arange(got["flow"].shape[1])[None, :] >= count[:, None]
            assert not got["flow"][past].any() and not got["flow_swap"][past].any()
        else:
            assert {"transcript", "trace_sib", "fri_sib"} <= set(got)
        runs.append(got)
    assert sorted(runs[0]) == sorted(runs[1])
    for name in runs[0]:
        assert np.array_equal(runs[0][name], runs[1][name]), name
