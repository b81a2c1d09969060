#!/usr/bin/env python3
"""Time of rsv_witness_sample_dev (sampled_values[0..2] of the next proof at the OODS point) and of rsv_sample_tree_dev
from coefficients, beside the commitment of the same trees at the same commit, one JSON line.

    python tools/bench_sample.py --fixture level9-1.bin --log-blowup 8 --proofs 1 --steps 5

Timed interleaved, `--steps` rounds, HIP events on the context's stream, medians:
  commit         rsv_witness_commit_dev on the chain's buffers (the yardstick; it interpolates the same 126 columns);
  sample         rsv_witness_sample_dev: interpolation in the workspace (RSV_SAMPLE_COLUMNS) + the dot products;
  coeffs_t1, t2  rsv_sample_tree_dev with RSV_SAMPLE_COEFFS on the per-proof buffers of trees 1 (60 columns, one point) and
                 2 (16 columns, two points), read as coefficients (any canonical words are; the traffic is what a
                 commitment's d_coeffs would give): 4 bytes per coefficient, `coeffs_share_of_8TBs` = that over the time
                 over the 8 TB/s peak;
  coeffs_t0      the same on tree 0's 50 columns, 49 of them one set shared by every proof (mostly cache traffic).
The interpolation alone is the k_cm_fft_* rows of `rocprofv3 --kernel-trace --stats -- python tools/bench_sample.py ...`."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fixture", default="level9-1.bin")
    ap.add_argument("--log-blowup", type=int, default=8)
    ap.add_argument("--proofs", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--copies", type=int, default=1)
    args = ap.parse_args()
    import rsvload
    rsv = rsvload.load_package()
    import torch
    import bench
    with open(os.path.join(ROOT, "tests", "golden", "manifest.json")) as f:
        man = {e["file"]: e for e in json.load(f)["proofs"]}
    e = man[args.fixture]
    inputs = [(i, tuple(v)) for i, v in e["inputs"]]
    cfg = rsv.PcsConfig(e["pow_bits"], e["log_blowup_factor"], e["log_last_layer_degree_bound"], e["n_queries"])
    proof = bench.read_fixture(args.fixture)
    wp = rsv.WitnessProgram.build(proof, cfg, inputs, copies=args.copies)
    lp, lq = wp.trace_sizes()
    F = wp.shape.flow_count
    n_ops = len(wp.gates()[1])
    n, b = args.proofs, args.log_blowup
    dev = torch.device("cuda:0")
    blob, offsets = rsv.pack([proof] * n)
    ctx = rsv.Context(0)
    d_blob, d_off = torch.from_numpy(blob.copy()).to(dev), torch.from_numpy(offsets.astype(np.int64)).to(dev)
    d_vars = torch.zeros((n, wp.n_vars, 4), dtype=torch.int32, device=dev)
    d_flow = torch.zeros((n, F, 32), dtype=torch.int32, device=dev)
    d_swap = torch.zeros((n, F), dtype=torch.uint8, device=dev)
    d_acc = torch.zeros(n, dtype=torch.uint8, device=dev)
    ctx.witness(wp, d_blob, d_off, n, d_vars, d_acc, inputs=inputs, d_flow=d_flow, d_flow_swap=d_swap)
    d_plonk = torch.zeros((n, 12, 1 << lp), dtype=torch.int32, device=dev)
    d_pos = torch.zeros((n, 48, 1 << lq), dtype=torch.int32, device=dev)
    d_ops = torch.zeros((n, max(n_ops, 1)), dtype=torch.int32, device=dev)
    ctx.witness_trace(wp, d_vars, d_acc, n, d_plonk=d_plonk, d_poseidon=d_pos, d_ops=d_ops, d_flow=d_flow, d_flow_swap=d_swap)
    del d_vars, d_flow, d_swap, d_blob
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
    d_roots, d_draws, d_ip, d_iq, d_sums = z(n, 3, 8), z(n, 12), z(n, 8, 1 << lp), z(n, 8, 1 << lq), z(n, 2, 4)
    d_ok = torch.zeros(n, dtype=torch.uint8, device=dev)
    rng = np.random.default_rng(1)
    d_oods = torch.from_numpy(rng.integers(0, 0x7FFFFFFF, (n, 8)).astype(np.int32)).to(dev)
    d_pts2 = torch.from_numpy(rng.integers(0, 0x7FFFFFFF, (n, 2, 8)).astype(np.int32)).to(dev)
    d_samples = z(n, 134, 4)
    ppre, qpre = wp.preprocessed()
    d_ppre = torch.from_numpy(np.ascontiguousarray(ppre, dtype=np.uint32).view(np.int32)).to(dev)
    d_qpre = torch.from_numpy(np.ascontiguousarray(qpre, dtype=np.uint32).view(np.int32)).to(dev)
    t0 = [{"log_size": lp, "d_cols": d_ppre, "n_cols": 10, "proof_stride": 0}, {"log_size": lq, "d_cols": d_qpre, "n_cols": 40, "proof_stride": 0}]
    t1 = [{"log_size": lp, "d_cols": d_plonk, "n_cols": 12}, {"log_size": lq, "d_cols": d_pos, "n_cols": 48}]
    t2 = [{"log_size": lp, "d_cols": d_ip, "n_cols": 8}, {"log_size": lq, "d_cols": d_iq, "n_cols": 8}]
    o0, o1, o2 = z(n, 1, 50, 4), z(n, 1, 60, 4), z(n, 2, 16, 4)
    calls = {
        "commit": lambda: ctx.witness_commit(wp, d_plonk, d_pos, d_ops, d_acc, n, b, d_roots, d_draws, d_ip, d_iq, d_sums, d_ok=d_ok),
        "sample": lambda: ctx.witness_sample(wp, d_plonk, d_pos, d_ops, d_ip, d_iq, d_acc, n, d_oods, d_samples, d_ok=d_ok),
        "coeffs_t0": lambda: ctx.sample_tree(t0, n, d_oods, 1, o0, d_mask=d_ok, source=rsv.SAMPLE_COEFFS),
        "coeffs_t1": lambda: ctx.sample_tree(t1, n, d_oods, 1, o1, d_mask=d_ok, source=rsv.SAMPLE_COEFFS),
        "coeffs_t2": lambda: ctx.sample_tree(t2, n, d_pts2, 2, o2, d_mask=d_ok, source=rsv.SAMPLE_COEFFS),
    }
    for _ in range(max(args.warmup, 1)):
        for call in calls.values():
            call()
    ctx.synchronize()
    stream = torch.cuda.ExternalStream(ctx.stream) if ctx.stream else torch.cuda.current_stream()
    times = {k: [] for k in calls}
    for _ in range(args.steps):
        for name, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    med = {k: float(np.median(v)) for k, v in times.items()}
    ok = int(d_ok.sum().item())
    coeff_bytes = 4 * ok * ((12 + 8) * (1 << lp) + (48 + 8) * (1 << lq))  # trees 1 and 2, every word once
    coeff_ms = med["coeffs_t1"] + med["coeffs_t2"]
    print(json.dumps({"tool": "bench_sample", "fixture": args.fixture, "log_plonk": lp, "log_poseidon": lq, "log_blowup": b, "proofs": n, "ok": ok,
                      "ms": {k: round(v, 4) for k, v in med.items()}, "ms_all": {k: [round(t, 4) for t in v] for k, v in times.items()},
                      "coeffs_t1_t2_bytes": coeff_bytes, "coeffs_t1_t2_ms": round(coeff_ms, 4),
                      "coeffs_share_of_8TBs": round(coeff_bytes / (coeff_ms * 1e-3) / 8e12, 4) if coeff_ms > 0 else None,
                      "sample_over_commit": round(med["sample"] / med["commit"], 5)}))
    ctx.close()
    wp.close()


if __name__ == "__main__":
    main()
