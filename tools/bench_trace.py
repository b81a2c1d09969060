#!/usr/bin/env python3
"""Throughput of rsv_witness_trace_dev (the recursion circuit's 60 trace columns for a batch), one JSON line.

    python tools/bench_trace.py --fixture level10-1.bin --proofs 1024 --steps 5 [--copies 1] [--layout by_proof]

The batch is `--proofs` copies of the fixture, every 17th with one flipped bit (rejected: zero columns, the same bytes).
`variables` and the PoseidonFlow are put in HBM once by rsv_witness_eval_dev; timed are the trace call alone, its Plonk
part alone (d_poseidon NULL: k_trace_plonk) and its Poseidon part alone (d_plonk NULL: k_trace_poseidon + the zero tail),
and the eval and the trace together.  roofline: HBM-write bound — bytes written per proof = 12 x 4 x 2^lp (Plonk) +
48 x 4 x 2^lq (Poseidon) + 4 per witness op; achieved = those bytes x proofs / time, against 8 TB/s.  For a per-kernel split
from the profiler, run the tool under `rocprofv3 --kernel-trace --stats -- python tools/bench_trace.py ...`."""
import argparse
import json
import time

import numpy as np
from chain_bench import open_fixture

PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fixture", default="level10-1.bin")
    ap.add_argument("--proofs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--copies", type=int, default=1)
    ap.add_argument("--layout", choices=["by_proof", "by_variable"], default="by_proof", help="RSV_OPT_WITNESS_LAYOUT of d_variables")
    args = ap.parse_args()
    rsv, proof, cfg, inputs = open_fixture(args)
    import torch
    import bench
    wp = rsv.WitnessProgram.build(proof, cfg, inputs, copies=args.copies)
    lp, lq = wp.trace_sizes()
    n_ops = len(wp.gates()[1])
    F = wp.shape.flow_count
    n = args.proofs
    dev = torch.device("cuda:0")
    batch = [proof] * n
    tampered = list(range(5, n, 17))
    for i in tampered:
        b = bytearray(proof)
        b[4000 + (i * 7919) % (len(proof) - 8000)] ^= 1
        batch[i] = bytes(b)
    blob, offsets = rsv.pack(batch)
    d_blob, d_off = torch.from_numpy(blob.copy()).to(dev), torch.from_numpy(offsets.astype(np.int64)).to(dev)
    shape = (wp.n_vars, n, 4) if args.layout == "by_variable" else (n, wp.n_vars, 4)
    d_vars = torch.empty(shape, dtype=torch.int32, device=dev)
    d_flow = torch.empty((n, F, 32), dtype=torch.int32, device=dev)
    d_swap = torch.empty((n, F), dtype=torch.uint8, device=dev)
    d_acc = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_plonk = torch.empty((n, 12, 1 << lp), dtype=torch.int32, device=dev)
    d_pos = torch.empty((n, 48, 1 << lq), dtype=torch.int32, device=dev)
    d_ops = torch.empty((n, max(n_ops, 1)), dtype=torch.int32, device=dev)
    ctx = rsv.Context(0)
    ctx.set_option("witness_layout", args.layout)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ctx.synchronize()
        t = time.perf_counter()
        for _ in range(args.steps):
            fn()
        ctx.synchronize()
        return (time.perf_counter() - t) / args.steps * 1e3

    def ev():
        ctx.witness(wp, d_blob, d_off, n, d_vars, d_acc, inputs=inputs, d_flow=d_flow, d_flow_swap=d_swap)

    def tr(plonk=True, poseidon=True, ops=True):
        ctx.witness_trace(wp, d_vars, d_acc, n, d_plonk=d_plonk if plonk else None, d_poseidon=d_pos if poseidon else None,
                          d_ops=d_ops if ops else None, d_flow=d_flow, d_flow_swap=d_swap)

    ev()
    ctx.synchronize()
    acc = d_acc.cpu().numpy()
    want = np.ones(n, np.uint8)
    want[tampered] = 0
    if not np.array_equal(acc, want):
        raise SystemExit("verdict mismatch")
    trace_ms = timed(tr)
    plonk_ms = timed(lambda: tr(poseidon=False, ops=False))
    poseidon_ms = timed(lambda: tr(plonk=False, ops=False))
    both_ms = timed(lambda: (ev(), tr()))
    b_plonk, b_pos, b_ops = 48 * (1 << lp), 192 * (1 << lq), 4 * n_ops
    gbs = lambda b, ms: b * n / (ms * 1e-3) / 1e9
    print(json.dumps({
        "metric": "recursion_circuit_traces_per_s", "value": n / (trace_ms * 1e-3), "unit": "proofs/s", "n_gpus": 1, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": trace_ms, "higher_is_better": True, "dtype": "u32 (M31)", "data": "synthetic",
        "config": {"workload": f"trace columns of the circuit verifying {args.fixture} x{args.copies}", "proofs": n, "layout": args.layout,
                   "log_plonk": lp, "log_poseidon": lq, "poseidon_invocations": F * args.copies, "witness_ops": n_ops,
                   "bytes_written_per_proof": {"plonk": b_plonk, "poseidon": b_pos, "ops": b_ops, "total": b_plonk + b_pos + b_ops}},
        "split_ms": {"trace": trace_ms, "plonk_only": plonk_ms, "poseidon_only": poseidon_ms, "eval_and_trace": both_ms},
        "roofline": {"bound": "hbm", "achieved": gbs(b_plonk + b_pos + b_ops, trace_ms), "peak": PEAK_GBS, "unit": "GB/s",
                     "frac": gbs(b_plonk + b_pos + b_ops, trace_ms) / PEAK_GBS,
                     "plonk": {"achieved": gbs(b_plonk, plonk_ms), "frac": gbs(b_plonk, plonk_ms) / PEAK_GBS},
                     "poseidon": {"achieved": gbs(b_pos, poseidon_ms), "frac": gbs(b_pos, poseidon_ms) / PEAK_GBS},
                     "note": "bytes written only (the Plonk gathers read 3 x 16 B per row, mostly from L2; the flow is 64 B per invocation)"},
        "kernel_sources_sha": bench.kernel_sources_sha()}))


if __name__ == "__main__":
    main()
