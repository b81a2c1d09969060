#!/usr/bin/env python3
"""Throughput of rsv_witness_interaction_dev (the recursion circuit's 16 interaction columns and two claimed sums for a
batch), one JSON line.

    python tools/bench_interaction.py --fixture level10-1.bin --proofs 1024 --steps 5 [--copies 1]

The batch is `--proofs` copies of the fixture, every 17th with one flipped bit (rejected: zero columns), each proof with
its own random lookup elements (z, alpha).  The trace columns are put in HBM once (rsv_witness_eval_dev +
rsv_witness_trace_dev); timed is the interaction call alone.  Bytes per proof are ALGORITHMIC: the trace words the
relations read (12 Plonk and 33 of the 48 Poseidon columns) plus the 16 columns and the sums written; the preprocessed
columns are one copy per program (shared by the batch, L2 / MALL resident) and listed apart.  `moved` adds what the kernels
move on top: f0 + f1 parked in column 1, read by the chunk sums and by the scan, and written again (64 B per row).
`roofline.bound` is whichever of HBM (bytes moved) and VALU issue is the larger fraction of its peak over the call.  The
VALU side is the call's wave64 VALU instructions per accepted proof for this shape (profiles/interaction_valu.json,
tools/interaction_valu.py from an `rocprofv3 --pmc SQ_INSTS_VALU` pass, keyed by the hash of the kernel sources) times
this run's accepted proofs, against one instruction per 2 cycles per SIMD at 2.4 GHz, bench.py's nominal rate; a stale
file or an unprofiled shape leaves the bound null.  For a per-kernel split run the tool under
`rocprofv3 --kernel-trace --stats -- python tools/bench_interaction.py ...`."""
import argparse
import json
import os
import time

import numpy as np
from chain_bench import open_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_GBS = 8000.0
SIMDS, GHZ = 1024, 2.4
VALU_FILE = os.path.join(ROOT, "profiles", "interaction_valu.json")
P = 0x7FFFFFFF


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fixture", default="level10-1.bin")
    ap.add_argument("--proofs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--copies", type=int, default=1)
    args = ap.parse_args()
    rsv, proof, cfg, inputs = open_fixture(args)
    import torch
    import bench
    wp = rsv.WitnessProgram.build(proof, cfg, inputs, copies=args.copies)
    lp, lq = wp.trace_sizes()
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
    d_vars = torch.empty((n, wp.n_vars, 4), dtype=torch.int32, device=dev)
    d_flow = torch.empty((n, F, 32), dtype=torch.int32, device=dev)
    d_swap = torch.empty((n, F), dtype=torch.uint8, device=dev)
    d_acc = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_plonk = torch.empty((n, 12, 1 << lp), dtype=torch.int32, device=dev)
    d_pos = torch.empty((n, 48, 1 << lq), dtype=torch.int32, device=dev)
    lookup = np.random.default_rng(1).integers(0, P, (n, 8)).astype(np.uint32)
    d_lookup = torch.from_numpy(lookup.view(np.int32)).to(dev)
    d_ip = torch.empty((n, 8, 1 << lp), dtype=torch.int32, device=dev)
    d_iq = torch.empty((n, 8, 1 << lq), dtype=torch.int32, device=dev)
    d_sums = torch.empty((n, 2, 4), dtype=torch.int32, device=dev)
    d_ok = torch.empty(n, dtype=torch.uint8, device=dev)
    ctx = rsv.Context(0)
    ctx.witness(wp, d_blob, d_off, n, d_vars, d_acc, inputs=inputs, d_flow=d_flow, d_flow_swap=d_swap)
    ctx.witness_trace(wp, d_vars, d_acc, n, d_plonk=d_plonk, d_poseidon=d_pos, d_flow=d_flow, d_flow_swap=d_swap)
    ctx.synchronize()
    want = np.ones(n, np.uint8)
    want[tampered] = 0
    if not np.array_equal(d_acc.cpu().numpy(), want):
        raise SystemExit("verdict mismatch")

    def call():
        ctx.witness_interaction(wp, d_plonk, d_pos, d_acc, d_lookup, n, d_ip, d_iq, d_sums, d_ok)

    for _ in range(args.warmup):
        call()
    ctx.synchronize()
    if not np.array_equal(d_ok.cpu().numpy(), want):
        raise SystemExit("ok mismatch")
    t = time.perf_counter()
    for _ in range(args.steps):
        call()
    ctx.synchronize()
    ms = (time.perf_counter() - t) / args.steps * 1e3
    N, Q = 1 << lp, 1 << lq
    read = 4 * (12 * N + 33 * Q)
    written = 4 * 8 * (N + Q) + 32
    moved = read + written + 64 * (N + Q)
    gbs = lambda b: b * n / (ms * 1e-3) / 1e9
    accepted = n - len(tampered)
    valu_frac, valu_note = None, "profiles/interaction_valu.json missing"
    try:
        with open(VALU_FILE) as f:
            vf = json.load(f)
        shape = vf["shapes"].get(f"{lp}/{lq}")
        if vf["kernel_sources_sha"] != bench.kernel_sources_sha():
            valu_note = f"profiles/interaction_valu.json was taken on other kernel sources ({vf['kernel_sources_sha']})"
        elif shape is None:
            valu_note = f"shape {lp}/{lq} not in profiles/interaction_valu.json"
        else:
            valu_frac = accepted * shape["total"] / (ms * 1e-3) / (SIMDS * GHZ * 1e9 / 2.0)
            valu_note = f"VALU instructions per accepted proof from {vf['tag']}"
    except (OSError, KeyError, ValueError):
        pass
    hbm_frac = gbs(moved) / PEAK_GBS
    bound = None if valu_frac is None else ("valu" if valu_frac > hbm_frac else "hbm")
    print(json.dumps({
        "metric": "recursion_circuit_interactions_per_s", "value": n / (ms * 1e-3), "unit": "proofs/s", "n_gpus": 1, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": ms, "higher_is_better": True, "dtype": "u32 (M31)", "data": "synthetic",
        "config": {"workload": f"interaction columns of the circuit verifying {args.fixture} x{args.copies}", "proofs": n,
                   "log_plonk": lp, "log_poseidon": lq, "rejected": len(tampered)},
        "bytes_per_proof": {"read": read, "written": written, "algorithmic": read + written, "moved": moved,
                            "preprocessed_shared": 4 * 8 * (N + Q)},
        "roofline": {"bound": bound, "achieved_algorithmic": gbs(read + written), "achieved_moved": gbs(moved), "peak": PEAK_GBS,
                     "unit": "GB/s", "frac_algorithmic": gbs(read + written) / PEAK_GBS, "frac_moved": hbm_frac,
                     "valu_issue_frac": valu_frac, "valu_note": valu_note},
        "kernel_sources_sha": bench.kernel_sources_sha()}))


if __name__ == "__main__":
    main()
