#!/usr/bin/env python3
"""Time of rsv_witness_decommit_dev (the openings of trees 0, 1 and 2 of the next proof at n_queries positions) beside the
commitment of the same trees at the same commit, one JSON line.

    python tools/bench_decommit.py --fixture level9-1.bin --log-blowup 8 --queries 16 --proofs 1 --steps 5

There is no earlier opening to compare with, so the yardstick is rsv_witness_commit_caps_dev on the same buffers: the three
calls (commitment, opening without caps, opening with caps) are timed interleaved, `--steps` rounds.  Without caps the
opening recomputes every block, about one commitment without the interaction columns; with caps only the blocks the queries
touch, `touched_blocks` of 2^log_blowup per tree (counted on the host from the positions, per proof: the queries are random
and differ per proof), plus the plan and gather launches.  For a per-kernel split run the tool under
`rocprofv3 --kernel-trace --stats -- python tools/bench_decommit.py ...`."""
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
    ap.add_argument("--queries", type=int, default=16)
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
    n, b, nq = args.proofs, args.log_blowup, args.queries
    top = max(lp, lq) + b
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
    d_caps = z(n, 3, 2 << b, 8)
    vcaps, wcap = rsv.witness_decommit_sizes(wp, b, nq)
    q = np.random.default_rng(1).integers(0, 1 << top, (n, nq)).astype(np.uint32)
    d_q = torch.from_numpy(q.view(np.int32)).to(dev)
    d_v, d_nv, d_w, d_nw = z(n, sum(vcaps)), z(n, 3), z(n, 3, wcap, 8), z(n, 3)
    touched = [len(set((row >> (top - b)).tolist())) for row in q]
    calls = {
        "commit": lambda: ctx.witness_commit(wp, d_plonk, d_pos, d_ops, d_acc, n, b, d_roots, d_draws, d_ip, d_iq, d_sums, d_ok=d_ok, d_caps=d_caps),
        "open_no_caps": lambda: ctx.witness_decommit(wp, d_plonk, d_pos, d_ops, d_ip, d_iq, d_acc, n, b, d_q, nq, d_v, d_nv, d_w, d_nw, d_ok=d_ok),
        "open_caps": lambda: ctx.witness_decommit(wp, d_plonk, d_pos, d_ops, d_ip, d_iq, d_acc, n, b, d_q, nq, d_v, d_nv, d_w, d_nw, d_ok=d_ok,
                                                  d_caps=d_caps),
    }
    for _ in range(max(args.warmup, 1)):
        for call in calls.values():
            call()
    ctx.synchronize()
    stream = torch.cuda.ExternalStream(ctx.stream) if ctx.stream else torch.cuda.current_stream()
    times = {k: [] for k in calls}
    for _ in range(args.steps):
        for name, call in calls.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            call()
            t1.record(stream)
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1))
    med = {k: float(np.median(v)) for k, v in times.items()}
    share = float(np.mean(touched)) / (1 << b)
    print(json.dumps({"tool": "bench_decommit", "fixture": args.fixture, "log_plonk": lp, "log_poseidon": lq, "log_blowup": b, "proofs": n,
                      "queries": nq, "ok": int(d_ok.sum().item()), "touched_blocks_mean": round(float(np.mean(touched)), 2),
                      "block_share": round(share, 4), "n_values": d_nv[0].cpu().tolist(), "n_witness": d_nw[0].cpu().tolist(),
                      "ms": {k: round(v, 3) for k, v in med.items()}, "ms_all": {k: [round(t, 3) for t in v] for k, v in times.items()},
                      "open_caps_over_commit": round(med["open_caps"] / med["commit"], 4),
                      "open_no_caps_over_commit": round(med["open_no_caps"] / med["commit"], 4)}))
    ctx.close()
    wp.close()


if __name__ == "__main__":
    main()
