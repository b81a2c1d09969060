#!/usr/bin/env python3
"""rsv_circuit_check_dev / rsv_circuit_flow_dev beside rsv_witness_trace_dev's two parts, in one session: the fixture's own
recursion circuit (default level10-1.bin) as a CREATED program (rsv.Circuit of the built program's gate list, flow wires and
witness ops) over the variables and the flow the built program's witness left, for 1, 16 and 1 024 proofs.  Times are HIP
events on the context's stream around each call, interleaved (tools/chain_bench.py).  Per call: the bytes the algorithm
needs — k_uc_gates 16 B of row table + 12 B of wires + 3 x 16 B gathered per row, k_uc_flow 48 B of table + 128 B gathered +
128 B record per invocation, k_trace_plonk 12 B + 48 B gathered + 48 B stored per PADDED row, k_trace_poseidon 128 B read +
1 152 B stored per padded invocation — over the call's time.  One JSON line per batch size.

    python tools/bench_user_circuit.py [--fixture level10-1.bin] [--sizes 1,16,1024] [--steps 20] [--warmup 3]"""
import argparse
import json

import numpy as np

import chain_bench as CB


def main():
    ap = argparse.ArgumentParser()
    CB.add_args(ap, "level10-1.bin", 1)
    ap.add_argument("--sizes", default="1,16,1024")
    ap.set_defaults(steps=20, warmup=3)
    args = ap.parse_args()
    import torch
    rsv, proof, cfg, inputs = CB.open_fixture(args)
    if rsv.device_count() < 1:
        raise SystemExit("bench_user_circuit needs a HIP device")
    wp = rsv.WitnessProgram.build(proof, cfg, inputs)
    gates, ops = wp.gates()
    wires = np.ascontiguousarray(wp.export().flow_wires, dtype=np.uint32)
    circ = rsv.Circuit(gates, wires, wp.n_vars, 3, ops)
    lp, lq = circ.trace_sizes()
    n_rows, n_flow = len(gates), len(wires)
    n_pad = max(32, -(-n_flow // 16) * 16)
    ctx = rsv.Context(0)
    for n in (int(x) for x in args.sizes.split(",")):
        src = rsv.Chain(ctx, wp, n, args.log_blowup)
        src.witness([proof] * n, inputs)
        ctx.synchronize()
        d_vars, d_flow, d_swap = src._vars, src._flow, src._swap
        ok = torch.ones(n, dtype=torch.uint8, device="cuda:0")
        bad = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        plonk = torch.zeros((n, 12, 1 << lp), dtype=torch.int32, device="cuda:0")
        poseidon = torch.zeros((n, 48, 1 << lq), dtype=torch.int32, device="cuda:0")
        calls = {
            "circuit_check": lambda: ctx.circuit_check(circ, d_vars, n, ok, bad),
            "circuit_flow": lambda: ctx.circuit_flow(circ, d_vars, n, d_flow, d_swap, ok, bad),
            "trace_plonk": lambda: ctx.witness_trace(circ, d_vars, ok, n, d_plonk=plonk),
            "trace_poseidon": lambda: ctx.witness_trace(circ, None, ok, n, d_poseidon=poseidon, d_flow=d_flow, d_flow_swap=d_swap),
        }
        times, med = CB.time_interleaved(ctx, calls, args.steps, args.warmup)
        ctx.synchronize()
        assert ok.cpu().numpy().all() and (bad.cpu().numpy().view(np.uint32) == 0xFFFFFFFF).all(), "the fixture's own witness failed a check"
        need = {"circuit_check": n * n_rows * (16 + 12 + 48), "circuit_flow": n * n_flow * (48 + 128 + 128),
                "trace_plonk": n * (1 << lp) * (12 + 48 + 48), "trace_poseidon": n * n_pad * (128 + 1152)}
        print(json.dumps({"fixture": args.fixture, "proofs": n, "rows": n_rows, "padded_rows": 1 << lp, "invocations": n_flow,
                          "n_vars": wp.n_vars, "steps": args.steps,
                          "ms_median": {k: round(v, 4) for k, v in med.items()},
                          "ms_min": {k: round(float(np.min(v)), 4) for k, v in times.items()},
                          "ms_max": {k: round(float(np.max(v)), 4) for k, v in times.items()},
                          "GBps_needed_bytes": {k: round(need[k] / med[k] / 1e6, 1) for k in med}}), flush=True)
        del src, d_vars, d_flow, d_swap, plonk, poseidon
    circ.close()
    wp.close()
    ctx.close()


if __name__ == "__main__":
    main()
