#!/usr/bin/env python3
"""rsv_circuit_eval_dev in both launch forms beside the two things it is made of, in one session: the fixture's own recursion
circuit (default level10-1.bin) as a CREATED evaluation program — its instructions turned into hints, everything that reads
the proof an INPUT taken from the built program's own vector, as tests/test_circuit_eval_gpu.py does — for 1, 16 and 1 024
witnesses.  Beside it rsv_witness_eval_dev on the same batch (the same variables, with the permutations taken from a
verifying pass instead of run in order) and rsv_circuit_flow_dev (the same permutations per witness with no dependencies
between them: the floor for the Poseidon part).  Times are HIP events on the context's stream around each call, interleaved
(tools/chain_bench.py).  First the program's level count and the per-level split of instructions and invocations, then one
JSON line per batch size.

    python tools/bench_circuit_eval.py [--fixture level10-1.bin] [--sizes 1,16,1024] [--steps 20] [--warmup 3]"""
import argparse
import json

import numpy as np

import chain_bench as CB

W_COPY, W_CINV, W_BIT, W_FLOW = 4, 8, 10, 11


def hints_of_program(instr, variables):
    """The built program's instructions as (hints, inputs): hint ops to their kinds, reads of a permutation's output left
    to the definition rule, every other read an INPUT with the value `variables` holds."""
    hints, inputs = [], []
    for op, dst, a, _b, i0, i1, _i2, _i3 in np.asarray(instr).tolist():
        if op < W_COPY or (op == W_FLOW and (i1 >> 2) >= 4):
            continue
        if op <= W_BIT:
            hints.append((dst, op - W_COPY + 1, a, i0 if op >= W_CINV else 0))
        else:
            hints.append((dst, 0, 0, len(inputs)))
            inputs.append(variables[dst])
    return np.array(hints, np.uint32), np.array(inputs, np.uint32)


def main():
    ap = argparse.ArgumentParser()
    CB.add_args(ap, "level10-1.bin", 1)
    ap.add_argument("--sizes", default="1,16,1024")
    ap.set_defaults(steps=20, warmup=3)
    args = ap.parse_args()
    import torch
    rsv, proof, cfg, inputs = CB.open_fixture(args)
    if rsv.device_count() < 1:
        raise SystemExit("bench_circuit_eval needs a HIP device")
    wp = rsv.WitnessProgram.build(proof, cfg, inputs)
    gates, ops = wp.gates()
    prog = wp.export()
    wires = np.ascontiguousarray(prog.flow_wires, dtype=np.uint32)
    ctx = rsv.Context(0)
    one = rsv.Chain(ctx, wp, 1, args.log_blowup)
    one.witness([proof], inputs)
    ctx.synchronize()
    variables = one._vars.cpu().numpy().view(np.uint32)[0]
    flow = one._flow.cpu().numpy().view(np.uint32)[0]
    hints, free = hints_of_program(prog.instr, variables)
    circ = rsv.Circuit(gates, wires, wp.n_vars, 3, ops, hints=hints, n_inputs=len(free))
    n_inputs, n_levels, n_instr = circ.eval_info()
    _, levels, _, flevels = circ.eval_export()
    per_i, per_f = np.diff(levels.astype(np.int64)), np.diff(flevels.astype(np.int64))
    print(json.dumps({"fixture": args.fixture, "n_vars": wp.n_vars, "inputs": n_inputs, "levels": n_levels, "instructions": n_instr,
                      "invocations": len(wires), "levels_with_invocations": int((per_f > 0).sum()),
                      "widest_level": {"instructions": int(per_i.max()), "invocations": int(per_f.max())},
                      "instructions_per_level": per_i.tolist(), "invocations_per_level": per_f.tolist()}), flush=True)
    flow_in = flow.copy()
    flow_in[:, 16:] = 0
    for h in range(2):
        flow_in[wires[:, h] != 0, 8 * h:8 * h + 8] = 0
    n_flow = len(wires)
    for n in (int(x) for x in args.sizes.split(",")):
        src = rsv.Chain(ctx, wp, n, args.log_blowup)
        src.witness([proof] * n, inputs)
        ctx.synchronize()
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a, (n,) + a.shape)).view(np.int32)).to("cuda:0")
        d_in, d_flow = dev(free), dev(flow_in)
        d_vars = torch.zeros((n, wp.n_vars, 4), dtype=torch.int32, device="cuda:0")
        d_swap = torch.zeros((n, n_flow), dtype=torch.uint8, device="cuda:0")
        ok = torch.ones(n, dtype=torch.uint8, device="cuda:0")
        bad = torch.zeros(n, dtype=torch.int32, device="cuda:0")

        def evaluate(form):
            def call():
                ctx.set_option("circuit_eval_form", form)
                ctx.circuit_eval(circ, d_in, n, d_vars, d_flow, d_swap, ok, bad)
                ctx.set_option("circuit_eval_form", "auto")
            return call
        calls = {
            "circuit_eval_per_level": evaluate("per_level"),
            "circuit_eval_walk": evaluate("walk"),
            "witness_eval": lambda: ctx.witness(wp, *src._blob, n, src._vars, src.acc, inputs=inputs, d_flow=src._flow, d_flow_swap=src._swap),
            "circuit_flow": lambda: ctx.circuit_flow(circ, src._vars, n, src._flow, src._swap, ok, bad),
        }
        times, med = CB.time_interleaved(ctx, calls, args.steps, args.warmup)
        ctx.synchronize()
        assert ok.cpu().numpy().all() and torch.equal(d_vars, src._vars) and torch.equal(d_flow, src._flow) and torch.equal(d_swap, src._swap), \
            "the evaluation does not reproduce the built program's witness"
        print(json.dumps({"fixture": args.fixture, "witnesses": n, "steps": args.steps,
                          "ms_median": {k: round(v, 4) for k, v in med.items()},
                          "ms_min": {k: round(float(np.min(v)), 4) for k, v in times.items()},
                          "ms_max": {k: round(float(np.max(v)), 4) for k, v in times.items()}}), flush=True)
        del src, d_in, d_flow, d_vars, d_swap
    circ.close()
    wp.close()
    ctx.close()


if __name__ == "__main__":
    main()
