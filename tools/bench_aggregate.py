#!/usr/bin/env python3
"""What aggregation costs: rsv_witness_eval_groups_dev + rsv_witness_trace_groups_dev against the same-proof calls, one
JSON line.

    python tools/bench_aggregate.py --fixture level10-1.bin --other level11-1.bin --copies 2 --groups 1,16,256 --steps 5

A group is `--copies` proofs, alternately the fixture and `--other` (one shape, one configuration), under the program built
from the fixture.  Per number of groups g, three times, interleaved (chain_bench.time_interleaved, HIP events on the
context's stream):
  grouped   witness_groups + witness_trace_groups on g * copies proofs: one circuit per group, every copy its own proof;
  same      witness + witness_trace with the same program on g proofs: one circuit per proof, every copy that proof;
  hints     the verifying pass alone (rsv_verify_hints_dev, the hint outputs the witness reads) on the g * (copies - 1)
            proofs the grouped call verifies beyond those g.
The grouped call verifies `copies` times as many proofs, so the expectation is grouped ~ same + hints; `extra_ms` is what
is left over (grouped - same - hints).  A verifying pass has a fixed cost that `hints` pays a second time, so the tool also
times the pass on all g * copies members and on g proofs: `marginal_hints_ms` is their difference, what the extra proofs
cost inside ONE pass, and `extra_marginal_ms` = grouped - same - marginal_hints."""
import argparse
import json

import numpy as np
from chain_bench import open_fixture, time_interleaved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fixture", default="level10-1.bin")
    ap.add_argument("--other", default="level11-1.bin")
    ap.add_argument("--copies", type=int, default=2)
    ap.add_argument("--groups", default="1,16,256")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    rsv, proof, cfg, inputs = open_fixture(args)
    import torch
    import bench
    other = bench.read_fixture(args.other)
    m = args.copies
    wp = rsv.WitnessProgram.build(proof, cfg, inputs, copies=m)
    lp, lq = wp.trace_sizes()
    n_ops, F, s = max(len(wp.gates()[1]), 1), wp.shape.flow_count, wp.shape
    M = max(s.log_size_plonk + 1, s.log_size_poseidon + 2) + s.log_blowup
    dev = torch.device("cuda:0")
    ctx = rsv.Context(0)

    def upload(batch):
        blob, offsets = rsv.pack(batch)
        return torch.from_numpy(blob.copy()).to(dev), torch.from_numpy(offsets.astype(np.int64)).to(dev)

    def i32(*shape):
        return torch.empty(shape, dtype=torch.int32, device=dev)

    def u8(*shape):
        return torch.zeros(shape, dtype=torch.uint8, device=dev)

    results = []
    for g in (int(x) for x in args.groups.split(",")):
        members = [proof if c % 2 == 0 else other for _ in range(g) for c in range(m)]
        b_members, b_same, b_extra = upload(members), upload([proof] * g), upload(members[:g * (m - 1)] or [proof])
        n_extra = g * (m - 1)
        d_vars, d_plonk, d_pos, d_ops = i32(g, wp.n_vars, 4), i32(g, 12, 1 << lp), i32(g, 48, 1 << lq), i32(g, n_ops)
        d_flow, d_swap, d_acc, d_macc = i32(g, m, F, 32), u8(g, m, F), u8(g), u8(g, m)
        d_acc1, d_hacc = u8(g), u8(max(n_extra, 1))
        d_tc, d_fc = i32(g * m, 4, s.n_queries, 64), i32(g * m, 1 + s.n_inner, s.n_queries, 3, 8)
        hint = dict(shape=(s.n_queries, M, s.n_inner), d_trace_cols=i32(max(n_extra, 1), 4, s.n_queries, 64),
                    d_fri_cols=i32(max(n_extra, 1), 1 + s.n_inner, s.n_queries, 3, 8), d_flow=d_flow.view(g * m, F, 32)[:max(n_extra, 1)],
                    d_flow_swap=d_swap.view(g * m, F)[:max(n_extra, 1)])

        def grouped():
            ctx.witness_groups(wp, *b_members, g, d_vars, d_acc, d_macc, inputs=inputs, d_flow=d_flow, d_flow_swap=d_swap)
            ctx.witness_trace_groups(wp, d_vars, d_acc, g, d_plonk=d_plonk, d_poseidon=d_pos, d_ops=d_ops, d_flow=d_flow, d_flow_swap=d_swap)

        def same():
            flow, swap = d_flow.view(g * m, F, 32)[:g], d_swap.view(g * m, F)[:g]
            ctx.witness(wp, *b_same, g, d_vars, d_acc1, inputs=inputs, d_flow=flow, d_flow_swap=swap)
            ctx.witness_trace(wp, d_vars, d_acc1, g, d_plonk=d_plonk, d_poseidon=d_pos, d_ops=d_ops, d_flow=flow, d_flow_swap=swap)

        def hints():
            if n_extra:
                ctx.verify_hints(*b_extra, n_extra, d_hacc, cfg=cfg, inputs=inputs, **hint)

        def hints_of(batch, n):  # the same pass with the same outputs on the first n proofs of a batch
            big = dict(hint, d_trace_cols=d_tc, d_fri_cols=d_fc, d_flow=d_flow.view(g * m, F, 32), d_flow_swap=d_swap.view(g * m, F))
            ctx.verify_hints(*batch, n, d_macc.view(-1), cfg=cfg, inputs=inputs, **big)

        grouped()
        same()
        ctx.synchronize()
        if not (d_acc.cpu().numpy().all() and d_macc.cpu().numpy().all() and d_acc1.cpu().numpy().all()):
            raise SystemExit("verdict mismatch")
        times, med = time_interleaved(ctx, {"grouped": grouped, "same": same, "hints": hints, "hints_members": lambda: hints_of(b_members, g * m),
                                            "hints_same": lambda: hints_of(b_same, g)}, args.steps, args.warmup)
        marginal = med["hints_members"] - med["hints_same"]
        results.append({"groups": g, "proofs": g * m, "grouped_ms": med["grouped"], "same_ms": med["same"], "hints_ms": med["hints"],
                        "extra_ms": med["grouped"] - med["same"] - med["hints"], "marginal_hints_ms": marginal,
                        "extra_marginal_ms": med["grouped"] - med["same"] - marginal,
                        "spread_ms": {k: [float(min(v)), float(max(v))] for k, v in times.items()}})
    last = results[-1]
    print(json.dumps({
        "metric": "aggregated_proofs_per_s", "value": last["proofs"] / (last["grouped_ms"] * 1e-3), "unit": "proofs/s", "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": last["grouped_ms"], "higher_is_better": True, "dtype": "u32 (M31)",
        "data": "synthetic",
        "config": {"workload": f"witness + trace of groups of {m}: {args.fixture}, {args.other}", "copies": m, "n_vars": wp.n_vars,
                   "log_plonk": lp, "log_poseidon": lq},
        "results": results, "kernel_sources_sha": bench.kernel_sources_sha()}))


if __name__ == "__main__":
    main()
